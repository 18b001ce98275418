#!/usr/bin/env python3
"""One SHA-256 per ``learn()`` configuration of both learners, to compare two commits bit for bit.

    python tools/learn_digest.py [--fields FILE] > digest.txt      # on each commit; the two files must be identical
    python tools/learn_digest.py --refusals > refusals.txt         # no GPU: what learn() refuses before it touches the device

The learn() tests assert finite losses and file names; a rewrite of ``alg_ppo.learn`` / ``alg_ac.learn`` that reorders one random
draw passes them.  This tool anchors such a rewrite against its parent: it drives only the public ``learn(...)`` and prints
``<config> <sha256>`` over ``model.params``, ``model.t``, every ``history`` key but the wall-clock ones, the sorted checkpoint
listing with the parameters read back from every checkpoint, and numpy's and torch's global generator states at the end (the
same number of draws was taken).  ``--fields FILE`` also writes one hash per hashed field, to name the field that differs.

Every configuration: Ant-vs-Ant, 32 envs (two 16-env tiles), nsteps 8 (A2C: 5), 3 updates, 4 minibatches x 2 epochs, a checkpoint
per update, a fresh log directory.  Zoo files are the vectors of tests/golden and the synthetic ones of the GPU tests."""
import contextlib
import hashlib
import io
import os
import re
import struct
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

ANT, N, UPDATES = "RoboSumo-Ant-vs-Ant-v0", 32, 3
WALL_CLOCK = ("fps", "rollout_s", "update_s", "select_s")
MLP = dict(network="mlp", value_network="copy", num_hidden=64, activation="relu")
PPO = dict(nsteps=8, nminibatches=4, noptepochs=2, lr=1e-3, gamma=0.995, lam=0.95, rho_bar=1.0, c_bar=1.0, anneal_bound=1000)
A2C = dict(nsteps=5, lr=1e-3, gamma=0.995, lam=0.95, anneal_bound=1000)
TIMING = re.compile(r"(fps|rollout|sgd|update|evaluation) [0-9.]+(?:e[+-]?[0-9]+)?(m?s)?(?= )")


def configs(zoo):
    """(name, learner, keywords).  ``zoo``: name -> file of a policy-zoo vector; '@name' in load_path: a checkpoint of that run."""
    fix = lambda path, **kw: dict(opponent_mode="fix", fix_opponent_path=path, **kw)
    league = [zoo["mlp"], zoo["lstm-synthetic"]]
    lstm = dict(network="lstm", nlstm=128)
    return [
        ("ppo-mlp-ours", "ppo", dict(MLP, opponent_mode="ours")),
        ("ppo-mlp-ours-fused-selector", "ppo", dict(MLP, opponent_mode="ours", fused_selector=True)),
        ("ppo-mlp-random-pool2", "ppo", dict(MLP, opponent_mode="random", opponent_pool=2)),
        ("ppo-mlp-latest-pool2", "ppo", dict(MLP, opponent_mode="latest", opponent_pool=2)),
        ("ppo-mlp-ours-both-kl10", "ppo", dict(MLP, opponent_mode="ours", use_opponent_data="both", kl_threshold=10.0)),
        ("ppo-mlp-ours-both-earlystop", "ppo", dict(MLP, opponent_mode="ours", use_opponent_data="both", kl_threshold=1e-9)),
        ("ppo-mlp-random-direct-vgap0", "ppo", dict(MLP, opponent_mode="random", use_opponent_data="direct", vgap=0)),
        ("ppo-mlp-fix-step", "ppo", dict(MLP, **fix(zoo["mlp"]))),
        ("ppo-mlp-fix-fused", "ppo", dict(MLP, **fix(zoo["mlp"], fused_fix_opponent=True))),
        ("ppo-mlp-fix-league-fused", "ppo", dict(MLP, **fix(league, fused_fix_opponent=True))),
        ("ppo-mlp-ours-load-path", "ppo", dict(MLP, opponent_mode="ours", load_path="@ppo-mlp-ours/00002")),
        ("ppo-mlp-ours-eval", "ppo", dict(MLP, opponent_mode="ours", run_log=True, eval_interval=1, eval_opponents=["00000"], eval_trials=16,
                                          eval_num_env=16)),
        ("ppo-lstm-ours", "ppo", dict(lstm, opponent_mode="ours")),
        ("ppo-lstm-ours-pool2", "ppo", dict(lstm, opponent_mode="ours", opponent_pool=2)),
        ("ppo-lstm-ours-both", "ppo", dict(lstm, opponent_mode="ours", use_opponent_data="both")),
        ("ppo-lstm-fix-lstm-fused", "ppo", dict(lstm, **fix(zoo["lstm"], fused_fix_opponent=True))),
        ("a2c-ours", "a2c", dict(MLP, opponent_mode="ours")),
        ("a2c-random-pool2", "a2c", dict(MLP, opponent_mode="random", opponent_pool=2)),
        ("a2c-random-direct", "a2c", dict(MLP, opponent_mode="random", use_opponent_data="direct")),
        ("a2c-fix-league", "a2c", dict(MLP, **fix(league, fused_fix_opponent=True))),
        ("ppo-mlp-ours-verbose", "ppo", dict(MLP, opponent_mode="ours", verbose=True, log_interval=1)),
        ("a2c-ours-verbose", "a2c", dict(MLP, opponent_mode="ours", verbose=True, log_interval=1)),
    ]


def feed(h, x):
    """``x`` into hash ``h``, type by type: arrays and tensors as dtype, shape and bytes; floats as their 8 bytes."""
    import numpy as np
    import torch
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    if isinstance(x, (np.ndarray, np.generic)):
        x = np.ascontiguousarray(x)
        h.update(("<%s%s>" % (x.dtype, x.shape)).encode())
        h.update(x.tobytes())
    elif isinstance(x, dict):
        h.update(b"{")
        for k in sorted(x):
            h.update(repr(k).encode())
            feed(h, x[k])
        h.update(b"}")
    elif isinstance(x, (list, tuple)):
        h.update(b"[")
        for y in x:
            feed(h, y)
        h.update(b"]")
    elif isinstance(x, float):
        h.update(b"f" + struct.pack("<d", x))
    else:
        assert x is None or isinstance(x, (bool, int, str)), type(x)
        h.update(repr(x).encode() + b";")


def fields_of(model, log_dir, stdout=None):
    """The hashed fields of a finished run, in a fixed order: (name, value) pairs."""
    import joblib
    import numpy as np
    import torch
    checkdir = os.path.join(log_dir, "checkpoints")
    names = sorted(os.listdir(checkdir))
    out = [("params", model.params), ("t", int(model.t))]
    out += [("history." + k, v) for k, v in sorted(model.history.items()) if k not in WALL_CLOCK and k != "eval"]
    out += [("checkpoints", names)] + [("checkpoint." + n, joblib.load(os.path.join(checkdir, n))) for n in names]
    out += [("numpy_state", list(np.random.get_state())), ("torch_state", torch.random.get_rng_state())]
    if stdout is not None:
        out.append(("stdout", TIMING.sub(lambda m: "%s <t>%s" % (m.group(1), m.group(2) or ""), stdout)))
    return out


def digest(fields, name, fields_file):
    total = hashlib.sha256()
    for key, value in fields:
        one = hashlib.sha256()
        feed(one, value)
        total.update(key.encode() + one.digest())
        if fields_file is not None:
            fields_file.write("%s:%s %s\n" % (name, key, one.hexdigest()))
            fields_file.flush()
    return total.hexdigest()


def run_digests(fields_path):
    import numpy as np
    import torch
    from zoo_lstm_helpers import golden, synthetic_lstm_flat
    from robosumo_selfplay_amd import alg_ac, alg_ppo
    from robosumo_selfplay_amd.vec_env import SumoVecEnv
    if torch.cuda.device_count() < 2:
        print("one GPU visible: no two-rank configuration", file=sys.stderr)
    fields_file = open(fields_path, "w") if fields_path else None
    with tempfile.TemporaryDirectory() as root:
        zoo = {}
        for key, vec in (("mlp", golden("ant-mlp-v3")), ("lstm", golden("ant-lstm-v3")), ("lstm-synthetic", synthetic_lstm_flat(120, 8, 7))):
            zoo[key] = os.path.join(root, "zoo-%s.npy" % key)
            np.save(zoo[key], vec)
        seen = {}
        for name, learner, kw in configs(zoo):
            kw = dict(dict(A2C if learner == "a2c" else PPO, seed=3, nagent=2, save_interval=1, verbose=False), **kw)
            if str(kw.get("load_path", "")).startswith("@"):
                run, ckpt = kw["load_path"][1:].split("/")
                kw["load_path"] = os.path.join(root, run, "checkpoints", ckpt)
            log_dir = os.path.join(root, name)          # fresh per configuration
            env = SumoVecEnv(ANT, num_envs=N, seed=1)
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf if kw["verbose"] else sys.stdout):
                model = (alg_ac if learner == "a2c" else alg_ppo).learn(env=env, total_timesteps=N * kw["nsteps"] * UPDATES, log_dir=log_dir, **kw)
            torch.cuda.synchronize()
            hist = model.history
            assert len(hist["lossvals"]) == UPDATES and len(hist["opponent_versions"]) in (0, UPDATES), name
            if name.endswith("earlystop"):
                assert any(s is not None for s in hist["early_stop_info"]), "the KL early stop did not trigger"
            seen[name] = digest(fields_of(model, log_dir, buf.getvalue() if kw["verbose"] else None), name, fields_file)
            print(name, seen[name], flush=True)
            if "eval" in hist:      # the evaluation leaves training as it was; its own results (less the wall clock) on a line of their own
                assert seen[name] == seen["ppo-mlp-ours"], "evaluation changed the training run"
                ev = [{k: v for k, v in e.items() if k != "seconds"} for e in hist["eval"]]
                assert len(ev) == UPDATES
                print(name + "/eval", digest([("eval", ev)], name + "/eval", fields_file), flush=True)
            env.close()


class DimsOnly(object):
    """An env with dimensions and nothing else: whatever learn() refuses with it, it refuses before it touches the device."""
    cfrc_mode = "zero"

    def __init__(self, num_envs=4, **kw):
        import numpy as np
        from robosumo_selfplay_amd.spaces import Box
        self.observation_space = [Box(-np.ones(121), np.ones(121))] * 2
        self.action_space = [Box(-np.ones(8), np.ones(8))] * 2
        self.num_envs = num_envs
        self.__dict__.update(kw)


def refusal_cases():
    env = DimsOnly()
    ev = dict(eval_interval=1, eval_opponents=["00000"])
    lstm = dict(network="lstm", nminibatches=2)
    return [
        # alg_ppo: the fused selector's checks come first
        ("ppo selector lstm", "ppo", dict(network="lstm", fused_selector=True)),
        ("ppo selector random", "ppo", dict(fused_selector=True, opponent_mode="random")),
        ("ppo selector fix", "ppo", dict(fused_selector=True, opponent_mode="fix")),
        ("ppo selector model_fn", "ppo", dict(fused_selector=True, model_fn=lambda **kw: None)),
        ("ppo selector lstm+random", "ppo", dict(network="lstm", fused_selector=True, opponent_mode="random")),
        ("ppo selector random+eval without interval", "ppo", dict(fused_selector=True, opponent_mode="random", eval_opponents=["00000"])),
        # the evaluation plan
        ("ppo eval cfrc_mode", "ppo", dict(ev, env=DimsOnly(cfrc_mode="rne_post"))),
        ("ppo eval without interval", "ppo", dict(eval_opponents=["00000"])),
        ("ppo eval without opponents", "ppo", dict(eval_interval=1)),
        ("ppo eval_env is env", "ppo", dict(ev, env=env, eval_env=env)),
        ("ppo eval_trials 0", "ppo", dict(ev, eval_trials=0)),
        ("ppo eval opponents string", "ppo", dict(eval_interval=1, eval_opponents="00000")),
        ("ppo eval cfrc_mode+trials 0", "ppo", dict(ev, env=DimsOnly(cfrc_mode="rne_post"), eval_trials=0)),
        ("ppo eval without interval+lstm bad reuse", "ppo", dict(lstm, eval_opponents=["00000"], use_opponent_data="sideways")),
        # the policy
        ("ppo normalize_observations", "ppo", dict(normalize_observations=True)),
        ("ppo lstm value_network copy", "ppo", dict(lstm, value_network="copy")),
        ("ppo lstm value_network copy+bad reuse", "ppo", dict(lstm, value_network="copy", use_opponent_data="sideways")),
        # a recurrent learner
        ("ppo lstm bad reuse", "ppo", dict(lstm, use_opponent_data="sideways")),
        ("ppo lstm reuse fix", "ppo", dict(lstm, use_opponent_data="direct", opponent_mode="fix")),
        ("ppo lstm bad reuse+fix", "ppo", dict(lstm, use_opponent_data="sideways", opponent_mode="fix")),
        ("ppo lstm minibatches", "ppo", dict(lstm, nminibatches=3)),
        ("ppo lstm reuse fix+minibatches", "ppo", dict(lstm, nminibatches=3, use_opponent_data="both", opponent_mode="fix")),
        # alg_ac
        ("a2c lstm", "a2c", dict(network="lstm")),
        ("a2c off_policy", "a2c", dict(use_opponent_data="off_policy")),
        ("a2c both", "a2c", dict(use_opponent_data="both")),
        ("a2c bad reuse", "a2c", dict(use_opponent_data="sideways")),
        ("a2c comm", "a2c", dict(comm=object())),
        ("a2c bad mode", "a2c", dict(opponent_mode="sideways")),
        ("a2c lstm+both", "a2c", dict(network="lstm", use_opponent_data="both")),
        ("a2c comm+bad mode", "a2c", dict(comm=object(), opponent_mode="sideways")),
        ("a2c bad mode+eval cfrc_mode", "a2c", dict(ev, opponent_mode="sideways", env=DimsOnly(cfrc_mode="rne_post"))),
        ("a2c eval cfrc_mode", "a2c", dict(ev, env=DimsOnly(cfrc_mode="rne_post"))),
        ("a2c eval without interval", "a2c", dict(eval_opponents=["00000"])),
        ("a2c eval_env is env", "a2c", dict(ev, env=env, eval_env=env)),
    ]


def run_refusals():
    from robosumo_selfplay_amd import alg_ac, alg_ppo
    for name, learner, kw in refusal_cases():
        args = dict(network="mlp", env=DimsOnly(), total_timesteps=64, nagent=2, nsteps=4, verbose=False)
        args.update(kw)
        try:
            (alg_ac if learner == "a2c" else alg_ppo).learn(**args)
        except (ValueError, NotImplementedError, AssertionError) as e:
            print("%s | %s: %s" % (name, type(e).__name__, e), flush=True)
        else:
            raise SystemExit("%s: learn() returned" % name)


if __name__ == "__main__":
    if "--refusals" in sys.argv[1:]:
        run_refusals()
    else:
        run_digests(sys.argv[sys.argv.index("--fields") + 1] if "--fields" in sys.argv else None)
