#!/usr/bin/env python3
"""One SHA-256 per rollout mode of the device-mode Runner and ``run()`` call, to compare two commits bit for bit.

    python tools/runner_mode_digest.py > modes.txt      # on each commit; the two files must be identical

The fused-vs-stepwise tests compare two paths of ONE commit; a change that rewrites both (a reordered generator draw, a mask wrong
on both) passes them.  This tool anchors a rewrite of ``runner.py`` against its parent: it drives only what both sides have
(``Runner(...)``, its public switches, ``run``) and prints ``<mode> call<k> <sha256>`` over the bytes of every tensor ``run()``
returns, the episode list, every engine's ``get_state()``, ``states[0]``, ``shadow_state``, ``zoo_state`` / the league's
``state`` and ``league_scores``.

Every mode: Ant-vs-Ant, 64 envs (4 tiles of 16), T = 6 in launches of 3 steps, step counters near the time limit so that episodes
end inside the window, two consecutive ``run()`` calls (carried-over states, the noise rows of a second buffer).  Learners and
zoo nets are the builders of tests/test_gpu_zoo_league.py."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

N, T, CHUNK, POOL = 64, 6, 3, 3


def modes():
    """(name, learner, nlstm, opponent, opt-in, groups, fused_rollout, whether a fused launch is expected to apply)."""
    out = []
    for learner in ("mlp", "lstm"):
        for opponent in ("self", "pool", "reuse", "zoo_mlp", "zoo_lstm", "league_mlp", "league_lstm", "league_mixed"):
            if opponent == "reuse" and learner == "mlp":
                continue
            zoo = opponent.startswith("zoo")
            for optin in ((True, False) if zoo else (True,)):
                for fused in (True, False):
                    if (learner, opponent, fused) == ("mlp", "pool", False):      # an MLP pool plays in the fused launch only
                        continue
                    name = "%s-%s%s-%s" % (learner, opponent, "" if optin or not zoo else "-nooptin", "fused" if fused else "step")
                    out.append((name, learner, 128, opponent, optin, 1, fused, fused and optin))
    out.append(("lstm64-self-step", "lstm", 64, "self", True, 1, False, False))
    for learner in ("mlp", "lstm"):
        for opponent in ("self", "league_mixed"):
            for fused in (True, False):
                out.append(("%s-%s-groups2-%s" % (learner, opponent, "fused" if fused else "step"), learner, 128, opponent, True, 2, fused, fused))
    return out


def main():
    os.environ["SUMO_ROLLOUT_CHUNK"] = str(CHUNK)
    import numpy as np
    import torch
    import test_gpu_zoo_league as L
    from zoo_lstm_helpers import golden
    from robosumo_selfplay_amd import opponent_pool, policy_zoo
    from robosumo_selfplay_amd.runner import Runner
    from robosumo_selfplay_amd.vec_env import SumoVecEnv
    assert (L.N, L.T) == (N, T)

    def build(learner, H, opponent, optin, groups, fused):
        env = SumoVecEnv(L.ANT, num_envs=N, seed=11, groups=groups)
        make = (lambda seed: L._lstm_learner(seed, H)) if learner == "lstm" else L._mlp_learner
        models = [make(5), make(6)]
        for k, m in enumerate(models):
            m.act_model.seed(101 + k)
        r = Runner(env=env, models=models, nsteps=T, nagent=2, gamma=0.995, lam=0.95, rho_bar=1.0, c_bar=1.0, anneal_bound=500)
        zoo = None
        if opponent == "pool":
            spec = models[0].spec if learner == "lstm" else models[0].act_model.spec
            pool = (opponent_pool.LstmOpponentPool if learner == "lstm" else opponent_pool.OpponentPool)(spec, POOL, N, env.device)
            for k in range(POOL):
                pool.set_snapshot(k, make(7 + k).act_model.params)
            if learner == "lstm":
                pool.assign([0, 1, 2, 1])
                pool.seed(102)
                r.models[1] = pool
            else:
                pool.assign(np.arange(N) * 5 % POOL)
                r.opponent_pool = pool
        elif opponent == "reuse":
            r.reuse_opponent = True
        elif opponent != "self":
            if opponent.startswith("league"):
                nets = [policy_zoo.load_zoo_policy_from_flat(f, L.A) for f in L._members(opponent[len("league_"):])]
                zoo = policy_zoo.ZooLeague(nets, N, env.device)
            else:
                zoo = policy_zoo.load_zoo_policy_from_flat(golden("ant-mlp-v3" if opponent == "zoo_mlp" else "ant-lstm-v3"), L.A)
            zoo.seed(202)
            r.models[1] = policy_zoo.FixedOpponentModel(zoo)
        r.fused_fix_opponent = optin
        r.fused_rollout = fused
        assert r.rollout_chunk == CHUNK
        return env, r, zoo

    def digest(env, r, zoo, out):
        h = hashlib.sha256()

        def add(x):
            if x is None:
                h.update(b"<none>")
            elif torch.is_tensor(x):
                add(x.cpu().numpy())
            else:
                x = np.ascontiguousarray(x)
                h.update(("%s%s" % (x.dtype, x.shape)).encode())
                h.update(x.tobytes())
        for x in out:
            if torch.is_tensor(x) or x is None:
                add(x)
            else:
                h.update(repr(list(x)).encode())           # the episode records
        for E in env.engines:
            for x in E.get_state():
                add(x)
        add(r.states[0] if torch.is_tensor(r.states[0]) else None)
        add(r.shadow_state)
        add(zoo.state if isinstance(zoo, policy_zoo.ZooLeague) else r.zoo_state)
        add(r.league_scores)
        return h.hexdigest()

    for name, learner, H, opponent, optin, groups, fused, expect in modes():
        env, r, zoo = build(learner, H, opponent, optin, groups, fused)
        applies = bool(r.fused_ok() or r.fused_lstm_ok() or r.fused_zoo_ok() or r.fused_lstm_zoo_ok() or r.fused_league_ok())
        assert applies == expect, (name, applies)
        L._near_time_limit(env)
        for k in range(2):
            out = r.run(250 + k)
            torch.cuda.synchronize()
            assert env.stats()["rollout_aborts"] == 0, name
            print(name, "call%d" % k, digest(env, r, zoo, out), flush=True)
        env.close()


if __name__ == "__main__":
    main()
