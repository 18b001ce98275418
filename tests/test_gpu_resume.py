"""Resuming on the GPU: the engine's snapshot replays the following steps bit for bit -- on the same env and on
a freshly built one, through resets, the time limit, the contact-force mode and a fused rollout launch -- every load error has its own
message and writes nothing, and a ``learn()`` that is killed and resumed leaves the files of the uninterrupted run.

Everything is compared with ``torch.equal`` / byte equality: the contract is bit-exactness, there is no tolerance to choose.  Shapes:
32 envs (two 16-env tiles, more than one workgroup), 5 + 6 steps; ``learn``: nsteps 8, 4 updates."""
import csv
import dataclasses
import os

import numpy as np
import pytest

from conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch
    from robosumo_selfplay_amd import alg_ppo, capi, mjcf, policies, resume, runlog
    from robosumo_selfplay_amd.model import PPOModel
    from robosumo_selfplay_amd.runner import Runner
    from robosumo_selfplay_amd.vec_env import SumoVecEnv

HERE = os.path.dirname(os.path.abspath(__file__))
ANT, SPIDER, ANT_BUG = "RoboSumo-Ant-vs-Ant-v0", "RoboSumo-Spider-vs-Spider-v0", "RoboSumo-Ant-vs-Bug-v0"
N, PRE, WINDOW = 32, 5, 6
H = 64          # capi.SNAPSHOT_HEADER_BYTES


def _actions(env, nsteps, seed):
    """Fixed pseudo-random actions [nsteps][N][2][act_stride] on the device."""
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.standard_normal((nsteps,) + tuple(env.act_dev.shape)).astype(np.float32)).to(env.device)


def _near_the_time_limit(env):
    """Counters through ``set_state`` so that the time limit (500 steps) falls at another step for every env of a tile of 8: before the
    snapshot, and at every step of the window."""
    for g, E in enumerate(env.engines):
        cnt = E.get_state()[3].copy()
        cnt[:, 0] = 500 - (PRE + WINDOW) + 1 + (np.arange(E.N) % 8)          # the episode ends 11 - e % 8 steps from here
        E.set_state(counters=cnt)


def _window(env, acts, extra=None):
    """WINDOW steps; every output of every step, cloned (and ``extra()`` per step: the contact forces of 'rne_post')."""
    rec = []
    for a in acts:
        out = env.step_device(a)
        rec.append([x.clone() for x in out] + ([extra()] if extra is not None else []))
    torch.cuda.synchronize()
    return rec


def _same(rec_a, rec_b):
    assert len(rec_a) == len(rec_b)
    for s, (xa, xb) in enumerate(zip(rec_a, rec_b)):
        assert len(xa) == len(xb)
        for k, (a, b) in enumerate(zip(xa, xb)):
            assert torch.equal(a, b), "step %d, output %d differs" % (s, k)


def _same_snapshot(a, b):
    for x, y in zip(a["blobs"], b["blobs"]):
        assert x.size == y.size and np.array_equal(x[H:], y[H:])         # the payload bytes
        assert np.array_equal(x[:H], y[:H])                              # and the header with them
    for k in SumoVecEnv._SNAP_BUFFERS:
        assert torch.equal(a[k], b[k]), k
    assert np.array_equal(a["seeds"], b["seeds"]) and a["_needs_seed"] == b["_needs_seed"] and a["adjust_z"] == b["adjust_z"]


def _snapshot_case(make_env, with_cfrc=False):
    """``with_cfrc``: every step also records ``get_cfrc_ext`` (cfrc_mode 'rne_post')."""
    env = make_env()
    cf = (lambda e: (lambda: torch.from_numpy(np.concatenate([E.get_cfrc_ext() for E in e.engines])))) if with_cfrc else (lambda e: None)
    env.reset_device()
    _near_the_time_limit(env)
    acts = _actions(env, PRE + WINDOW, 7)
    for a in acts[:PRE]:
        env.step_device(a)
    snap = env.snapshot()
    first = _window(env, acts[PRE:], cf(env))
    after = env.snapshot()
    # not vacuous: episodes ended inside the window (and not all at once), and the steps changed the state
    ends = torch.stack([r[2][:, 0] for r in first]).bool()
    assert ends.any() and not ends.all(), "no episode ended inside the window"
    assert not np.array_equal(snap["blobs"][0][H:], after["blobs"][0][H:]) and not torch.equal(snap["obs_dev"], after["obs_dev"])
    # the same env, put back
    env.restore(snap)
    _same_snapshot(env.snapshot(), snap)
    _same(_window(env, acts[PRE:], cf(env)), first)
    _same_snapshot(env.snapshot(), after)
    # a freshly built env that loads the first one's snapshot (its tensors from the host, as a state file holds them)
    env2 = make_env()
    env2.reset_device()
    env2.step_device(acts[0])
    env2.restore(resume._host(snap))
    assert env2.adjust_z == env.adjust_z
    _same(_window(env2, acts[PRE:], cf(env2)), first)
    _same_snapshot(env2.snapshot(), after)
    env.close(); env2.close()
    return first


@pytest.mark.parametrize("env_id,static", [(ANT, True), (ANT, False), (SPIDER, True), (ANT_BUG, False)],
                         ids=["ant-static", "ant-dynamic", "spider", "ant-vs-bug"])
def test_snapshot_replays_the_steps(env_id, static, monkeypatch):
    if env_id == ANT and not static:
        monkeypatch.setenv("SUMO_STATIC_LAYOUT", "0")
    kinds = []

    def make():
        env = SumoVecEnv(env_id, num_envs=N, seed=5)
        kinds.append(env.engine.static_layout())
        return env
    _snapshot_case(make)
    assert kinds == [static, static]                                     # the kernels the case is about ran


def test_snapshot_replays_the_reset_stream():
    """adjust_z = -10: every env loses at every step and is re-seeded, so every step of the window draws from the reset stream.  The
    fresh env is built with another adjust_z and takes the snapshot's."""
    made = []

    def make():
        made.append(SumoVecEnv(ANT, num_envs=N, seed=5, adjust_z=-10.0 if not made else 0.0))
        return made[-1]
    env = make()
    env.reset_device()
    acts = _actions(env, PRE + WINDOW, 7)
    for a in acts[:PRE]:
        env.step_device(a)
    snap = env.snapshot()
    first = _window(env, acts[PRE:])
    after = env.snapshot()
    assert all(bool(r[2].all()) for r in first)                          # every env ended at every step
    counts = np.concatenate([E.get_state()[3] for E in env.engines])
    assert (counts[:, 1] == PRE + WINDOW + 1).all() and (counts[:, 0] == 0).all()      # reset_count: one reset, then one per step
    assert not torch.equal(first[0][0], first[1][0])                     # another reset state each time
    env.restore(snap)
    _same(_window(env, acts[PRE:]), first)
    _same_snapshot(env.snapshot(), after)
    env2 = make()
    env2.reset_device()
    env2.restore(resume._host(snap))
    assert env2.adjust_z == -10.0
    _same(_window(env2, acts[PRE:]), first)
    _same_snapshot(env2.snapshot(), after)
    env.close(); env2.close()


def test_snapshot_carries_the_contact_forces():
    """cfrc_mode 'rne_post': the blob also holds the pre-step state and cfrc_ext; ``get_cfrc_ext`` replays with the steps and reads the
    snapshot's forces right after a restore."""
    make = lambda: SumoVecEnv(ANT, num_envs=N, seed=5, cfrc_mode="rne_post")
    first = _snapshot_case(make, with_cfrc=True)
    assert any(bool((r[6] != 0).any()) for r in first)                   # there were contact forces to carry
    env, zero = make(), SumoVecEnv(ANT, num_envs=N, seed=5)
    assert env.engine.snapshot().size > zero.engine.snapshot().size      # state_prev and cfrc_ext ride along
    env.reset_device()
    acts = _actions(env, 3, 1)
    for a in acts:
        env.step_device(a)
    snap, f0 = env.snapshot(), env.engine.get_cfrc_ext()
    env.step_device(acts[0])
    assert not np.array_equal(env.engine.get_cfrc_ext(), f0)
    env.restore(snap)
    assert np.array_equal(env.engine.get_cfrc_ext(), f0)
    env.close(); zero.close()


def _mlp_runner(env, params=None):
    spec = policies.PolicySpec(env.observation_space[0].shape[0], env.action_space[0].shape[0], value_network="copy", activation="relu")
    models = [PPOModel(policy=spec, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, trainable=False) for _ in range(2)]
    for i, m in enumerate(models):
        if params is not None:
            m.params.copy_(params[i])
        m.act_model.seed(100 + i)
    r = Runner(env=env, models=models, nsteps=WINDOW, nagent=2, gamma=0.995, lam=0.95, rho_bar=1.0, c_bar=1.0)
    assert r.fused_ok(), "fused rollout path unavailable"
    return r


def _same_rollout(a, b):
    for k, (x, y) in enumerate(zip(a, b)):
        if torch.is_tensor(x):
            assert torch.equal(x, y), "rollout output %d differs" % k
        else:
            assert x == y, "rollout output %d differs" % k


def test_snapshot_replays_a_fused_rollout_launch():
    """The 6 steps as ONE ``sumo_rollout_steps`` launch of K = 6 through an MLP Runner: the launch writes hand-over tags into the
    counters, which derive from the engine's launch count -- the snapshot carries that too, so the payload bytes agree at the end."""
    np.random.seed(0)
    env = SumoVecEnv(ANT, num_envs=N, seed=5)
    r = _mlp_runner(env)
    r.run(1)                                                             # one launch behind us: tags in the counters, dones from the env
    _near_the_time_limit(env)
    snap, models, rs = env.snapshot(), [resume.model_state(m) for m in r.models], resume.runner_state(r)
    first = r.run(2)
    torch.cuda.synchronize()
    after = env.snapshot()
    ep_done = first[2][0]                                                # agent 0's masks [N * T]
    assert ep_done.any() and not ep_done.all() and len(first[11]) > 0    # episodes ended inside the launch
    assert not np.array_equal(snap["blobs"][0][H:], after["blobs"][0][H:])
    env.restore(snap)
    for m, s in zip(r.models, models):
        resume.apply_model_state(m, s)
    resume.apply_runner_state(r, rs)
    _same_rollout(r.run(2), first)
    _same_snapshot(env.snapshot(), after)
    # a fresh env and Runner (whose engine has made no launch yet)
    env2 = SumoVecEnv(ANT, num_envs=N, seed=5)
    r2 = _mlp_runner(env2, [m.params for m in r.models])
    env2.restore(resume._host(snap))
    for m, s in zip(r2.models, models):
        resume.apply_model_state(m, s)
    resume.apply_runner_state(r2, rs)
    _same_rollout(r2.run(2), first)
    _same_snapshot(env2.snapshot(), after)
    assert env.stats()["rollout_aborts"] == 0 and env2.stats()["rollout_aborts"] == 0
    env.close(); env2.close()


def test_every_load_error_has_its_own_message_and_writes_nothing():
    env = SumoVecEnv(ANT, num_envs=N, seed=5)
    env.reset_device()
    acts = _actions(env, 3, 2)
    env.step_device(acts[0])
    snap = env.snapshot()
    good = snap["blobs"][0]
    others = dict(n=SumoVecEnv(ANT, num_envs=16, seed=5), scene=SumoVecEnv(SPIDER, num_envs=N, seed=5),
                  cfrc=SumoVecEnv(ANT, num_envs=N, seed=5, cfrc_mode="rne_post"))
    for e in others.values():
        e.reset_device()
    magic = good.copy(); magic[3] ^= 0x40
    version = good.copy(); version[8] += 1
    cases = [("another N", others["n"].engine.snapshot(), "taken of 16 envs, this engine has 32"),
             ("another scene", others["scene"].engine.snapshot(), "state rows of another scene"),
             ("rne_post against zero", others["cfrc"].engine.snapshot(), "taken in cfrc_mode 1, this engine is in cfrc_mode 0"),
             ("a byte flipped in the magic", magic, "bad magic"),
             ("another version", version, "version 2, this library reads version 1"),
             ("a short buffer", good[:-8], "bytes with a payload of"),
             ("less than a header", good[:40], "fewer than a header")]
    msgs = []
    for what, blob, msg in cases:
        with pytest.raises(capi.SumoHipError, match=msg) as e:
            env.engine.restore(blob)
        msgs.append(str(e.value))
    assert len(set(msgs)) == len(cases)
    with pytest.raises(capi.SumoHipError, match="taken in cfrc_mode 0, this engine is in cfrc_mode 1"):
        others["cfrc"].engine.restore(good)
    # the env-level refusals, before an engine is asked
    with pytest.raises(ValueError, match="num_envs=32 cannot be restored into one with num_envs=16"):
        others["n"].restore(snap)
    with pytest.raises(ValueError, match="env_id='%s' cannot be restored into one with env_id='%s'" % (ANT, SPIDER)):
        others["scene"].restore(snap)
    with pytest.raises(ValueError, match="cfrc_mode='zero' cannot be restored into one with cfrc_mode='rne_post'"):
        others["cfrc"].restore(snap)
    two = SumoVecEnv(ANT, num_envs=N, seed=5, groups=2)
    with pytest.raises(ValueError, match="groups=1 cannot be restored into one with groups=2"):
        two.restore(snap)
    # nothing was written: the next step is the step after the snapshot
    _same_snapshot(env.snapshot(), snap)
    one = _window(env, acts[1:2])
    env.restore(snap)
    _same(_window(env, acts[1:2]), one)
    for e in list(others.values()) + [two, env]:
        e.close()


def test_a_refusal_from_a_later_group_undoes_the_earlier_groups():
    """Two groups, the second group's blob damaged: the first group's engine has taken its blob by then and gets back what it held."""
    env = SumoVecEnv(ANT, num_envs=N, seed=5, groups=2)
    env.reset_device()
    acts = _actions(env, 4, 3)
    env.step_device(acts[0])
    snap = env.snapshot()
    env.step_device(acts[1])
    env.step_device(acts[2])
    now = env.snapshot()
    assert not np.array_equal(now["blobs"][0][H:], snap["blobs"][0][H:])
    bad = dict(snap, blobs=[snap["blobs"][0], snap["blobs"][1].copy()])
    bad["blobs"][1][2] ^= 0x01
    with pytest.raises(capi.SumoHipError, match="bad magic"):
        env.restore(bad)
    _same_snapshot(env.snapshot(), now)                                  # group 0 included: as before the attempt
    one = _window(env, acts[3:4])
    env.restore(now)
    _same(_window(env, acts[3:4]), one)
    env.restore(snap)                                                    # and the undamaged snapshot still loads
    _same_snapshot(env.snapshot(), snap)
    env.close()


# ---- learn() -------------------------------------------------------------------------------------------------------------------
UPDATES, NSTEPS, KILL_AT = 4, 8, 3
MLP = dict(network="mlp", value_network="copy", num_hidden=64, activation="relu")
LSTM = dict(network="lstm", nlstm=128)
WALL_CLOCK = ("fps", "rollout_s", "update_s")
TIME_COLUMNS = WALL_CLOCK + ("misc/time_elapsed",)


class _Killed(Exception):
    pass


def _golden_file(root, key):
    path = os.path.join(root, key + ".npy")
    if not os.path.exists(path):
        with np.load(os.path.join(HERE, "golden", "zoo_v3_params.npz"), allow_pickle=False) as z:
            np.save(path, z[key])
    return path


def _configs(root):
    zoo_mlp, zoo_lstm = _golden_file(root, "ant-mlp-v3"), _golden_file(root, "ant-lstm-v3")
    return {
        # (learn keywords, env id, env keywords, timestep limit of the training env or None for the scene's own)
        "mlp-ours": (dict(MLP, opponent_mode="ours", lr=lambda f: 1e-3 * f, cliprange=lambda f: 0.1 + 0.1 * f), ANT, {}, 6),
        "mlp-latest-both": (dict(MLP, opponent_mode="latest", use_opponent_data="both"), ANT, {}, None),
        "mlp-fix-zoo-lstm-fused": (dict(MLP, opponent_mode="fix", fix_opponent_path=zoo_lstm, fused_fix_opponent=True), ANT, {}, 6),
        "mlp-fix-league": (dict(MLP, opponent_mode="fix", fix_opponent_path=[zoo_mlp, zoo_lstm]), ANT, {}, 6),
        "lstm-random": (dict(LSTM, opponent_mode="random", nminibatches=4), ANT, {}, 6),
        "lstm-ours-both": (dict(LSTM, opponent_mode="ours", use_opponent_data="both"), ANT, {}, 6),
        "mlp-ours-spider-groups2": (dict(MLP, opponent_mode="ours"), SPIDER, dict(groups=2), 6),
    }


def _learn(cfg, log_dir, **more):
    kw, env_id, env_kw, limit = cfg
    model = mjcf.load_model(env_id)
    if limit is not None:                                                # short episodes: every rollout harvests some
        model = dataclasses.replace(model, timestep_limit=limit)
    env = SumoVecEnv(env_id, num_envs=N, seed=3, model=model, **env_kw)
    args = dict(env=env, seed=3, nagent=2, total_timesteps=N * NSTEPS * UPDATES, log_dir=log_dir, verbose=False, nsteps=NSTEPS, nminibatches=2,
                noptepochs=2, lr=1e-3, gamma=0.995, lam=0.95, rho_bar=1.0, c_bar=1.0, anneal_bound=1000, save_interval=1, log_interval=1,
                run_log=True)
    args.update(kw)
    args.update(more)
    try:
        return alg_ppo.learn(**args)
    finally:
        torch.cuda.synchronize()
        env.close()


_RUNS = {}


def _runs(name, tmp_path_factory):
    """Run A straight through; run B killed by ``update_fn`` at update 3 with a state per update on disk (update 2's is the last), then
    continued by a second ``learn(resume=True)`` on a fresh env with the same arguments.  Once per configuration."""
    if name not in _RUNS:
        root = str(tmp_path_factory.mktemp("resume-" + name))
        cfg = _configs(root)[name]
        a_dir, b_dir = os.path.join(root, "a"), os.path.join(root, "b")
        a = _learn(cfg, a_dir)
        rng_a = np.random.get_state()[1].copy(), torch.get_rng_state().clone()

        def kill(update):
            if update == KILL_AT:
                raise _Killed()
        with pytest.raises(_Killed):
            _learn(cfg, b_dir, resume_interval=1, update_fn=kill)
        assert resume.read_state(b_dir)["update"] == KILL_AT - 1
        assert sorted(os.listdir(os.path.join(b_dir, "checkpoints"))) == ["%.5i" % u for u in range(KILL_AT)]
        seen = []
        b = _learn(cfg, b_dir, resume_interval=1, resume=True, update_fn=seen.append)
        rng_b = np.random.get_state()[1].copy(), torch.get_rng_state().clone()
        assert seen == list(range(KILL_AT, UPDATES + 1))                 # the loop went on after the saved update
        _RUNS[name] = dict(cfg=cfg, root=root, a=a, b=b, a_dir=a_dir, b_dir=b_dir, rng_a=rng_a, rng_b=rng_b)
    return _RUNS[name]


def _same_series(a, b):
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same_series(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def _rows(log_dir):
    with open(os.path.join(log_dir, "progress.csv")) as f:
        return [{k: v for k, v in r.items() if k not in TIME_COLUMNS} for r in csv.DictReader(f)]


def _episodes(log_dir):
    lines = open(os.path.join(log_dir, runlog.MONITOR_FILE)).read().splitlines()
    return [ln.rsplit(",", 1)[0] for ln in lines[2:]]


def _same_run(a, b, a_dir, b_dir):
    names = ["%.5i" % u for u in range(UPDATES + 1)]
    assert sorted(os.listdir(os.path.join(a_dir, "checkpoints"))) == sorted(os.listdir(os.path.join(b_dir, "checkpoints"))) == names
    for n in names:
        with open(os.path.join(a_dir, "checkpoints", n), "rb") as f, open(os.path.join(b_dir, "checkpoints", n), "rb") as g:
            assert f.read() == g.read(), "checkpoint %s differs" % n
    assert torch.equal(a.params, b.params) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v) and a.t == b.t
    ha, hb = a.history, b.history
    assert set(ha) == set(hb)
    for k in ha:
        assert len(ha[k]) == len(hb[k]), k
        if k not in WALL_CLOCK and k != "eval":
            assert _same_series(ha[k], hb[k]), "history[%r] differs" % k
    assert len(ha["lossvals"]) == UPDATES
    ra, rb = _rows(a_dir), _rows(b_dir)
    assert [r["misc/nupdates"] for r in rb] == [str(u) for u in range(1, UPDATES + 1)]      # every update once
    assert ra == rb
    assert _episodes(a_dir) == _episodes(b_dir)


@pytest.mark.parametrize("name", ["mlp-ours", "mlp-latest-both", "mlp-fix-zoo-lstm-fused", "mlp-fix-league", "lstm-random", "lstm-ours-both",
                                  "mlp-ours-spider-groups2"])
def test_killed_and_resumed_equals_straight_through(name, tmp_path_factory):
    r = _runs(name, tmp_path_factory)
    _same_run(r["a"], r["b"], r["a_dir"], r["b_dir"])
    assert np.array_equal(r["rng_a"][0], r["rng_b"][0]) and torch.equal(r["rng_a"][1], r["rng_b"][1])      # the global streams end alike
    if r["cfg"][3] is not None:
        assert len(_episodes(r["a_dir"])) > 0                            # the monitor file had rows to continue
    if name == "mlp-fix-league":
        assert len(r["a"].history["league_tiles"]) == UPDATES and r["a"].history["league_tiles"][1] != r["a"].history["league_tiles"][2]
    st = resume.read_state(r["b_dir"])
    assert st["update"] == UPDATES                                       # written after the last update too
    assert (st["opponent_data"] is not None) == (r["cfg"][0]["opponent_mode"] == "ours")


def test_what_the_killed_process_left_after_the_state_is_cut_off(tmp_path_factory):
    """A state every 2 updates, the kill at update 4: the state on disk is update 2's, and the killed process has left checkpoint 00003,
    update 3's rows of log.txt / progress.csv and its episodes in the monitor file.  The resumed run drops them and writes them again."""
    r = _runs("mlp-ours", tmp_path_factory)
    d_dir = os.path.join(r["root"], "d")

    def kill(update):
        if update == UPDATES:
            raise _Killed()
    with pytest.raises(_Killed):
        _learn(r["cfg"], d_dir, resume_interval=2, update_fn=kill)
    st = resume.read_state(d_dir)
    assert st["update"] == 2 and len(st["run_log"]["rows"]) == 2
    assert "00003" in os.listdir(os.path.join(d_dir, "checkpoints")) and [x["misc/nupdates"] for x in _rows(d_dir)] == ["1", "2", "3"]
    assert len(_episodes(d_dir)) > st["run_log"]["monitor_rows"] > 0     # update 3's episodes are in the file, past the state's count
    d = _learn(r["cfg"], d_dir, resume_interval=2, resume=True)
    _same_run(r["a"], d, r["a_dir"], d_dir)
    assert open(os.path.join(d_dir, "log.txt")).read().count("misc/nupdates") == UPDATES
    assert resume.read_state(d_dir)["update"] == UPDATES


def test_resume_on_an_empty_directory_is_a_plain_run(tmp_path_factory, capsys):
    r = _runs("mlp-ours", tmp_path_factory)
    c_dir = os.path.join(r["root"], "c")
    c = _learn(r["cfg"], c_dir, resume=True)
    assert "resume: no state file %s, starting from update 1" % resume.state_path(c_dir) in capsys.readouterr().out
    _same_run(r["a"], c, r["a_dir"], c_dir)
    assert not os.path.exists(os.path.join(c_dir, "resume"))             # resume_interval 0: no state is written


def test_resume_with_other_arguments_is_refused(tmp_path_factory):
    r = _runs("mlp-ours", tmp_path_factory)
    before = open(resume.state_path(r["b_dir"]), "rb").read()
    with pytest.raises(resume.ResumeError, match=r"nsteps=8; this call has nsteps=16"):
        _learn(r["cfg"], r["b_dir"], resume=True, nsteps=16)
    with pytest.raises(resume.ResumeError, match=r"num_envs=32; this call has num_envs=16"):
        kw, env_id, env_kw, limit = r["cfg"]
        env = SumoVecEnv(env_id, num_envs=16, seed=3)
        try:
            alg_ppo.learn(env=env, seed=3, nagent=2, total_timesteps=N * NSTEPS * UPDATES, log_dir=r["b_dir"], verbose=False, nsteps=NSTEPS,
                          nminibatches=2, noptepochs=2, resume=True, **kw)
        finally:
            env.close()
    assert open(resume.state_path(r["b_dir"]), "rb").read() == before
    assert sorted(os.listdir(os.path.join(r["b_dir"], "checkpoints"))) == ["%.5i" % u for u in range(UPDATES + 1)]
