"""Co-training rollouts in the engine's fused launch (``sumo_rollout_steps_pair``, POLICY 16) against the
step-by-step path they replace -- ``ppo_mixed_pair_step`` + ``sumo_step`` + ``ppo_post_step`` per step -- bit for bit: whole rollouts of
``co_train.PairRunner(engine_fused=True)`` on the mixed match-ups of every nv, episode ends inside a launch, the launch called directly
with full records, its failure path and argument errors, and ``co_train.learn(fused_rollout=True)``."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import has_gpu

pytestmark = pytest.mark.gpu
if has_gpu():
    import torch
    from robosumo_selfplay_amd import capi, co_train, mixed, mjcf, policies, ppo_capi
    from robosumo_selfplay_amd.model import PPOModel
    from robosumo_selfplay_amd.vec_env import SumoVecEnv

ANT_BUG = "RoboSumo-Ant-vs-Bug-v0"
SHARED = ("rew", "ep_done", "ep_r", "ep_l")


def _dims(env):
    return list(zip(env.model.obs_dims, env.model.act_dims))


def _models(dims, seed=5):
    np.random.seed(seed)
    out = []
    for s, (D, A) in enumerate(dims):
        m = PPOModel(policy=policies.PolicySpec(D, A, value_network="copy", activation="relu"), ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5,
                     trainable=False)
        m.act_model.seed(100 + 17 * s)
        out.append(m)
    return out


def _frozen(dims, seed=9):
    rng = np.random.default_rng(seed)
    return [(0.1 * rng.standard_normal(ppo_capi.lib().ppo_param_count(D, A))).astype(np.float32) for D, A in dims]


def _run(env_id, N, T, groups, nroll, prepare=None, **runner_kw):
    """``nroll`` rollouts of a PairRunner whose frozen rows differ from the live ones (as tests/test_gpu_co_train.py builds them);
    ``prepare(env)`` runs after the runner's reset.  Returns what the comparisons read, the env closed."""
    env = SumoVecEnv(env_id, num_envs=N, seed=3, groups=groups)
    dims = _dims(env)
    r = co_train.PairRunner(env, _models(dims), T, 0.995, 0.95, anneal_bound=10, **runner_kw)
    for s, v in enumerate(_frozen(dims)):
        r.set_frozen(s, v)
    if prepare is not None:
        prepare(env)
    outs = [r.run(u + 1) for u in range(nroll)]
    torch.cuda.synchronize()
    state = {k: getattr(env, k).clone() for k in ("obs_dev", "done_dev", "act_dev", "ep_r_dev", "ep_l_dev")}
    env.close()
    return outs, r.last_buffers, state


def _assert_same_rollout(a, b):
    assert len(a) == len(b) == 15
    for k, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, tuple):
            assert torch.equal(x[0], y[0]) and x[1] is None and y[1] is None, k
        elif x is None:
            assert y is None, k
        elif torch.is_tensor(x):
            assert torch.equal(x, y), k
        else:
            assert list(x) == list(y), k                        # the episode records


def _assert_launch_equals_steps(env_id, N, T, groups, nroll, prepare=None, rollout_chunk=0):
    f, bf, sf = _run(env_id, N, T, groups, nroll, prepare, engine_fused=True, rollout_chunk=rollout_chunk)
    d, bd, sd = _run(env_id, N, T, groups, nroll, prepare, fused=True)
    for u in range(nroll):
        for side in range(2):
            _assert_same_rollout(f[u][side], d[u][side])
    for k in sf:
        assert torch.equal(sf[k], sd[k]), k
    for k in SHARED:
        assert torch.equal(bf[k], bd[k]), k
    for side in range(2):
        own = co_train.own_envs(N, side)
        other = co_train.own_envs(N, 1 - side)
        for k in ("obs", "act", "val", "nlp", "done", "noise"):
            assert torch.equal(bf["side"][side][k][:, own], bd["side"][side][k][:, own]), (side, k)
        for k in ("obs", "act", "val", "nlp", "done"):            # the half nobody trains on is left alone: exactly zero
            assert not bool(bf["side"][side][k][:, other].any()), (side, k)
            assert bool(bd["side"][side][k][:, other].float().abs().sum() > 0) or k == "done", (side, k)
    return bf, f


@pytest.mark.parametrize("env_id", [ANT_BUG, "RoboSumo-Bug-vs-Ant-v0", "RoboSumo-Bug-vs-Spider-v0", "RoboSumo-Ant-vs-Spider-v0"])
def test_launch_equals_the_pair_step_path(env_id):
    """Two consecutive rollouts at N = 32, T = 6: nv 32 with D0 < D1, its mirror, nv 40 and nv 36."""
    _assert_launch_equals_steps(env_id, 32, 6, 1, 2)


def test_chunked_launches_on_two_groups():
    """Launches of 2 steps on two env groups: the hand-over between launches, and a non-zero env_offset in the tile index."""
    _assert_launch_equals_steps(ANT_BUG, 64, 6, 2, 2, rollout_chunk=2)


def test_every_env_ends_at_every_step():
    """adjust_z = -10: every agent reports a torso below the lose threshold, so every episode ends at every step and the launch resets
    every env between any two of its steps."""
    bf, _ = _assert_launch_equals_steps(ANT_BUG, 32, 6, 1, 1, prepare=lambda env: env.set_adjust_z(-10.0))
    assert bool(bf["ep_done"].all())
    for side in range(2):
        assert bool(bf["side"][side]["done"][1:, co_train.own_envs(32, side)].all())


def _agent0_outside(model, N, envs):
    """(qpos, qvel, warm, counters) of the oracle's reset state with agent 0's torso at x = 2.7 -- beyond the tatami's edge -- in ``envs``,
    after checking on the CPU that exactly these envs end at their first step."""
    from oracle.oracle import OracleSim
    sim = OracleSim(model, N)
    sim.reset(seeds=np.uint64(3) + np.arange(N, dtype=np.uint64))
    q, v, w, c = sim.get_state()
    q[envs, int(model.agent_qposadr[0])] = 2.7
    sim.set_state(q, v, w, c)
    _, _, done, _, _, _ = sim.step(np.zeros((N, 2, sim.act_stride), np.float32))
    want = np.zeros(N, bool)
    want[envs] = True
    assert done[:, 0].astype(bool).tolist() == want.tolist() and done[:, 1].astype(bool).tolist() == want.tolist()
    return q, v, w, c


def test_one_tile_ends_inside_the_launch():
    """Agent 0 placed outside the tatami in tile 0 only: set and clear done flags meet in one launch."""
    N = 32
    state = _agent0_outside(mjcf.load_model(ANT_BUG), N, slice(0, 16))

    def prepare(env):
        torch.cuda.synchronize()
        env.engine.set_state(*state)

    bf, _ = _assert_launch_equals_steps(ANT_BUG, N, 6, 1, 1, prepare=prepare)
    ep = bf["ep_done"].bool()
    assert bool(ep[0, :16].all()) and not bool(ep[0, 16:].any())
    own0 = bf["side"][0]["done"][:, co_train.own_envs(N, 0)]      # tile 0 is learner 0's: its own done record holds both values
    assert not bool(own0[0].any()) and bool(own0[1].all())
    assert bool((bf["ep_l"][0, :16] == 1).all())


def _full_record_setup(env_id, N, T):
    env = SumoVecEnv(env_id, num_envs=N, seed=7)
    dims = _dims(env)
    models = _models(dims)
    seats = []
    for s, (m, v) in enumerate(zip(models, _frozen(dims))):
        table = torch.stack([m.params, torch.from_numpy(v).to(env.device)]).contiguous()
        seats.append(mixed.LearnerSeat(dims[s][0], dims[s][1], device=env.device, table=table))
    g = torch.Generator(device=env.device)
    g.manual_seed(11)
    f32 = torch.float32
    B = dict(rew=torch.zeros((2, T, N), dtype=f32, device=env.device), ep_done=torch.zeros((T, N), dtype=torch.uint8, device=env.device),
             ep_r=torch.zeros((T, N), dtype=torch.float64, device=env.device), ep_l=torch.zeros((T, N), dtype=torch.int32, device=env.device), side=[])
    for D, A in dims:
        B["side"].append(dict(obs=torch.zeros((T, N, D), dtype=f32, device=env.device), act=torch.zeros((T, N, A), dtype=f32, device=env.device),
                              val=torch.zeros((T, N), dtype=f32, device=env.device), nlp=torch.zeros((T, N), dtype=f32, device=env.device),
                              done=torch.zeros((T, N), dtype=torch.uint8, device=env.device),
                              noise=torch.randn((T, N, A), generator=g, device=env.device, dtype=f32)))
    env.reset_device()
    env.done_dev.zero_()
    return env, seats, B


def _pair_struct(env, seats, B, T, tile_rows=(None, None), record_row=-1, s0=0, K=None):
    ro = capi.RolloutPair()
    for s, (seat, b) in enumerate(zip(seats, B["side"])):
        p = ro.side[s]
        p.table, p.tile_row = seat.table.data_ptr(), None if tile_rows[s] is None else tile_rows[s].data_ptr()
        p.nrows, p.row_stride, p.ob_dim, p.ac_dim, p.record_row = len(seat), int(seat.table.stride(0)), seat.ob_dim, seat.ac_dim, record_row
        p.noise, p.obs, p.act, p.val, p.nlp, p.done = (b[k].data_ptr() for k in ("noise", "obs", "act", "val", "nlp", "done"))
    ro.T, ro.Ntot, ro.env_offset, ro.s0, ro.K, ro.alpha = T, env.num_envs, 0, s0, T if K is None else K, 0.75
    ro.rew, ro.ep_done, ro.ep_r, ro.ep_l = (B[k].data_ptr() for k in SHARED)
    return ro


@pytest.mark.parametrize("env_id", [ANT_BUG, "RoboSumo-Ant-vs-Ant-v0"], ids=["mixed", "homogeneous"])
def test_record_everywhere_equals_a_pair_step_loop(env_id):
    """``record_row = -1`` through ``Engine.rollout_steps_pair`` at N = 16: all records are written everywhere and equal a loop of
    ``pair_step`` with full records, ``step_device`` and ``ppo_post_step``.  A homogeneous scene is a valid one (equal widths)."""
    N, T = 16, 5
    env, seats, B = _full_record_setup(env_id, N, T)
    env.rollout_steps_pair_group(0, _pair_struct(env, seats, B, T))
    st = env.engine.rollout_status()
    assert st["aborted"] == 0 and st["tickets"] == N * T
    env2, seats2, B2 = _full_record_setup(env_id, N, T)
    L = ppo_capi.lib()
    for s in range(T):
        records = tuple({k: b[k][s] for k in mixed.RECORD_KEYS} for b in B2["side"])
        co_train.pair_step(env2, seats2, None, tuple(b["noise"][s] for b in B2["side"]), records, True)
        env2.step_device(env2.act_dev)
        ppo_capi.chk(L.ppo_post_step(env2.info_dev.data_ptr(), N, 0.75, B2["rew"][0, s].data_ptr(), T * N, env2.done_dev.data_ptr(),
                                     env2.ep_r_dev.data_ptr(), env2.ep_l_dev.data_ptr(), B2["ep_done"][s].data_ptr(), B2["ep_r"][s].data_ptr(),
                                     B2["ep_l"][s].data_ptr(), env2._stream()))
    torch.cuda.synchronize()
    for k in SHARED:
        assert torch.equal(B[k], B2[k]), k
    for side in range(2):
        for k in ("obs", "act", "val", "nlp", "done"):
            assert torch.equal(B["side"][side][k], B2["side"][side][k]), (side, k)
        assert bool(B["side"][side]["val"].abs().min() > 0) and bool(B["side"][side]["nlp"].abs().min() > 0)
    for k in ("obs_dev", "done_dev", "act_dev", "ep_r_dev", "ep_l_dev", "info_dev"):
        assert torch.equal(getattr(env, k), getattr(env2, k)), k
    env.close()
    env2.close()


def test_a_tile_row_outside_the_table_fails_the_launch():
    """A ``tile_row`` entry equal to ``nrows`` raises the launch's abort flag: ``rollout_status`` raises (row 0 plays, nothing faults)."""
    N, T = 32, 2
    env, seats, B = _full_record_setup(ANT_BUG, N, T)
    rows = (torch.tensor([0, 2], dtype=torch.int32, device=env.device), None)
    env.rollout_steps_pair_group(0, _pair_struct(env, seats, B, T, tile_rows=rows))
    with pytest.raises(capi.SumoHipError, match="-20"):
        env.engine.rollout_status()
    env.close()


def test_argument_errors_return_their_code_before_a_launch():
    N, T = 32, 4
    env, seats, B = _full_record_setup(ANT_BUG, N, T)
    rows = tuple(torch.zeros(N // 16, dtype=torch.int32, device=env.device) for _ in range(2))
    L = capi.lib()
    ptrs = env.env_ptrs(0)
    assert env.engine.rollout_status()["tickets"] == 0

    def rc(change, tile_rows=(None, None)):
        ro = _pair_struct(env, seats, B, T, tile_rows=tile_rows)
        change(ro)
        code = L.sumo_rollout_steps_pair(env.engine.h, C.byref(ro), *ptrs, None)
        return code, L.sumo_last_error().decode()

    def setf(path, value):
        def change(ro):
            obj = ro
            for name in path[:-1]:
                obj = obj[name] if isinstance(name, int) else getattr(obj, name)
            setattr(obj, path[-1], value)
        return change

    cases = [(setf(("K",), T + 1), -5, "steps [0, 5)"), (setf(("s0",), -1), -5, "steps [-1"), (setf(("Ntot",), N - 1), -6, "envs [0, 32)"),
             (setf(("side", 1, "ob_dim"), 121), -4, "side 1: ob_dim 121"), (setf(("side", 0, "ac_dim"), 12), -4, "side 0: ob_dim 121 / ac_dim 12"),
             (setf(("side", 0, "nrows"), 0), -7, "side 0: nrows 0"), (setf(("side", 1, "row_stride"), 100), -17, "side 1: row_stride 100"),
             (setf(("side", 1, "table"), None), -13, "side 1: missing parameter table"), (setf(("side", 0, "noise"), None), -14, "side 0: missing noise"),
             (setf(("side", 0, "val"), None), -15, "side 0: missing record"), (setf(("side", 1, "done"), None), -15, "side 1: missing record"),
             (setf(("ep_r",), None), -2, "missing buffer")]
    for change, code, msg in cases:
        got, text = rc(change)
        assert got == code and msg in text, (code, got, text)

    def off_grid(ro):
        ro.env_offset, ro.Ntot = 8, N + 16
    got, text = rc(off_grid, tile_rows=rows)
    assert got == -11 and "side 0: a table row per 16-env tile" in text
    ro = _pair_struct(env, seats, B, T)
    assert L.sumo_rollout_steps_pair(env.engine.h, None, *ptrs, None) == -1
    assert L.sumo_rollout_steps_pair(env.engine.h, C.byref(ro), None, *ptrs[1:], None) == -1
    assert env.engine.rollout_status()["tickets"] == 0           # none of the refused calls launched anything
    env.close()
    env = SumoVecEnv(ANT_BUG, num_envs=N, seed=7, cfrc_mode="rne_post")
    code = L.sumo_rollout_steps_pair(env.engine.h, C.byref(ro), *env.env_ptrs(0), None)
    assert code == -12 and "cfrc_mode rne_post" in L.sumo_last_error().decode()
    with pytest.raises(ValueError, match="engine_fused=False"):
        co_train.PairRunner(env, [None, None], 4, 0.99, 0.95, engine_fused=True)
    env.close()


def _learn(log, fused_rollout):
    env = SumoVecEnv(ANT_BUG, num_envs=32, seed=1)
    try:
        co_train.learn(env=env, seed=4, opponent_mode="latest", log_dir=log, log_interval=1, value_network="copy", num_hidden=64,
                       activation="relu", total_timesteps=3 * 16 * 8, nsteps=8, nminibatches=2, noptepochs=1, verbose=False,
                       fused_rollout=fused_rollout)
    finally:
        env.close()
    out = {}
    for s in range(2):
        ck = os.path.join(log, "agent%d" % s, "checkpoints")
        assert sorted(os.listdir(ck)) == ["00000", "00001", "00002", "00003"]
        for f in sorted(os.listdir(ck)):
            out[(s, f)] = open(os.path.join(ck, f), "rb").read()
    return out


def test_learn_writes_the_same_checkpoints(tmp_path):
    fused = _learn(os.path.join(str(tmp_path), "fused"), True)
    steps = _learn(os.path.join(str(tmp_path), "steps"), False)
    assert fused == steps and fused[(0, "00000")] != fused[(0, "00003")] and fused[(1, "00000")] != fused[(1, "00003")]
