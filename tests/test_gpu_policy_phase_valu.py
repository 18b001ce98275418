"""The fused launches' MLP policy phase on the vector ALU (csrc/ppo_tile.h mlp_rows_valu: a lane owns one hidden unit of all of a
step's trunks) against the step-by-step path, whose kernels evaluate the same nets on MFMA tiles (trunk_forward).  The lane's fmaf
chain runs in the tile's accumulation order, so nothing is approximate: every comparison here is bitwise (np.array_equal on the
arrays Runner.run returns -- observations, actions, neglogp, opponent neglogp, values, done masks, rewards -- and on the final env
state)."""
import functools

import numpy as np
import pytest

from conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch
    from robosumo_selfplay_amd import matches, model as model_mod, policies
    from robosumo_selfplay_amd.runner import Runner
    from robosumo_selfplay_amd.vec_env import SumoVecEnv

ANT = "RoboSumo-Ant-vs-Ant-v0"
D, A = 121, 8


def _random_params(seed, scale=0.1):
    rng = np.random.RandomState(seed)
    return [p + rng.normal(0, scale, p.shape).astype(np.float32) for p in policies.init_param_list(D, A, rng)]


def _edge_params(seed, flip):
    """Sums whose value depends on the order of their terms, and the edges of the accumulation: layers scaled by 1e-3 / 1e3 (which
    layer gets which flips between the two nets), biases that leave relu about half of the units, head weights large enough that the
    64 terms of a mean cancel to O(1), a weight row of exact zeros, -0.0 and denormal weights, a large negative bias on one unit."""
    rng = np.random.RandomState(seed)
    pl = policies.init_param_list(D, A, rng)
    lo, hi = (np.float32(1e-3), np.float32(1e3)) if not flip else (np.float32(1e3), np.float32(1e-3))
    for base, (s0, s1) in ((0, (lo, hi)), (4, (hi, lo))):          # policy trunk, value trunk
        w0, b0, w1, b1 = (pl[base + k] for k in range(4))
        w0 *= s0
        b0[:] = (s0 * rng.normal(0, 1.0, b0.shape)).astype(np.float32)
        w1 *= s1
        b1[:] = (s0 * s1 * rng.normal(0, 1.0, b1.shape)).astype(np.float32)
        w0[5, :] = 0.0                                             # a weight row of exact zeros
        w1[7, :] = 0.0
        w0[10, ::3] = -0.0
        w0[11, ::2] = np.float32(1e-40)                            # denormal
        w0[12, 1::2] = np.float32(-1e-40)
        w0[D - 1, ::5] = np.float32(-1e-40)                        # the row behind which the tile pads its k-steps
        w1[3, ::4] = -0.0
        w1[4, 1::4] = np.float32(1e-40)
        b0[9] = np.float32(-1e6) * max(s0, np.float32(1.0))        # a unit relu always kills
        b1[20] = np.float32(-1e6) * max(s0 * s1, np.float32(1.0))
    pl[8] *= np.float32(30.0)                                      # head: 64 terms of either sign that cancel
    pl[8][3, :] = -0.0
    pl[8][6, ::2] = np.float32(1e-40)
    pl[9][:] = rng.normal(0, 0.1, pl[9].shape).astype(np.float32)
    pl[10][:] = rng.normal(-0.5, 0.2, pl[10].shape).astype(np.float32)
    pl[11] *= np.float32(100.0)
    pl[12][:] = np.float32(0.25)
    for p in pl:
        assert np.isfinite(p).all()
    return pl


def _model(plist):
    spec = policies.PolicySpec(D, A, value_network="copy", activation="relu")
    m = model_mod.PPOModel(policy=spec, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, trainable=False)
    m.set_param_list(plist)
    return m


def _host(x):
    return x.cpu().numpy() if torch.is_tensor(x) else x


def _rollout(N, T, fused, learner_pl, opp_pl, chunk=0, pool=None):
    env = SumoVecEnv(ANT, num_envs=N, seed=11)
    learner, opp = _model(learner_pl), _model(opp_pl)
    learner.act_model.seed(101); opp.act_model.seed(202)
    r = Runner(env=env, models=[learner, opp], nsteps=T, nagent=2, gamma=0.995, lam=0.95, rho_bar=1.0, c_bar=1.0, anneal_bound=500)
    r.fused_rollout, r.rollout_chunk = fused, chunk
    if pool is not None:
        r.opponent_pool = pool(learner.spec, N, env.device)
    outs = [[_host(x) for x in r.run(250)], [_host(x) for x in r.run(251)]]   # two rollouts: episode state carries over
    torch.cuda.synchronize()
    st, aborts = env.engine.get_state(), env.stats()["rollout_aborts"]
    env.close()
    assert aborts == 0
    return outs, st


def _assert_same(a, b):
    (ao, ast), (bo, bst) = a, b
    for k, (f, s_) in enumerate(zip(ao, bo)):
        assert len(f) == len(s_)
        for j, (x, y) in enumerate(zip(f, s_)):
            if isinstance(x, np.ndarray):
                assert x.dtype == y.dtype and x.shape == y.shape, (k, j)
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (k, j, np.argwhere(x != y)[:5])
            else:
                assert x == y, (k, j)
    for x, y in zip(ast, bst):
        assert np.array_equal(x, y)


@functools.lru_cache(maxsize=None)
def _case1(fused, rep=0):
    return _rollout(16, 3, fused, _random_params(3), _random_params(4))


def test_small_ant_rollout():
    """Ant-vs-Ant, N = 16, T = 3, one group; learner and opponent carry different random parameters."""
    _assert_same(_case1(True), _case1(False))


def test_order_sensitive_parameters():
    """The same shape with parameters that make the sums order-sensitive and exercise the accumulation's edges (_edge_params)."""
    lp, op = _edge_params(21, False), _edge_params(22, True)
    f, s_ = _rollout(16, 3, True, lp, op), _rollout(16, 3, False, lp, op)
    _assert_same(f, s_)
    val, act = f[0][0][4], f[0][0][3]
    assert np.isfinite(val).all() and np.isfinite(act).all() and np.unique(act).size > act.size // 2   # (the nets still say something)


def test_per_env_opponent_pool():
    """Three snapshots, N = 48, T = 2, the snapshot index changing inside every 16-env tile: env by env the fused rollout equals the
    step-by-step rollout against that env's snapshot alone."""
    from robosumo_selfplay_amd.opponent_pool import OpponentPool
    N, T = 48, 2
    snaps = [torch.from_numpy(policies.flatten_params(_random_params(40 + k, 0.2))) for k in range(3)]
    idx = (np.arange(N) * 7 // 3) % 3
    assert all(np.unique(idx[t:t + 16]).size == 3 for t in range(0, N, 16))

    def pool(spec, n, dev):
        p = OpponentPool(spec, 4, n, dev)
        for k, v in enumerate(snaps):
            p.set_snapshot(k, v.to(dev), label="snap%d" % k)
        p.assign(idx)
        return p
    lp = _random_params(3)
    fo, _ = _rollout(N, T, True, lp, _random_params(4), pool=pool)
    for k in range(3):
        so, _ = _rollout(N, T, False, lp, policies.unflatten_params(snaps[k].numpy(), D, A))
        cols = np.nonzero(idx == k)[0]
        rows = (cols[:, None] * T + np.arange(T)[None, :]).ravel()                           # env-major flattening (sf01)
        for j in (0, 1, 2, 3, 4, 5, 6, 7):
            assert np.array_equal(fo[0][j][:, rows], so[0][j][:, rows]), (k, j)


def test_edge_shapes():
    """N = 17 (fills no 16-env tile), T = 5 split into launches of two steps (a launch boundary inside the rollout)."""
    lp, op = _random_params(5), _random_params(6)
    _assert_same(_rollout(17, 5, True, lp, op, chunk=2), _rollout(17, 5, False, lp, op, chunk=2))


@pytest.mark.parametrize("deterministic", [True, False])
def test_match_mode(deterministic):
    """sumo_match_steps (two policy trunks per step) against the step-by-step match path: N = 16, two launches of six steps."""
    N, K = 16, 6
    ef, es = (SumoVecEnv(ANT, num_envs=N, seed=11, adjust_z=-0.5) for _ in range(2))
    spec = policies.PolicySpec(D, A, value_network="copy", activation="relu")
    table = matches.SnapshotTable(spec, 3, ef.device)
    for j, pl in enumerate((_random_params(30, 0.3), _random_params(31, 0.3), _edge_params(32, False))):
        table.set(j, policies.flatten_params(pl))
    idx0 = (np.arange(N) % 3).astype(np.int32)
    idx1 = ((np.arange(N) // 2) % 3).astype(np.int32)
    assert (idx0 == idx1).any() and (idx0 != idx1).any()
    for e in (ef, es):
        e.reset_device()
    qpos, qvel, warm, cnt = ef.engine.get_state()
    cnt[:, 0] = ef.model.timestep_limit - 8 + (np.arange(N) % 7)   # episodes end (and auto-reset) inside the launches
    for e in (ef, es):
        e.engine.set_state(qpos, qvel, warm, cnt)
    i0, i1 = torch.from_numpy(idx0).cuda(), torch.from_numpy(idx1).cuda()
    sf = torch.zeros((N, 3), dtype=torch.int32, device="cuda")
    ss = torch.zeros_like(sf)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    for chunk in range(2):
        noise = None if deterministic else tuple(torch.randn((K, N, A), generator=gen, device="cuda") for _ in range(2))
        matches.match_steps_fused(ef, table, i0, i1, sf, 2, K, noise)
        matches.match_steps_stepwise(es, table, idx0, idx1, ss, 2, K, noise)
        torch.cuda.synchronize()
        for name, x, y in zip(("obs", "info", "done", "actions"), (ef.obs_dev, ef.info_dev, ef.done_dev, ef.act_dev),
                              (es.obs_dev, es.info_dev, es.done_dev, es.act_dev)):
            x, y = x.cpu().numpy(), y.cpu().numpy()
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (name, chunk, np.argwhere(x != y)[:5])
        for x, y in zip(ef.engine.get_state(), es.engine.get_state()):
            assert np.array_equal(x, y), chunk
        assert torch.equal(sf, ss), chunk
    assert sf.sum().item() > 0, "no episode ended inside the launches"
    assert ef.stats()["rollout_aborts"] == 0
    ef.close(); es.close()


def test_repeat_determinism():
    """The small rollout run twice on fresh engines gives identical arrays."""
    _assert_same(_case1(True), _case1(True, 1))
