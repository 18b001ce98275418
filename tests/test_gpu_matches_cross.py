"""Cross-family matches on the GPU: MLP(64,64) checkpoints against LSTM(128) checkpoints in either seating (include/sumo_hip.h
sumo_match_steps_cross) and LSTM(128) checkpoints against policy-zoo MLP nets (sumo_match_steps_lstm_zoo), each against the
step-by-step path -- per step and side the launch of that side's family (ppo_forward, ppo_lstm_step, ppo_forward_filtered), then
env.step_device and the score update.  Everything is compared as bit patterns: observations, info rows, done flags, actions, the
recurrent state, qpos / qvel / warm start / counters and the score counters.  Both paths are tied to the models' own step; then the
per-table index checks, the quota, the C ABI's refusals and the drivers built on the launches."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from zoo_lstm_helpers import golden, synthetic_lstm_flat  # noqa: E402

pytestmark = pytest.mark.gpu

ANT, SPIDER = "RoboSumo-Ant-vs-Ant-v0", "RoboSumo-Spider-vs-Spider-v0"
N_MLP, N_LSTM = 3, 2                                              # the two tables differ in size: each index has its own bound


def _env(env_id, N, groups=1, seed=11):
    from robosumo_selfplay_amd.vec_env import SumoVecEnv
    return SumoVecEnv(env_id, num_envs=N, seed=seed, adjust_z=-0.5, groups=groups)


def _dims(env):
    return env.observation_space[0].shape[0], env.action_space[0].shape[0]


def _lstm_plist(D, A, rng, H=128, scale=0.1):
    from robosumo_selfplay_amd import policies
    pl = policies.init_lstm_param_list(D, A, H, rng=np.random.RandomState(int(rng.integers(1 << 30))))
    return [p + scale * rng.standard_normal(p.shape).astype(np.float32) for p in pl]


def _mlp_plist(D, A, rng, scale=0.3):
    from robosumo_selfplay_amd import policies
    return [p + scale * rng.standard_normal(p.shape).astype(np.float32) for p in policies.init_param_list(D, A)]


def _lstm_table(env, k=N_LSTM, seed=0, H=128):
    from robosumo_selfplay_amd import matches
    from robosumo_selfplay_amd.lstm_model import LstmSpec
    D, A = _dims(env)
    rng = np.random.default_rng(seed)
    t = matches.LstmSnapshotTable(LstmSpec(D, A, H), k, env.device)
    for j in range(k):
        t.set(j, _lstm_plist(D, A, rng, H))
    return t


def _mlp_table(env, k=N_MLP, seed=1):
    from robosumo_selfplay_amd import matches, policies
    D, A = _dims(env)
    rng = np.random.default_rng(seed)
    t = matches.SnapshotTable(policies.PolicySpec(D, A, value_network="copy", activation="relu"), k, env.device)
    for j in range(k):
        t.set(j, policies.flatten_params(_mlp_plist(D, A, rng)))
    return t


def _synthetic_zoo_flat(D, A, seed):
    """A zoo-shaped MLP vector with a non-trivial observation filter and O(1) weights (as tests/test_gpu_zoo_fused.py)."""
    from robosumo_selfplay_amd import policy_zoo
    rng = np.random.default_rng(seed)
    sh = policy_zoo.zoo_mlp_shapes(D, A)
    parts = []
    for k in policy_zoo._ZOO_MLP_ORDER:
        s = sh[k]
        if k.endswith("/count"):
            v = np.array(1000.0)
        elif k.endswith("/sum"):
            v = 1000.0 * rng.normal(0, 0.5, s)
        elif k.endswith("/sumsq"):
            v = 1000.0 * (0.25 + rng.uniform(0.0, 2.0, s))
        elif k == "logstd":
            v = rng.normal(-1.0, 0.3, s)
        elif k.endswith("/w"):
            v = rng.normal(0, 1.0 / np.sqrt(s[0]), s)
        else:
            v = rng.normal(0, 0.1, s)
        parts.append(np.asarray(v, np.float32).ravel())
    return np.concatenate(parts)


def _golden_v3():
    return golden("ant-mlp-v3")


def _zoo_table(env):
    """The golden ant-mlp-v3 net plus a synthetic one (Ant); two synthetic ones for the other scenes."""
    from robosumo_selfplay_amd import policy_zoo
    D, A = _dims(env)
    first = _golden_v3() if D == 121 else _synthetic_zoo_flat(D - 1, A, 20)
    return policy_zoo.ZooTable([first, _synthetic_zoo_flat(D - 1, A, 21)], A, env.device)


def _snapshot(env, state):
    import torch
    torch.cuda.synchronize()
    host = [x.cpu().numpy().copy() for x in (env.obs_dev, env.info_dev, env.done_dev, env.act_dev, state)]
    for E in env.engines:
        host += list(E.get_state())
    return host


NAMES = ("obs", "info", "done", "actions", "state") + ("qpos", "qvel", "warm", "counters") * 2


def _near_time_limit(envs):
    """Every episode starts at timestep_limit - 40 + e % 37: it ends (and the env auto-resets, masking the state) inside the launches."""
    for g in range(envs[0].groups):
        qpos, qvel, warm, cnt = envs[0].engines[g].get_state()
        first = g * envs[0].group_size
        cnt[:, 0] = envs[0].model.timestep_limit - 40 + ((first + np.arange(len(cnt))) % 37)
        for e in envs:
            e.engines[g].set_state(qpos, qvel, warm, cnt)


def _indices(N, n0, n1, layout, rng):
    if layout == "random":
        return rng.integers(0, n0, N).astype(np.int32), rng.integers(0, n1, N).astype(np.int32)
    blk = np.arange(N) // 256                                     # contiguous blocks (play_cross_matches' layout), waves migrate
    return (blk % n0).astype(np.int32), ((blk // n0) % n1).astype(np.int32)


def _compare_paths(ef, es, fused, stepwise, n0, n1, A, deterministic, layout, chunks, K):
    """``chunks`` launches of K steps on both paths from episodes near the time limit; fused(env, idx0, idx1, state, score, noise)
    and stepwise(...) play them.  Returns the fused path's score counters and state."""
    import torch
    N = ef.num_envs
    idx0, idx1 = _indices(N, n0, n1, layout, np.random.default_rng(5))
    assert idx0.max() == n0 - 1 and idx1.max() == n1 - 1         # the last row of each table plays
    for e in (ef, es):
        e.reset_device()
    _near_time_limit([ef, es])
    i0, i1 = torch.from_numpy(idx0).cuda(), torch.from_numpy(idx1).cuda()
    stf = torch.zeros((N, 256), dtype=torch.float32, device="cuda")
    sts = torch.zeros_like(stf)
    cf = torch.zeros((N, 3), dtype=torch.int32, device="cuda")
    cs = torch.zeros_like(cf)
    quota = 2
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    for chunk in range(chunks):
        noise = None if deterministic else tuple(torch.randn((K, N, A), generator=gen, device="cuda") for _ in range(2))
        fused(ef, i0, i1, stf, cf, quota, K, noise)
        stepwise(es, idx0, idx1, sts, cs, quota, K, noise)
        a, b = _snapshot(ef, stf), _snapshot(es, sts)
        assert len(a) == len(b) == 5 + 4 * ef.groups
        for name, x, y in zip(NAMES, a, b):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (name, chunk, np.argwhere(x != y)[:5])
        assert torch.equal(cf, cs), chunk
    sc = cf.cpu().numpy()
    assert sc.sum(1).max() <= quota
    assert ef.stats()["rollout_aborts"] == 0
    return sc, stf


# (env, N, env groups, index layout, launches, K)
SHAPES = [(ANT, 96, 1, "random", 3, 24), (SPIDER, 32, 1, "random", 3, 24), (ANT, 32, 2, "random", 3, 24)]
BIG = (ANT, 4096, 1, "blocks", 1, 8)                              # more envs than persistent waves: one short launch per seating
CROSS_CASES = [s + (g, d) for s in SHAPES for g in (0, 1) for d in (True, False)] + [BIG + (0, False), BIG + (1, True)]
LSTM_ZOO_CASES = [s + (d,) for s in SHAPES for d in (True, False)] + [BIG + (False,)]


# ---- 1. fused == step by step ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id,N,groups,layout,chunks,K,lstm_side,deterministic", CROSS_CASES)
def test_cross_launch_equals_stepwise_path(env_id, N, groups, layout, chunks, K, lstm_side, deterministic):
    from robosumo_selfplay_amd import matches
    ef, es = _env(env_id, N, groups), _env(env_id, N, groups)
    mt, lt = _mlp_table(ef), _lstm_table(ef)
    n0, n1 = (N_LSTM, N_MLP) if lstm_side == 0 else (N_MLP, N_LSTM)

    def fused(env, i0, i1, st, sc, quota, k, noise):
        matches.cross_match_steps_fused(env, mt, lt, lstm_side, i0, i1, st, sc, quota, k, noise)

    def stepwise(env, i0, i1, st, sc, quota, k, noise):
        matches.cross_match_steps_stepwise(env, mt, lt, lstm_side, i0, i1, st, sc, quota, k, noise)
    sc, st = _compare_paths(ef, es, fused, stepwise, n0, n1, mt.spec.ac_dim, deterministic, layout, chunks, K)
    if chunks > 1:
        assert sc.sum() > 0, "no episode ended inside the launches"
    assert float(st.abs().sum()) > 0
    ef.close(); es.close()


@pytest.mark.parametrize("env_id,N,groups,layout,chunks,K,deterministic", LSTM_ZOO_CASES)
def test_lstm_zoo_launch_equals_stepwise_path(env_id, N, groups, layout, chunks, K, deterministic):
    from robosumo_selfplay_amd import matches
    ef, es = _env(env_id, N, groups), _env(env_id, N, groups)
    lt, zoo = _lstm_table(ef), _zoo_table(ef)

    def fused(env, i0, i1, st, sc, quota, k, noise):
        matches.lstm_zoo_match_steps_fused(env, lt, zoo, i0, i1, st, sc, quota, k, noise)

    def stepwise(env, i0, i1, st, sc, quota, k, noise):
        matches.lstm_zoo_match_steps_stepwise(env, lt, zoo, i0, i1, st, sc, quota, k, noise)
    sc, st = _compare_paths(ef, es, fused, stepwise, N_LSTM, 2, lt.spec.ac_dim, deterministic, layout, chunks, K)
    if chunks > 1:
        assert sc.sum() > 0, "no episode ended inside the launches"
    assert float(st.abs().sum()) > 0
    ef.close(); es.close()


# ---- 2. the first step against the models ---------------------------------------------------------------------------------------
def _first_step_setup(N, rng):
    import torch
    es, ef = _env(ANT, N), _env(ANT, N)
    for e in (es, ef):
        e.reset_device()
    done = torch.from_numpy(rng.integers(0, 2, (N, 2)).astype(np.uint8)).cuda()
    for e in (es, ef):
        e.done_dev.copy_(done)
    S = torch.from_numpy(rng.standard_normal((N, 256)).astype(np.float32)).cuda()
    return es, ef, done, S


@pytest.mark.parametrize("deterministic", [True, False])
@pytest.mark.parametrize("lstm_side", [0, 1])
def test_cross_first_step_equals_the_models(lstm_side, deterministic):
    """One step of both paths from random states and done flags: the MLP side's action equals PPOModel.step, the LSTM side's action
    and new state LstmPPOModel.step(obs, S, M) with that agent's done flags."""
    import torch
    from robosumo_selfplay_amd import matches, policies
    from robosumo_selfplay_amd.lstm_model import LstmPPOModel, LstmSpec
    from robosumo_selfplay_amd.model import PPOModel
    N = 48
    rng = np.random.default_rng(9)
    es, ef, done, S = _first_step_setup(N, rng)
    D, A = _dims(es)
    lspec, mspec = LstmSpec(D, A, 128), policies.PolicySpec(D, A, value_network="copy", activation="relu")
    lm = LstmPPOModel(policy=lspec, trainable=False)
    lm.set_param_list(_lstm_plist(D, A, rng))
    mm = PPOModel(policy=mspec, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, trainable=False)
    mm.set_param_list(_mlp_plist(D, A, rng))
    lt = matches.LstmSnapshotTable(lspec, 2, es.device)
    lt.set(1, lm); lt.set(0, _lstm_plist(D, A, rng))
    mt = matches.SnapshotTable(mspec, 3, es.device)
    mt.set(2, mm); mt.set(0, policies.flatten_params(_mlp_plist(D, A, rng))); mt.set(1, policies.flatten_params(_mlp_plist(D, A, rng)))
    gl, gm = lstm_side, 1 - lstm_side
    idx = [None, None]
    idx[gl], idx[gm] = np.full(N, 1, np.int32), np.full(N, 2, np.int32)
    noise = None
    if not deterministic:
        gen = torch.Generator(device="cuda")
        gen.manual_seed(77)
        noise = [None, None]
        noise[gm] = torch.randn((N, A), generator=gen, device="cuda", dtype=torch.float32)[None].contiguous()   # PPOModel.step's draw
        noise[gl] = torch.randn((1, N, A), device="cuda")
        mm.act_model.seed(77)
    obs = es.obs_dev[:, :, :D].clone()
    ss, sf = S.clone(), S.clone()
    sc = torch.zeros((N, 3), dtype=torch.int32, device="cuda")
    matches.cross_match_steps_stepwise(es, mt, lt, lstm_side, idx[0], idx[1], ss, sc, 1, 1, noise)
    matches.cross_match_steps_fused(ef, mt, lt, lstm_side, torch.from_numpy(idx[0]).cuda(), torch.from_numpy(idx[1]).cuda(), sf, sc.clone(),
                                    1, 1, noise)
    torch.cuda.synchronize()
    act_l, _, st, _ = lm.step(obs[:, gl], S=S, M=done[:, gl], deterministic=deterministic, noise=None if noise is None else noise[gl][0])
    act_m = mm.step(obs[:, gm].contiguous(), deterministic=deterministic)[0]
    for name, x in (("stepwise", es), ("fused", ef)):
        assert torch.equal(x.act_dev[:, gl, :A], act_l), (name, "lstm side")
        assert torch.equal(x.act_dev[:, gm, :A], act_m), (name, "mlp side")
    assert torch.equal(ss, st) and torch.equal(sf, st)
    assert not torch.equal(st, S)
    es.close(); ef.close()


@pytest.mark.parametrize("deterministic", [True, False])
def test_lstm_zoo_first_step_equals_the_models(deterministic):
    """The same for sumo_match_steps_lstm_zoo: agent 0 against LstmPPOModel.step, agent 1 against ZooMLPPolicy's kernel
    (ppo_forward_filtered) on the golden ant-mlp-v3 net."""
    import torch
    from robosumo_selfplay_amd import matches, policy_zoo, ppo_capi
    from robosumo_selfplay_amd.lstm_model import LstmPPOModel, LstmSpec
    N = 48
    rng = np.random.default_rng(10)
    es, ef, done, S = _first_step_setup(N, rng)
    D, A = _dims(es)
    lspec = LstmSpec(D, A, 128)
    lm = LstmPPOModel(policy=lspec, trainable=False)
    lm.set_param_list(_lstm_plist(D, A, rng))
    lt = matches.LstmSnapshotTable(lspec, 2, es.device)
    lt.set(1, lm); lt.set(0, _lstm_plist(D, A, rng))
    flat = _golden_v3()
    zoo = policy_zoo.ZooTable([_synthetic_zoo_flat(D - 1, A, 21), flat], A, es.device)
    zp = policy_zoo.ZooMLPPolicy(flat, A)
    idx = np.full(N, 1, np.int32)
    noise = None if deterministic else tuple(torch.randn((1, N, A), device="cuda") for _ in range(2))
    obs = es.obs_dev[:, :, :D].clone()
    ss, sf = S.clone(), S.clone()
    sc = torch.zeros((N, 3), dtype=torch.int32, device="cuda")
    i = torch.from_numpy(idx).cuda()
    matches.lstm_zoo_match_steps_stepwise(es, lt, zoo, idx, idx, ss, sc, 1, 1, noise)
    matches.lstm_zoo_match_steps_fused(ef, lt, zoo, i, i, sf, sc.clone(), 1, 1, noise)
    torch.cuda.synchronize()
    act0, _, st, _ = lm.step(obs[:, 0], S=S, M=done[:, 0], deterministic=deterministic, noise=None if noise is None else noise[0][0])
    act1 = zp.evaluate(obs[:, 1].contiguous(), ppo_capi.FWD_PI, deterministic=deterministic,
                       noise=None if noise is None else noise[1][0].contiguous())["action"]
    for name, x in (("stepwise", es), ("fused", ef)):
        assert torch.equal(x.act_dev[:, 0, :A], act0), (name, "agent 0")
        assert torch.equal(x.act_dev[:, 1, :A], act1), (name, "agent 1")
    assert torch.equal(ss, st) and torch.equal(sf, st)
    es.close(); ef.close()


# ---- 3. / 4. index checks per table, quota ----------------------------------------------------------------------------------------
def test_index_checks_per_table_and_quota():
    import torch
    from robosumo_selfplay_amd import capi, matches
    N = 40
    env = _env(ANT, N)
    mt, lt, zoo = _mlp_table(env), _lstm_table(env), _zoo_table(env)
    env.reset_device()
    sc = torch.zeros((N, 3), dtype=torch.int32, device="cuda")
    st = torch.zeros((N, 256), dtype=torch.float32, device="cuda")
    zero = torch.zeros(N, dtype=torch.int32, device="cuda")
    two = zero.clone(); two[3] = 2                               # row 2: the MLP table has it, the LSTM table does not
    for lstm_side in (0, 1):
        on_mlp, on_lstm = ((zero, two), (two, zero)) if lstm_side == 0 else ((two, zero), (zero, two))
        matches.cross_match_steps_fused(env, mt, lt, lstm_side, *on_mlp, st, sc, 1, 4)
        with pytest.raises(capi.SumoHipError, match="cut short"):
            matches.cross_match_steps_fused(env, mt, lt, lstm_side, *on_lstm, st, sc, 1, 4)
        env.reset_device()
    three = zero.clone(); three[5] = 3
    with pytest.raises(capi.SumoHipError, match="cut short"):
        matches.cross_match_steps_fused(env, mt, lt, 1, three, zero, st, sc, 1, 4)      # past the MLP table as well
    env.reset_device()
    one = zero.clone(); one[7] = 1
    matches.lstm_zoo_match_steps_fused(env, lt, zoo, one, one, st, sc, 1, 4)            # the last row of either table
    with pytest.raises(capi.SumoHipError, match="cut short"):
        matches.lstm_zoo_match_steps_fused(env, lt, zoo, zero, two, st, sc, 1, 4)       # idx1 against nzoo
    env.reset_device()
    with pytest.raises(capi.SumoHipError, match="cut short"):
        matches.lstm_zoo_match_steps_fused(env, lt, zoo, two, zero, st, sc, 1, 4)       # idx0 against nsnap
    # the step-by-step paths check the same bounds on the host
    h0, h2 = np.zeros(N, np.int32), two.cpu().numpy()
    with pytest.raises(ValueError, match="snapshot index"):
        matches.cross_match_steps_stepwise(env, mt, lt, 0, h2, h0, st, sc, 1, 1)
    with pytest.raises(ValueError, match="snapshot index"):
        matches.lstm_zoo_match_steps_stepwise(env, lt, zoo, h0, h2, st, sc, 1, 1)
    # counters stop at the quota even though the envs keep playing
    for launch in (lambda: matches.cross_match_steps_fused(env, mt, lt, 0, zero, zero, st, sc, 1, 256),
                   lambda: matches.cross_match_steps_fused(env, mt, lt, 1, zero, zero, st, sc, 1, 256),
                   lambda: matches.lstm_zoo_match_steps_fused(env, lt, zoo, zero, zero, st, sc, 1, 256)):
        env.reset_device()
        sc.zero_(); st.zero_()
        for _ in range(3):
            launch()
        assert sc.sum(1).max().item() == 1 and sc.sum(1).min().item() == 1
    env.close()


# ---- 5. refusals through the C ABI ------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi():
    import torch
    from robosumo_selfplay_amd import capi, policy_zoo, ppo_capi
    N = 16
    env = _env(ANT, N)
    D, A = _dims(env)
    mt, lt, zoo = _mlp_table(env), _lstm_table(env), _zoo_table(env)
    i = torch.zeros(N, dtype=torch.int32, device="cuda")
    sc = torch.zeros((N, 3), dtype=torch.int32, device="cuda")
    st = torch.zeros((N, 256), dtype=torch.float32, device="cuda")
    env.reset_device()
    E = env.engine
    bufs = env.env_ptrs(0)
    keep = []

    def proto(**kw):
        p = ppo_capi.LstmNet.from_buffer_copy(lt.proto)
        for k, v in kw.items():
            setattr(p, k, v)
        keep.append(p)
        return C.addressof(p)

    def mc(**kw):
        m = capi.MatchCross(params=mt.params.data_ptr(), nsnap_mlp=N_MLP, ob_dim=D, ac_dim=A, proto=proto(), nets_dev=lt.nets_dev.data_ptr(),
                            nsnap_lstm=N_LSTM, state=st.data_ptr(), lstm_side=1, idx0=i.data_ptr(), idx1=i.data_ptr(), T=4, s0=0, K=4,
                            quota=1, score=sc.data_ptr())
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    def ml(**kw):
        m = capi.MatchLstm(proto=proto(), nets_dev=lt.nets_dev.data_ptr(), idx0=i.data_ptr(), idx1=i.data_ptr(), nsnap=N_LSTM,
                           state0=st.data_ptr(), T=4, s0=0, K=4, quota=1, score=sc.data_ptr())
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    def zs(**kw):
        z = zoo.struct()
        for k, v in kw.items():
            setattr(z, k, v)
        return z
    for bad, what in ((dict(lstm_side=2), "lstm_side"), (dict(lstm_side=-1), "lstm_side"), (dict(state=None), "state"),
                      (dict(nsnap_lstm=0), "nsnap"), (dict(nsnap_mlp=0), "nsnap"), (dict(proto=proto(hidden=64)), "hidden 128"),
                      (dict(noise0=st.data_ptr()), "noise"), (dict(noise1=st.data_ptr()), "noise"), (dict(params=None), "missing buffer"),
                      (dict(nets_dev=None), "missing buffer"), (dict(score=None), "missing buffer"), (dict(ob_dim=D + 1), "do not match"),
                      (dict(proto=proto(ob_dim=D + 1)), "do not match"), (dict(K=5), "outside the rollout buffers")):
        with pytest.raises(capi.SumoHipError, match=what):
            E.match_steps_cross(mc(**bad), *bufs)
    with pytest.raises(capi.SumoHipError, match="state1 must be NULL"):
        E.match_steps_lstm_zoo(ml(state1=st.data_ptr()), zs(), *bufs)
    with pytest.raises(capi.SumoHipError, match="state"):
        E.match_steps_lstm_zoo(ml(state0=None), zs(), *bufs)
    with pytest.raises(capi.SumoHipError, match="noise"):
        E.match_steps_lstm_zoo(ml(noise1=st.data_ptr()), zs(), *bufs)
    # the zoo table, as sumo_match_steps_zoo refuses it: wider than the scene's observation, empty, no filter, no clip
    for bad, what in ((dict(ob_dim=D + 1), "ob_dim"), (dict(ob_dim=0), "ob_dim"), (dict(nzoo=0), "nzoo"), (dict(filt=None), "missing"),
                      (dict(obs_clip=0.0), "obs_clip")):
        with pytest.raises(capi.SumoHipError, match=what):
            E.match_steps_lstm_zoo(ml(), zs(**bad), *bufs)
    E.set_cfrc_mode("rne_post")
    with pytest.raises(capi.SumoHipError, match="rne_post"):
        E.match_steps_cross(mc(), *bufs)
    with pytest.raises(capi.SumoHipError, match="rne_post"):
        E.match_steps_lstm_zoo(ml(), zs(), *bufs)
    E.set_cfrc_mode("zero")
    # a heterogeneous scene
    het = _env("RoboSumo-Ant-vs-Bug-v0", N)
    het.reset_device()
    with pytest.raises(capi.SumoHipError, match="homogeneous"):
        het.engine.match_steps_cross(mc(), *het.env_ptrs(0))
    with pytest.raises(capi.SumoHipError, match="homogeneous"):
        het.engine.match_steps_lstm_zoo(ml(), zs(), *het.env_ptrs(0))
    het.close()
    # after all of them, valid launches succeed
    for side in (0, 1):
        E.match_steps_cross(mc(lstm_side=side), *bufs)
        E.rollout_status()
    E.match_steps_lstm_zoo(ml(), zs(), *bufs)
    E.rollout_status()
    env.close()


# ---- 6. drivers ---------------------------------------------------------------------------------------------------------------------
def test_play_cross_matches_fused_equals_stepwise():
    from robosumo_selfplay_amd import matches
    env = _env(ANT, 40)
    mt, lt = _mlp_table(env), _lstm_table(env)
    for t0, t1, pairs in ((mt, lt, [(2, 1), (0, 0), (1, 1)]), (lt, mt, [(1, 2), (0, 0), (1, 1)])):
        kw = dict(rounds_per_env=2, envs_per_pair=12, deterministic=False, seed=7, chunk=128)
        res = matches.play_cross_matches(env, t0, t1, pairs, **kw)
        assert len(res) == 3
        for r in res:
            assert r["rounds"] == 24 == r["wins"] + r["losses"] + r["draws"]
            assert r["env_steps"] > 0 and r["env_steps"] % (128 * 12) == 0
        assert res == matches.play_cross_matches(env, t0, t1, pairs, fused=False, **kw)
    assert env.adjust_z == -0.5
    # LSTM(64) plays step by step only
    l64 = _lstm_table(env, H=64)
    with pytest.raises(ValueError, match=r"LSTM\(128\)"):
        matches.play_cross_matches(env, mt, l64, [(0, 1)], 1, 8, chunk=64)
    r64 = matches.play_cross_matches(env, l64, mt, [(1, 0)], 1, 8, chunk=256, fused=False)
    assert r64[0]["rounds"] == 8
    env.close()


def _save_runs(tmp_path, rng, n_mlp=3, n_lstm=2, H=128, suffix=""):
    """An MLP run and an LSTM run as PPOModel.save / LstmPPOModel.save write them (version 00000 is skipped by the drivers)."""
    import joblib
    runs = []
    for name, n, make in (("mlp" + suffix, n_mlp, lambda: _mlp_plist(121, 8, rng)), ("lstm" + suffix, n_lstm, lambda: _lstm_plist(121, 8, rng, H))):
        for v in range(n + 1):
            path = str(tmp_path / name / "checkpoints" / ("%.5i" % v))
            os.makedirs(os.path.dirname(path), exist_ok=True)
            joblib.dump(make(), path)
        runs.append(str(tmp_path / name))
    return runs


def test_compare_versions_cli_cross_family(tmp_path):
    import compare_versions
    from robosumo_selfplay_amd import matches
    mlp, lstm = _save_runs(tmp_path, np.random.default_rng(2))
    for p1, p2, nets in ((mlp, lstm, ["mlp", "lstm"]), (lstm, mlp, ["lstm", "mlp"])):
        with pytest.warns(UserWarning):                           # 3 versions against 2
            rec = compare_versions.main(["--p1", p1, "--p2", p2, "--trials", "8", "--num_env", "16", "--seed", "3", "--cross_family"])
        assert (rec["network"], rec["nlstm"], rec["cross_family"]) == ("cross", 128, True)
        assert [n["network"] for n in rec["networks"]] == nets
        assert rec["versions"] == [["00001", "00001"], ["00002", "00002"]]
        saved = json.load(open(os.path.join(p1, "compare_versions_vs_%s.json" % os.path.basename(p2))))
        assert saved["network"] == "cross" and saved["networks"] == rec["networks"] and saved["win_rate"] == rec["win_rate"]
        assert saved["networks"][nets.index("lstm")] == {"network": "lstm", "nlstm": 128}
        for r in rec["results"]:
            assert r["rounds"] == 8
        with pytest.warns(UserWarning):
            ref = matches.compare_history_versions(p1, p2, 8, num_env=16, seed=3, cross_family=True, fused=False)
        assert ref["network"] == "cross" and ref["win_rate"] == rec["win_rate"] and ref["results"] == rec["results"]
    # LSTM(64) against an MLP run: step by step only
    mlp64, lstm64 = _save_runs(tmp_path, np.random.default_rng(4), n_mlp=1, n_lstm=1, H=64, suffix="64")
    with pytest.raises(ValueError, match=r"LSTM\(128\)"):
        matches.compare_history_versions(mlp64, lstm64, 4, num_env=8, cross_family=True)
    r64 = matches.compare_history_versions(mlp64, lstm64, 4, num_env=8, cross_family=True, fused=False)
    assert r64["nlstm"] == 64 and r64["results"][0]["rounds"] == 4


def test_evaluate_lstm_run_against_mixed_zoo_files(tmp_path):
    from robosumo_selfplay_amd import matches
    _, lstm = _save_runs(tmp_path, np.random.default_rng(6))
    files = [str(tmp_path / "agent-params-v3.npy"), str(tmp_path / "lstm-params.npy")]
    np.save(files[0], _golden_v3())
    np.save(files[1], synthetic_lstm_flat(120, 8, 8))
    kw = dict(start=1, num_env=16, seed=5, chunk=128)
    with pytest.raises(ValueError, match="zoo MLP nets"):
        matches.evaluate_history_against_zoo(lstm, files, 8, **kw)
    res = matches.evaluate_history_against_zoo(lstm, files, 8, cross_family=True, **kw)
    assert res["checkpoints"] == [1, 2] and list(res["results"]) == [(1, 0), (1, 1), (2, 0), (2, 1)]
    for r in res["results"].values():
        assert r["rounds"] == 8 and abs(r["win"] + r["draw"] + r["lose"] - 1.0) < 1e-12
    assert (res["network"], res["nlstm"], res["opponent_networks"]) == ("lstm", 128, ["mlp", "lstm"])
    ref = matches.evaluate_history_against_zoo(lstm, files, 8, cross_family=True, fused=False, **kw)
    assert ref["results"] == res["results"]
    # the CLI passes the flag through and records it with the families that met
    import eval_against_fix
    argv = ["--path", lstm, "--opponent_path", files[0], "--opponent_path", files[1], "--fused", "--trials", "8", "--num_env", "16",
            "--start", "1", "--seed", "5"]
    with pytest.raises(ValueError, match="zoo MLP nets"):
        eval_against_fix.main(argv)
    tab = eval_against_fix.main(argv + ["--cross_family"])
    assert tab.shape == (2, 7) and np.allclose(tab, np.array(json.load(open(os.path.join(lstm, "eval_against_fix.json")))))
    meta = json.load(open(os.path.join(lstm, "eval_against_fix_networks.json")))
    assert meta["cross_family"] is True and meta["networks"] == [{"network": "lstm", "nlstm": 128}, ["mlp", "lstm"]]
