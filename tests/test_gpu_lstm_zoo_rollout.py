"""A recurrent learner against policy-zoo nets (learn(network='lstm', opponent_mode='fix'); include/sumo_hip.h
sumo_rollout_steps_lstm_zoo / sumo_rollout_steps_lstm_zoo_lstm) on the GPU: the fused launches against the step-by-step launches
they replace (ppo_lstm_step for the learner and a zoo LSTM net, ppo_forward_filtered for a zoo MLP net, sumo_step, ppo_post_step)
bit for bit, both against the numpy restatement of the nets on the recorded observations, the table row per 16-env tile, learn()
end to end on either path, and the launches' loud failures.

Tolerances of the numpy comparison.  Zoo side, from tests/test_gpu_zoo_lstm_rollout.py unchanged: 5e-5 absolute on the zoo net's
action mean and on its final state, 1e-3 * (1 + max |neglogp|) on its likelihoods.  Learner side (LSTM(128), float32 sums of 121 +
128 products on the vector ALU against float32 numpy): LEARNER_* below, see their comment."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import has_gpu
from zoo_lstm_helpers import golden, synthetic_lstm_flat

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch
    from robosumo_selfplay_amd import capi, lstm_model, policy_zoo
    from robosumo_selfplay_amd.runner import Runner
    from robosumo_selfplay_amd.vec_env import SumoVecEnv
    from oracle import ppo_oracle as po

NAMES = ["obs", "returns", "masks", "actions", "values", "neglogpacs", "rewards", "opp_neglogpacs", "opp_obs", "opp_actions", "states",
         "epinfos", "off_policy_ratio", "off_env_ratio", "total_ratio"]
ANT = "RoboSumo-Ant-vs-Ant-v0"
KINDS = ("mlp", "lstm")

# Bounds of the learner's numbers against numpy: four times the error of the STEP-BY-STEP launches (SUMO_FUSED_ROLLOUT=0,
# ppo_lstm_step; the `stepwise` cases of test 2 print it), rounded up to the next of 1 / 2 / 5 x 10^k.  Measured on an MI355X at the
# shapes of test 2 against the golden v3 nets, the larger of the two zoo families each: action mean 2.70e-6, value 1.56e-6, final
# state rows 2.26e-6 absolute; neglogp 8.51e-6 at max |neglogp| = 21.7, i.e. 3.7e-7 * (1 + max).  The fused launch equals the
# step-by-step launches bit for bit (test 1) and is held to the same bounds.
LEARNER_MEAN_TOL, LEARNER_VALUE_TOL, LEARNER_STATE_TOL, LEARNER_NLP_TOL = 2e-5, 1e-5, 1e-5, 2e-6

def _dims(env):
    return env.observation_space[0].shape[0], env.action_space[0].shape[0]


def synthetic_mlp_flat(D, A, seed):
    """A zoo-MLP-shaped vector with a non-trivial observation filter and O(1) weights (as tests/test_gpu_zoo_fused.py builds it)."""
    rng = np.random.default_rng(seed)
    sh = policy_zoo.zoo_mlp_shapes(D, A)
    cnt = 1000.0
    parts = []
    for k in policy_zoo._ZOO_MLP_ORDER:
        s = sh[k]
        if k.endswith("/count"):
            v = np.array(cnt)
        elif k.endswith("/sum"):
            v = cnt * rng.normal(0, 0.5, s)
        elif k.endswith("/sumsq"):
            v = cnt * (0.25 + rng.uniform(0.0, 2.0, s))
        elif k == "logstd":
            v = rng.normal(-1.0, 0.3, s)
        elif k.endswith("/w"):
            v = rng.normal(0, 1.0 / np.sqrt(s[0]), s)
        else:
            v = rng.normal(0, 0.1, s)
        parts.append(np.asarray(v, np.float32).ravel())
    return np.concatenate(parts)


def _zoo_flat(kind, D, A, seed):
    return (synthetic_lstm_flat if kind == "lstm" else synthetic_mlp_flat)(D - 1, A, seed)


def _learner(N, T, D, A, seed=5, H=128):
    """An LSTM learner with livelier heads than the 0.01-scaled initialisation (as tests/test_gpu_lstm_rollout.py)."""
    spec = lstm_model.LstmSpec(D, A, H)
    np.random.seed(seed)
    m = lstm_model.LstmPPOModel(policy=spec, nbatch_act=N, nsteps=T, trainable=False)
    rng = np.random.default_rng(seed)
    pl = [p + rng.normal(0, 0.3 if p.ndim == 2 and p.shape[0] == H else 0.02, p.shape).astype(np.float32) for p in m.get_param_list()]
    m.set_param_list(pl)
    return m, pl


def _fix_runner(env, T, zoo_flat, opt_in=True, H=128):
    """What learn(network='lstm', opponent_mode='fix') builds: a Runner of two recurrent models whose second one is then replaced
    by the fixed zoo opponent."""
    N = env.num_envs
    D, A = _dims(env)
    learner, pl = _learner(N, T, D, A, H=H)
    other, _ = _learner(N, T, D, A, seed=6, H=H)
    r = Runner(env=env, models=[learner, other], nsteps=T, nagent=2, gamma=0.995, lam=0.95, rho_bar=1.0, c_bar=1.0, anneal_bound=500)
    zoo = policy_zoo.load_zoo_policy_from_flat(zoo_flat, A)
    learner.seed(101); zoo.seed(202)
    r.models[1] = policy_zoo.FixedOpponentModel(zoo)
    r.fused_fix_opponent = opt_in
    assert r.device_mode and r.recurrent
    return r, pl


def _near_time_limit(env):
    """Every episode starts near the time limit, so episodes end (auto-reset, and both state resets) inside the rollouts."""
    for E in env.engines:
        qpos, qvel, warm, cnt = E.get_state()
        cnt[:, 0] = env.model.timestep_limit - 40 + (np.arange(len(cnt)) % 37)
        E.set_state(qpos, qvel, warm, cnt)


def _bytes_equal(x, y):
    x, y = (z.cpu().numpy() if torch.is_tensor(z) else np.asarray(z) for z in (x, y))
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


# ---- 1. fused == step by step -------------------------------------------------------------------------------------------------
def _rollout_pair(kind, env_id, N, T, groups, fused, monkeypatch):
    monkeypatch.setenv("SUMO_FUSED_ROLLOUT", "1" if fused else "0")
    env = SumoVecEnv(env_id, num_envs=N, seed=11, groups=groups)
    if "Bug" in env_id:
        assert not env.engine.static_layout()                         # the runtime-layout kernel variant
    D, A = _dims(env)
    r, _ = _fix_runner(env, T, _zoo_flat(kind, D, A, 9))
    assert type(r.models[1].act_model) is (policy_zoo.ZooLSTMPolicy if kind == "lstm" else policy_zoo.ZooMLPPolicy)
    assert r.lstm_zoo_opponent() is not None and r.fused_lstm_zoo_ok() == fused
    assert not r.fused_ok() and not r.fused_lstm_ok() and not r.fused_zoo_ok() and r.zoo_opponent() is None
    _near_time_limit(env)
    outs = [r.run(250), r.run(251)]                                   # two consecutive rollouts: episodes and recurrent states carry over
    torch.cuda.synchronize()
    st = [E.get_state() for E in env.engines]
    s0, zs = r.states[0].clone(), r.zoo_state.clone()
    aborts = env.stats()["rollout_aborts"]
    env.close()
    return outs, st, s0, zs, aborts


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("env_id,N,T,groups", [(ANT, 96, 24, 1), (ANT, 64, 12, 2), ("RoboSumo-Bug-vs-Bug-v0", 32, 8, 1)])
def test_lstm_zoo_rollout_kernel_matches_stepwise_path(kind, env_id, N, T, groups, monkeypatch):
    """Runner.run of a recurrent learner in fix mode with the opt-in: the fused launch against the step-by-step launches fed the same
    noise rows -- every returned array, the episode records, the env states, agent 0's state rows and (LSTM net) agent 1's are
    bit-identical."""
    fo, fs, f0, fz, fa = _rollout_pair(kind, env_id, N, T, groups, True, monkeypatch)
    so, ss, s0, sz, sa = _rollout_pair(kind, env_id, N, T, groups, False, monkeypatch)
    assert fa == 0 and sa == 0
    for f, s_ in zip(fo, so):
        for k, (x, y) in enumerate(zip(f, s_)):
            if torch.is_tensor(x):
                assert _bytes_equal(x, y), NAMES[k]
            else:
                assert x == y, NAMES[k]
    for a, b in zip(fs, ss):
        for x, y in zip(a, b):
            assert _bytes_equal(x, y)
    assert _bytes_equal(f0, s0) and float(f0.abs().max()) > 0
    assert _bytes_equal(fz, sz)
    if kind == "lstm":
        assert float(fz.abs().max()) > 0
    # at least one episode of each agent ended inside the compared rollouts (else the state resets are never exercised)
    assert sum(len(o[11]) for o in fo) > 0
    assert any(bool(o[2][0].any()) for o in fo) and any(bool(o[2][1].any()) for o in fo)
    assert all(bool(torch.isfinite(o[4]).all()) for o in fo)


def test_lstm64_learner_takes_the_stepwise_path(monkeypatch):
    """An LSTM(64) learner is outside the fused launch: the predicate says so and the step-by-step branch plays the rollout."""
    monkeypatch.setenv("SUMO_FUSED_ROLLOUT", "1")
    env = SumoVecEnv(ANT, num_envs=16, seed=3)
    D, A = _dims(env)
    r, _ = _fix_runner(env, 4, _zoo_flat("lstm", D, A, 9), H=64)
    assert r.lstm_zoo_opponent() is None and not r.fused_lstm_zoo_ok()
    out = r.run(250)
    assert torch.isfinite(out[4]).all() and torch.isfinite(out[5]).all() and float(r.zoo_state.abs().max()) > 0
    env.close()


# ---- 2. against numpy ---------------------------------------------------------------------------------------------------------
def numpy_errors(kind, fused, monkeypatch):
    """One rollout (N = 32, T = 16, golden v3 nets) on the chosen path; errors of every recorded number against numpy."""
    monkeypatch.setenv("SUMO_FUSED_ROLLOUT", "1" if fused else "0")
    N, T, H = 32, 16, 128
    env = SumoVecEnv(ANT, num_envs=N, seed=5)
    D, A = _dims(env)
    flat = golden("ant-lstm-v3" if kind == "lstm" else "ant-mlp-v3")
    Dz, p = (policy_zoo.split_zoo_lstm if kind == "lstm" else policy_zoo.split_zoo_mlp)(flat, A)
    assert Dz == D - 1
    r, pl = _fix_runner(env, T, flat)
    assert r.fused_lstm_zoo_ok() == fused
    _near_time_limit(env)
    out = r.run(250)
    torch.cuda.synchronize()
    assert env.stats()["rollout_aborts"] == 0
    gen = torch.Generator(device="cuda")
    gen.manual_seed(202)                                              # the zoo net's generator: its one [T, N, A] draw of the rollout
    noise1 = torch.randn((T, N, A), generator=gen, device="cuda", dtype=torch.float32).cpu().numpy().astype(np.float64)
    gen.manual_seed(101)                                              # the learner's: T consecutive [N, A] draws
    noise0 = np.stack([torch.randn((N, A), generator=gen, device="cuda", dtype=torch.float32).cpu().numpy() for _ in range(T)]).astype(np.float64)
    h = lambda k, *tail: out[k].cpu().numpy().reshape(2, N, T, *tail)  # sf01 order: env-major rows
    obs, done = h(0, D), h(2)
    act, val, nlp, onlp = [h(k, *tail).astype(np.float64) for k, tail in ((3, (A,)), (4, ()), (5, ()), (7, ()))]
    assert done[0].any() and done[1].any(), "no episode ended inside the rollout"
    wx, wh, b, pw, pb, ls, vw, vb = pl
    ls_l, ls_z = ls.astype(np.float64).ravel(), p["logstd"].astype(np.float64).ravel()
    heads = lambda lat: (lat @ pw + pb, (lat @ vw + vb)[:, 0])
    S0 = np.zeros((N, 2 * H), np.float32)
    zstate, zzero = np.zeros((4, N, 64), np.float32), np.zeros((4, N, 64), np.float32)
    e = dict(l_mean=0.0, l_val=0.0, l_nlp=0.0, z_mean=0.0, z_on0=0.0, z_on1=0.0)
    for t in range(T):
        # learner: agent 0 from its carried state (masked by dones[:, 0]); agent 1 from zeros, one evaluation scores and values
        lat0, S0 = po.lstm_step_baselines(wx, wh, b, obs[0, :, t], S0, done[0, :, t] != 0)
        lat1, _ = po.lstm_step_baselines(wx, wh, b, obs[1, :, t], np.zeros_like(S0), None)
        (m0, v0), (m1, v1) = heads(lat0), heads(lat1)
        e["l_mean"] = max(e["l_mean"], np.abs(act[0, :, t] - np.exp(ls_l) * noise0[t] - m0).max())
        e["l_val"] = max(e["l_val"], np.abs(val[0, :, t] - v0).max(), np.abs(val[1, :, t] - v1).max())
        e["l_nlp"] = max(e["l_nlp"], np.abs(nlp[0, :, t] - po.neglogp(m0.astype(np.float64), ls_l, act[0, :, t])).max(),
                         np.abs(nlp[1, :, t] - po.neglogp(m1.astype(np.float64), ls_l, act[1, :, t])).max())
        if kind == "lstm":
            zstate[:, done[1, :, t] != 0, :] = 0                      # M = dones[:, 1] of the previous step
            z1, _, zstate = po.zoo_lstm_step(p, obs[1, :, t, :Dz], zstate)
            zstate = zstate.astype(np.float32)
            z0, _, _ = po.zoo_lstm_step(p, obs[0, :, t, :Dz], zzero)  # the scoring call starts from zeros
        else:
            z1, z0 = po.zoo_mlp_forward(p, obs[1, :, t, :Dz])[0], po.zoo_mlp_forward(p, obs[0, :, t, :Dz])[0]
        e["z_mean"] = max(e["z_mean"], np.abs(act[1, :, t] - np.exp(ls_z) * noise1[t] - z1).max())
        e["z_on1"] = max(e["z_on1"], np.abs(onlp[1, :, t] - po.neglogp(z1.astype(np.float64), ls_z, act[1, :, t])).max())
        e["z_on0"] = max(e["z_on0"], np.abs(onlp[0, :, t] - po.neglogp(z0.astype(np.float64), ls_z, act[0, :, t])).max())
    e["l_state"] = np.abs(r.states[0].cpu().numpy() - S0).max()
    zs = r.zoo_state.cpu().numpy()
    e["z_state"] = max(np.abs(zs[:, :64] - zstate[2]).max(), np.abs(zs[:, 64:] - zstate[3]).max()) if kind == "lstm" else float(np.abs(zs).max())
    e.update(nlp_max=np.abs(nlp).max(), on0_max=np.abs(onlp[0]).max(), on1_max=np.abs(onlp[1]).max(), val_max=np.abs(val).max())
    env.close()
    print("%s zoo net, %s: " % (kind, "fused" if fused else "step by step") + ", ".join("%s %.3g" % kv for kv in sorted(e.items())))
    return e


@pytest.mark.parametrize("fused", (False, True), ids=("stepwise", "fused"))
@pytest.mark.parametrize("kind", KINDS)
def test_lstm_zoo_rollout_matches_numpy_nets(kind, fused, monkeypatch):
    """Both paths against numpy (oracle.ppo_oracle), each printing its errors: the step-by-step launches, which the learner's bounds
    come from, and the fused launch, held to the same bounds."""
    e = numpy_errors(kind, fused, monkeypatch)
    print("learner bounds: mean %.3g, value %.3g, state %.3g, neglogp %.3g * (1 + max)" % (LEARNER_MEAN_TOL, LEARNER_VALUE_TOL, LEARNER_STATE_TOL,
                                                                                           LEARNER_NLP_TOL))
    assert e["z_mean"] < 5e-5 and e["z_state"] < 5e-5                 # (MLP net: zoo_state stays zero)
    assert e["z_on1"] < 1e-3 * (1 + e["on1_max"]) and e["z_on0"] < 1e-3 * (1 + e["on0_max"])
    assert e["l_mean"] < LEARNER_MEAN_TOL and e["l_val"] < LEARNER_VALUE_TOL and e["l_state"] < LEARNER_STATE_TOL
    assert e["l_nlp"] < LEARNER_NLP_TOL * (1 + e["nlp_max"])


# ---- 3. a table row per 16-env tile -------------------------------------------------------------------------------------------
RECORD = ("obs", "act", "rew", "val", "nlp", "onlp", "done", "ep_done", "ep_r", "ep_l")


def _direct_launch(kind, flats, tile_net, N=32, T=6):
    """One launch of the group method on a fresh env (same seed, zero states, same noise): the record, agent 0's and the zoo state."""
    env = SumoVecEnv(ANT, num_envs=N, seed=13)
    D, A = _dims(env)
    r, _ = _fix_runner(env, T, flats[0])
    m0 = r.models[0]
    table = (policy_zoo.ZooLstmTable if kind == "lstm" else policy_zoo.ZooTable)(flats, A, env.device)
    B = r._alloc_device(T)
    g = torch.Generator(device="cuda"); g.manual_seed(7)
    noise = [torch.randn((T, N, A), generator=g, device="cuda", dtype=torch.float32) for _ in range(2)]
    tn = None if tile_net is None else torch.tensor(tile_net, dtype=torch.int32, device="cuda")
    ro = capi.RolloutLstm(learner=C.addressof(m0._net), opponents_dev=None, tile_net_dev=None if tn is None else tn.data_ptr(),
                          npool=table.capacity, state0=r.states[0].data_ptr(), state1=None, T=T, Ntot=N, env_offset=0, s0=0, K=T, alpha=0.5,
                          noise0=noise[0].data_ptr(), noise1=noise[1].data_ptr())
    for f in RECORD:
        setattr(ro, f, B[f].data_ptr())
    if kind == "lstm":
        env.rollout_steps_lstm_zoo_lstm_group(0, ro, table.struct(r.zoo_state))
    else:
        env.rollout_steps_lstm_zoo_group(0, ro, table.struct())
    torch.cuda.synchronize()
    try:
        env.engine.rollout_status()
        status = None
    except capi.SumoHipError as ex:
        status = str(ex)
    rec = {f: B[f].cpu().numpy() for f in RECORD}
    rec["state0"], rec["zoo_state"] = r.states[0].cpu().numpy(), r.zoo_state.cpu().numpy()
    if status is not None:
        env.reset_device()
    env.close()
    return rec, status


@pytest.mark.parametrize("kind", KINDS)
def test_lstm_zoo_rollout_table_row_per_tile(kind):
    """tile_net selects the table row per 16-env tile: with [A, B] and tile_net [0, 1], tile 0's rows equal the run against [A] and
    tile 1's the run against [B] bit for bit (envs are independent); a row outside the table raises the abort flag."""
    D, A = 121, 8
    fa, fb = _zoo_flat(kind, D, A, 31), _zoo_flat(kind, D, A, 32)
    both, st = _direct_launch(kind, [fa, fb], [0, 1])
    assert st is None
    for flats, tile in (([fa], 0), ([fb], 1)):
        one, st = _direct_launch(kind, flats, None)
        assert st is None
        cols = slice(16 * tile, 16 * tile + 16)
        for f in RECORD:
            x, y = (z[..., cols] if f in ("ep_done", "ep_r", "ep_l") else z[:, :, cols] for z in (both[f], one[f]))
            assert _bytes_equal(x, y), (f, tile)
        for f in ("state0", "zoo_state"):
            assert _bytes_equal(both[f][cols], one[f][cols]), (f, tile)
    other, _ = _direct_launch(kind, [fb], None)
    assert not np.array_equal(both["act"][1][:, :16], other["act"][1][:, :16])     # (the two rows do play differently)
    _, st = _direct_launch(kind, [fa, fb], [0, 2])
    assert st is not None and "-20" in st and "cut short" in st


# ---- 4. learn end to end ------------------------------------------------------------------------------------------------------
def _learn(path, log, fused_fix):
    from robosumo_selfplay_amd import alg_ppo
    env = SumoVecEnv(ANT, num_envs=16, seed=1)
    model = alg_ppo.learn(network="lstm", nlstm=128, env=env, seed=1, total_timesteps=16 * 8 * 2, nagent=2, log_dir=log, verbose=False,
                          nsteps=8, nminibatches=4, noptepochs=2, lr=1e-3, gamma=0.995, lam=0.95, rho_bar=1.0, c_bar=1.0,
                          opponent_mode="fix", fix_opponent_path=path, anneal_bound=1000, fused_fix_opponent=fused_fix)
    assert len(model.history["lossvals"]) == 2 and all(np.isfinite(l).all() for l in model.history["lossvals"])
    assert sum(model.history["env_rollout_aborts"]) == 0
    params = model.params.clone()
    env.close()
    return params


@pytest.mark.parametrize("kind", KINDS)
def test_learn_lstm_against_zoo_file(kind, tmp_path, monkeypatch):
    """learn(network='lstm', opponent_mode='fix') with a zoo file of either family: the fused launch (counted) and the step-by-step
    launches under the opt-in train the same parameters bit for bit; the plain step-by-step path (no opt-in) trains too."""
    calls = {"n": 0}
    name = "rollout_steps_lstm_zoo_lstm_group" if kind == "lstm" else "rollout_steps_lstm_zoo_group"
    orig = getattr(SumoVecEnv, name)

    def counted(self, g, ro, zoo):
        calls["n"] += 1
        return orig(self, g, ro, zoo)
    monkeypatch.setattr(SumoVecEnv, name, counted)
    path = os.path.join(str(tmp_path), "agent-params-test.npy")
    np.save(path, _zoo_flat(kind, 121, 8, 7))
    params = []
    for fused in (True, False):
        monkeypatch.setenv("SUMO_FUSED_ROLLOUT", "1" if fused else "0")
        params.append(_learn(path, os.path.join(str(tmp_path), "log%d" % fused), True))
        assert calls["n"] == 2                                        # updates x env groups, on the fused run only
    assert torch.isfinite(params[0]).all() and torch.equal(params[0], params[1])
    monkeypatch.setenv("SUMO_FUSED_ROLLOUT", "1")
    plain = _learn(path, os.path.join(str(tmp_path), "plain"), False)  # per-step draws from each net's own generator
    assert torch.isfinite(plain).all() and calls["n"] == 2


# ---- 5. loud failures ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_lstm_zoo_rollout_launch_refusals(kind):
    N, T = 16, 4
    env = SumoVecEnv(ANT, num_envs=N, seed=2)
    D, A = _dims(env)
    r, _ = _fix_runner(env, T, _zoo_flat(kind, D, A, 9))
    m0 = r.models[0]
    small = lstm_model.LstmPPOModel(policy=lstm_model.LstmSpec(D, A, 64), nbatch_act=N, nsteps=T, trainable=False)
    zoo = (policy_zoo.ZooLstmTable if kind == "lstm" else policy_zoo.ZooTable)([_zoo_flat(kind, D, A, 20 + j) for j in range(2)], A, env.device)
    B = r._alloc_device(T)
    noise = [torch.randn((T, N, A), device="cuda") for _ in range(2)]
    st1 = torch.zeros((N, 128), dtype=torch.float32, device="cuda")
    tile = torch.ones(1, dtype=torch.int32, device="cuda")
    E, bufs = env.engine, env.env_ptrs(0)
    launch = E.rollout_steps_lstm_zoo_lstm if kind == "lstm" else E.rollout_steps_lstm_zoo

    def ro(**kw):
        o = capi.RolloutLstm(learner=C.addressof(m0._net), opponents_dev=None, tile_net_dev=tile.data_ptr(), npool=2,
                             state0=r.states[0].data_ptr(), state1=None, T=T, Ntot=N, env_offset=0, s0=0, K=T, alpha=0.5,
                             noise0=noise[0].data_ptr(), noise1=noise[1].data_ptr())
        for f in RECORD:
            setattr(o, f, B[f].data_ptr())
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def zs(**kw):
        z = zoo.struct(st1) if kind == "lstm" else zoo.struct()
        for k, v in kw.items():
            setattr(z, k, v)
        return z

    launch(ro(), zs(), *bufs)                                         # a good launch, row 1 of the table
    E.rollout_status()
    env.reset_device()
    # refused before any launch
    cases = [("opponents_dev", dict(opponents_dev=st1.data_ptr()), {}), ("state1", dict(state1=st1.data_ptr()), {}),
             ("missing", dict(state0=None), {}), ("missing", dict(learner=None), {}), ("hidden 128", dict(learner=C.addressof(small._net)), {}),
             ("nzoo", {}, dict(nzoo=1)), ("nzoo", dict(npool=0), dict(nzoo=0)), ("ob_dim", {}, dict(ob_dim=D + 1)), ("ob_dim", {}, dict(ob_dim=0)),
             ("params", {}, dict(params=None)), ("filt", {}, dict(filt=None)), ("obs_clip", {}, dict(obs_clip=0.0)),
             ("missing", dict(noise1=None), {}), ("missing", dict(onlp=None), {}), ("outside", dict(K=T + 1), {}),
             ("multiples of 16", dict(env_offset=8, Ntot=N + 8), {})]
    if kind == "lstm":
        cases += [("state", {}, dict(state=None)), ("hidden", {}, dict(hidden=128)), ("emb_dim", {}, dict(emb_dim=32))]
    for field, rkw, zkw in cases:
        with pytest.raises(capi.SumoHipError, match=field):
            launch(ro(**rkw), zs(**zkw), *bufs)
    E.set_cfrc_mode("rne_post")
    with pytest.raises(capi.SumoHipError, match="rne_post"):
        launch(ro(), zs(), *bufs)
    E.set_cfrc_mode("zero")
    env.reset_device()
    env.close()
    mixed = SumoVecEnv("RoboSumo-Ant-vs-Bug-v0", num_envs=4, seed=2)   # mixed match-ups stay refused
    with pytest.raises(capi.SumoHipError, match="homogeneous"):
        mixed_launch = mixed.engine.rollout_steps_lstm_zoo_lstm if kind == "lstm" else mixed.engine.rollout_steps_lstm_zoo
        mixed_launch(ro(Ntot=4), zs(), *mixed.env_ptrs(0))
    mixed.close()
