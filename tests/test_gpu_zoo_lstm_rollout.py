"""The fused rollout launch against a policy-zoo LSTM net (include/sumo_hip.h sumo_rollout_steps_zoo_lstm, learn(opponent_mode='fix')
with an LSTM file) on the GPU: against the step-by-step launches it replaces (ppo_forward for the learner, ppo_lstm_step on the zoo
net's policy branch, sumo_step, ppo_post_step) bit for bit, against the numpy restatement of both nets on the recorded
observations, learn() end to end on either path, and the launch's loud failures.

Tolerances of the numpy comparison, from the project's tests of the same nets: 5e-5 absolute on the zoo net's action mean and on
its final state (tests/test_gpu_zoo_lstm_fused.py), 1e-3 * (1 + max |neglogp|) on likelihoods and 2e-5 * (1 + max |v|) on the
learner's values (tests/test_gpu_zoo_fused.py)."""
import os

import numpy as np
import pytest

from conftest import has_gpu
from zoo_lstm_helpers import golden, synthetic_lstm_flat

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch
    from robosumo_selfplay_amd import capi, policies, policy_zoo
    from robosumo_selfplay_amd.model import PPOModel
    from robosumo_selfplay_amd.runner import Runner
    from robosumo_selfplay_amd.vec_env import SumoVecEnv
    from oracle import ppo_oracle as po

NAMES = ["obs", "returns", "masks", "actions", "values", "neglogpacs", "rewards", "opp_neglogpacs", "opp_obs", "opp_actions", "states",
         "epinfos", "off_policy_ratio", "off_env_ratio", "total_ratio"]


def _dims(env):
    return env.observation_space[0].shape[0], env.action_space[0].shape[0]


def _learner(D, A, seed):
    np.random.seed(seed)
    spec = policies.PolicySpec(D, A, value_network="copy", activation="relu")
    m = PPOModel(policy=spec, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, trainable=False)
    rng = np.random.RandomState(seed)
    pl = [p + rng.normal(0, 0.1, p.shape).astype(np.float32) for p in m.get_param_list()]
    m.set_param_list(pl)
    return m, pl


def _fix_runner(env, T, zoo_flat, seed=3, opt_in=True):
    D, A = _dims(env)
    learner, pl = _learner(D, A, seed)
    zoo = policy_zoo.ZooLSTMPolicy(zoo_flat, A)
    learner.act_model.seed(101); zoo.seed(202)
    r = Runner(env=env, models=[learner, policy_zoo.FixedOpponentModel(zoo)], nsteps=T, nagent=2, gamma=0.995, lam=0.95, rho_bar=1.0,
               c_bar=1.0, anneal_bound=500)
    r.fused_fix_opponent = opt_in
    return r, pl


def _near_time_limit(env):
    """Every episode starts near the time limit, so episodes end (auto-reset, and agent 1's state rows reset) inside the rollouts."""
    for E in env.engines:
        qpos, qvel, warm, cnt = E.get_state()
        cnt[:, 0] = env.model.timestep_limit - 40 + (np.arange(len(cnt)) % 37)
        E.set_state(qpos, qvel, warm, cnt)


# ---- 1. fused == step by step -------------------------------------------------------------------------------------------------
def _rollout_pair(env_id, N, T, groups, fused, monkeypatch):
    monkeypatch.setenv("SUMO_FUSED_ROLLOUT", "1" if fused else "0")
    env = SumoVecEnv(env_id, num_envs=N, seed=11, groups=groups)
    if "Bug" in env_id:
        assert not env.engine.static_layout()                         # the runtime-layout kernel variant
    D, A = _dims(env)
    r, _ = _fix_runner(env, T, synthetic_lstm_flat(D - 1, A, 9))
    assert isinstance(r.models[1].act_model, policy_zoo.ZooLSTMPolicy)
    assert r.zoo_opponent() is not None and r.fused_zoo_ok() == fused and not r.fused_ok() and not r.fused_lstm_ok()
    _near_time_limit(env)
    outs = [r.run(250), r.run(251)]                                   # two consecutive rollouts: episode and recurrent state carry over
    torch.cuda.synchronize()
    st = [E.get_state() for E in env.engines]
    zs = r.zoo_state.clone()
    aborts = env.stats()["rollout_aborts"]
    env.close()
    return outs, st, zs, aborts


@pytest.mark.parametrize("env_id,N,T,groups", [("RoboSumo-Ant-vs-Ant-v0", 96, 24, 1), ("RoboSumo-Ant-vs-Ant-v0", 64, 12, 2),
                                               ("RoboSumo-Bug-vs-Bug-v0", 32, 8, 1)])
def test_zoo_lstm_rollout_kernel_matches_stepwise_path(env_id, N, T, groups, monkeypatch):
    """Runner.run in fix mode with the opt-in: sumo_rollout_steps_zoo_lstm against the step-by-step launches fed the same noise
    rows -- every returned array, the episode records, the env states and agent 1's final state rows are bit-identical."""
    fo, fs, fz, fa = _rollout_pair(env_id, N, T, groups, True, monkeypatch)
    so, ss, sz, _ = _rollout_pair(env_id, N, T, groups, False, monkeypatch)
    assert fa == 0
    for f, s_ in zip(fo, so):
        for k, (x, y) in enumerate(zip(f, s_)):
            if torch.is_tensor(x):
                assert x.dtype == y.dtype and x.shape == y.shape, NAMES[k]
                assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8)), NAMES[k]
            else:
                assert x == y, NAMES[k]
    for a, b in zip(fs, ss):
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert np.array_equal(fz.cpu().numpy().view(np.uint8), sz.cpu().numpy().view(np.uint8))
    assert float(fz.abs().max()) > 0
    # at least one episode ended inside the compared rollouts (else the state reset is never exercised)
    assert sum(len(o[11]) for o in fo) > 0 and any(bool(o[2][1].any()) for o in fo)


# ---- 2. against numpy ---------------------------------------------------------------------------------------------------------
def test_zoo_lstm_rollout_matches_numpy_nets():
    N, T = 32, 16
    env = SumoVecEnv("RoboSumo-Ant-vs-Ant-v0", num_envs=N, seed=5)
    D, A = _dims(env)
    flat = golden("ant-lstm-v3")
    Dz, p = policy_zoo.split_zoo_lstm(flat, A)
    assert Dz == D - 1
    r, pl = _fix_runner(env, T, flat)
    assert r.fused_zoo_ok()
    _near_time_limit(env)
    out = r.run(250)
    torch.cuda.synchronize()
    assert env.stats()["rollout_aborts"] == 0
    gen = torch.Generator(device="cuda")
    gen.manual_seed(202)                                              # the zoo net's generator: its one [T, N, A] draw of the rollout
    noise1 = torch.randn((T, N, A), generator=gen, device="cuda", dtype=torch.float32).cpu().numpy().astype(np.float64)
    h = lambda k, *tail: out[k].cpu().numpy().reshape(2, N, T, *tail)  # sf01 order: env-major rows
    obs, done = h(0, D), h(2)
    act, val, nlp, onlp = [h(k, *tail).astype(np.float64) for k, tail in ((3, (A,)), (4, ()), (5, ()), (7, ()))]
    assert done[1].any(), "no episode of agent 1 ended inside the rollout"
    ls_l, ls_z = pl[10].astype(np.float64).ravel(), p["logstd"].astype(np.float64).ravel()
    state = np.zeros((4, N, 64), np.float32)
    zero = np.zeros((4, N, 64), np.float32)
    e_mean = e_on1 = e_on0 = 0.0
    for t in range(T):
        state[:, done[1, :, t] != 0, :] = 0                           # M = dones[:, 1] of the previous step
        mean1, _, state = po.zoo_lstm_step(p, obs[1, :, t, :Dz], state)
        state = state.astype(np.float32)
        mean0, _, _ = po.zoo_lstm_step(p, obs[0, :, t, :Dz], zero)    # the scoring call starts from zeros
        e_mean = max(e_mean, np.abs(act[1, :, t] - np.exp(ls_z) * noise1[t] - mean1).max())
        e_on1 = max(e_on1, np.abs(onlp[1, :, t] - po.neglogp(mean1.astype(np.float64), ls_z, act[1, :, t])).max())
        e_on0 = max(e_on0, np.abs(onlp[0, :, t] - po.neglogp(mean0.astype(np.float64), ls_z, act[0, :, t])).max())
    zs = r.zoo_state.cpu().numpy()
    e_state = max(np.abs(zs[:, :64] - state[2]).max(), np.abs(zs[:, 64:] - state[3]).max())
    print("zoo mean err %.3g, final state err %.3g, onlp[1] err %.3g, onlp[0] err %.3g (max |onlp| %.3g / %.3g)"
          % (e_mean, e_state, e_on1, e_on0, np.abs(onlp[1]).max(), np.abs(onlp[0]).max()))
    worst = []
    for g in range(2):
        mean_l, v_l, _ = po.forward(pl, obs[g].reshape(N * T, D).astype(np.float64))
        e_val = np.abs(val[g].ravel() - v_l).max()
        e_nlp = np.abs(nlp[g].ravel() - po.neglogp(mean_l, ls_l, act[g].reshape(N * T, A))).max()
        print("agent %d: learner value err %.3g (max |v| %.3g), nlp err %.3g (max |nlp| %.3g)" % (g, e_val, np.abs(v_l).max(), e_nlp, np.abs(nlp[g]).max()))
        worst.append((e_val, np.abs(v_l).max(), e_nlp, np.abs(nlp[g]).max()))
    assert e_mean < 5e-5 and e_state < 5e-5
    assert e_on1 < 1e-3 * (1 + np.abs(onlp[1]).max())
    assert e_on0 < 1e-3 * (1 + np.abs(onlp[0]).max())
    for e_val, vmax, e_nlp, nmax in worst:
        assert e_val < 2e-5 * (1 + vmax)
        assert e_nlp < 1e-3 * (1 + nmax)
    env.close()


# ---- 3. learn end to end ------------------------------------------------------------------------------------------------------
def _learn_ppo(path, log, fused_fix):
    from robosumo_selfplay_amd import alg_ppo
    env = SumoVecEnv("RoboSumo-Ant-vs-Ant-v0", num_envs=16, seed=1)
    model = alg_ppo.learn(network="mlp", env=env, seed=1, total_timesteps=16 * 16 * 2, nagent=2, log_dir=log, verbose=False, nsteps=16,
                          nminibatches=4, noptepochs=2, lr=1e-3, gamma=0.995, lam=1.0, rho_bar=10.0, c_bar=1.0, opponent_mode="fix",
                          fix_opponent_path=path, value_network="copy", num_hidden=64, activation="relu", anneal_bound=1000,
                          fused_fix_opponent=fused_fix)
    assert len(model.history["lossvals"]) == 2 and all(np.isfinite(l).all() for l in model.history["lossvals"])
    assert sum(model.history["env_rollout_aborts"]) == 0
    params = model.params.clone()
    env.close()
    return params


def test_learn_against_zoo_lstm_file(tmp_path, monkeypatch):
    """learn(opponent_mode='fix') with a zoo LSTM file: the fused launch and the step-by-step launches under the opt-in train the
    same parameters bit for bit; the plain step-by-step path (no opt-in) trains too; alg_ac.learn accepts the same file."""
    from robosumo_selfplay_amd import alg_ac, defaults
    path = os.path.join(str(tmp_path), "agent-params-lstm-test.npy")
    np.save(path, synthetic_lstm_flat(120, 8, 7))
    params = []
    for fused in (True, False):
        monkeypatch.setenv("SUMO_FUSED_ROLLOUT", "1" if fused else "0")
        params.append(_learn_ppo(path, os.path.join(str(tmp_path), "log%d" % fused), True))
    assert torch.isfinite(params[0]).all() and torch.equal(params[0], params[1])
    monkeypatch.setenv("SUMO_FUSED_ROLLOUT", "1")
    plain = _learn_ppo(path, os.path.join(str(tmp_path), "plain"), False)     # per-step draws from the policy's own generator
    assert torch.isfinite(plain).all()
    env = SumoVecEnv("RoboSumo-Ant-vs-Ant-v0", num_envs=16, seed=1)
    kw = defaults.get_default_params("RoboSumo-Ant-vs-Ant-v0", "ac")
    kw.update(nsteps=5)
    model = alg_ac.learn(network="mlp", env=env, seed=1, total_timesteps=16 * 5 * 2, nagent=2, log_dir=os.path.join(str(tmp_path), "ac"),
                         verbose=False, opponent_mode="fix", fix_opponent_path=path, fused_fix_opponent=True, **kw)
    assert len(model.history["lossvals"]) == 2 and all(np.isfinite(l).all() for l in model.history["lossvals"])
    assert torch.isfinite(model.params).all()
    env.close()


def test_fixed_opponent_model_wraps_a_zoo_lstm_policy():
    """What install_fixed_opponent builds for an LSTM file, driven as the host-mode Runner drives it (numpy in, S=None)."""
    A, Dz, n = 8, 120, 5
    zoo = policy_zoo.load_zoo_policy_from_flat(synthetic_lstm_flat(Dz, A, 4), A)
    assert isinstance(zoo, policy_zoo.ZooLSTMPolicy)
    m = policy_zoo.FixedOpponentModel(zoo)
    zoo.seed(1)
    rng = np.random.default_rng(0)
    ob = rng.standard_normal((n, Dz + 1)).astype(np.float32)
    a, _, S, nlp = m.step(ob, S=None, M=np.zeros(n, bool))
    assert S is None and a.shape == (n, A) and nlp.shape == (n,) and np.isfinite(a).all() and np.isfinite(nlp).all()
    h1 = zoo.state[3].clone()
    assert float(h1.abs().max()) > 0
    # scoring starts from zeros and writes no state; the first acting step started from zeros too, so it reproduces its neglogp
    nlp2 = m.act_model.action_probability(ob, given_action=a)
    assert torch.equal(zoo.state[3], h1) and np.array_equal(nlp2.view(np.uint8), nlp.view(np.uint8))
    # M zeroes the rows it marks before the cell runs: row 2 acts as from a fresh state, row 1 does not
    M = np.zeros(n, bool); M[2] = True
    a3 = m.step(ob, S=None, M=M, deterministic=True)[0]
    fresh = zoo.evaluate(torch.from_numpy(ob).cuda(), state=torch.zeros((n, 128), device="cuda"), deterministic=True)["action"].cpu().numpy()
    assert np.array_equal(a3[2].view(np.uint8), fresh[2].view(np.uint8)) and not np.array_equal(a3[1], fresh[1])
    assert np.isfinite(m.value(ob, S=None, M=M)).all()


# ---- 4. loud failures ---------------------------------------------------------------------------------------------------------
def test_zoo_lstm_rollout_launch_refusals():
    N, T = 16, 4
    env = SumoVecEnv("RoboSumo-Ant-vs-Ant-v0", num_envs=N, seed=2)
    D, A = _dims(env)
    zoo = policy_zoo.ZooLstmTable([synthetic_lstm_flat(D - 1, A, 20 + j) for j in range(2)], A, env.device)
    r, _ = _fix_runner(env, T, synthetic_lstm_flat(D - 1, A, 9))
    B = r._alloc_device(T)
    noise = [torch.randn((T, N, A), device="cuda") for _ in range(2)]
    learner = r.models[0].act_model
    st1 = torch.zeros((N, 128), dtype=torch.float32, device="cuda")
    E, bufs = env.engine, env.env_ptrs(0)

    def ro(**kw):
        o = capi.Rollout(learner_params=learner.params.data_ptr(), opponent_params=None, opponent_index=None, npool=2, ob_dim=D, ac_dim=A,
                         T=T, Ntot=N, env_offset=0, s0=0, K=T, alpha=0.5, noise0=noise[0].data_ptr(), noise1=noise[1].data_ptr())
        for f in ("obs", "act", "rew", "val", "nlp", "onlp", "done", "ep_done", "ep_r", "ep_l"):
            setattr(o, f, B[f].data_ptr())
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def zs(**kw):
        z = zoo.struct(st1)
        for k, v in kw.items():
            setattr(z, k, v)
        return z

    idx = torch.ones(N, dtype=torch.int32, device="cuda")
    E.rollout_steps_zoo_lstm(ro(opponent_index=idx.data_ptr()), zs(), *bufs)          # a good launch, net 1 of the table
    E.rollout_status()
    bad = idx.clone(); bad[3] = 2
    E.rollout_steps_zoo_lstm(ro(opponent_index=bad.data_ptr()), zs(), *bufs)          # an index outside the table
    with pytest.raises(capi.SumoHipError, match="cut short"):
        E.rollout_status()
    env.reset_device()
    # refused before any launch
    for field, rkw, zkw in (("opponent_params", dict(opponent_params=learner.params.data_ptr()), {}), ("nzoo", {}, dict(nzoo=1)),
                            ("nzoo", dict(npool=0), dict(nzoo=0)), ("ob_dim", {}, dict(ob_dim=D + 1)), ("ob_dim", {}, dict(ob_dim=0)),
                            ("ob_dim", dict(ob_dim=D - 1), {}), ("params", {}, dict(params=None)), ("filt", {}, dict(filt=None)),
                            ("state", {}, dict(state=None)), ("obs_clip", {}, dict(obs_clip=0.0)), ("hidden", {}, dict(hidden=128)),
                            ("emb_dim", {}, dict(emb_dim=32)), ("missing", dict(noise1=None), {}), ("missing", dict(onlp=None), {}),
                            ("outside", dict(K=T + 1), {})):
        with pytest.raises(capi.SumoHipError, match=field):
            E.rollout_steps_zoo_lstm(ro(**rkw), zs(**zkw), *bufs)
    E.set_cfrc_mode("rne_post")
    with pytest.raises(capi.SumoHipError, match="rne_post"):
        E.rollout_steps_zoo_lstm(ro(), zs(), *bufs)
    E.set_cfrc_mode("zero")
    env.reset_device()
    env.close()
    mixed = SumoVecEnv("RoboSumo-Ant-vs-Bug-v0", num_envs=4, seed=2)                  # mixed match-ups stay refused
    with pytest.raises(capi.SumoHipError, match="homogeneous"):
        mixed.engine.rollout_steps_zoo_lstm(ro(Ntot=4), zs(), *mixed.env_ptrs(0))
    mixed.close()
