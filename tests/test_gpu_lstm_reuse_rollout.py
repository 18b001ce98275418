"""The recurrent rollout under opponent-data reuse (Runner.reuse_opponent: the learner's shadow state along agent 1's stream) on the
GPU: the fused launch sumo_rollout_steps_lstm_reuse against the step-by-step launches (bit for bit), the mode against the same
rollout without it (only agent 1's values / neglogp and what V-trace makes of them may move), the recorded numbers against the
numpy oracle replayed from the shadow start state, and the C ABI's refusals."""
import ctypes as C

import numpy as np
import pytest

from conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch
    from robosumo_selfplay_amd import capi, lstm_model
    from robosumo_selfplay_amd.runner import Runner
    from robosumo_selfplay_amd.vec_env import SumoVecEnv
    from oracle import ppo_oracle as po
    from test_gpu_lstm_rollout import NAMES, _models

# the entries of run()'s tuple that the shadow state may change: agent 1's rows of returns / values / neglogpacs, the three ratios
MOVED = {"returns": 1, "values": 4, "neglogpacs": 5, "off_policy_ratio": 12, "off_env_ratio": 13, "total_ratio": 14}


def _run_pair(N, T, groups, pool_k, fused, reuse=True, chunk=0, seed=5, runs=2):
    """tests/test_gpu_lstm_rollout.py::_run_pair with ``reuse_opponent``: a third of the envs placed just before the time limit so
    that episodes end (done flags -> masked states, auto-reset) inside the rollout."""
    env = SumoVecEnv("RoboSumo-Ant-vs-Ant-v0", num_envs=N, seed=21, groups=groups)
    learner, opp = _models(N, T, 128, pool_k, seed, env.observation_space[0].shape[0], env.action_space[0].shape[0])
    r = Runner(env=env, models=[learner, opp], nsteps=T, nagent=2, gamma=0.995, lam=0.95, rho_bar=1.0, c_bar=1.0, anneal_bound=500)
    for E in env.engines:
        qpos, qvel, warm, cnt = E.get_state()
        cnt[::3, 0] = 500 - 1 - (np.arange(len(cnt[::3])) % 7)
        E.set_state(qpos, qvel, warm, cnt)
    assert r.device_mode and r.recurrent and r.shadow_state.shape == (N, 256) and not r.shadow_state.any()
    r.reuse_opponent = reuse
    r.fused_rollout = fused
    r.rollout_chunk = chunk
    assert r.fused_lstm_ok() == fused
    outs, starts = [], []
    for k in range(runs):
        outs.append(r.run(250 + k))
        starts.append(None if r.shadow_state0 is None else r.shadow_state0.clone())
    torch.cuda.synchronize()
    res = dict(outs=outs, starts=starts, states=[s.clone() for s in r.states], shadow=r.shadow_state.clone(),
               engine=[E.get_state() for E in env.engines], stats=env.stats(), learner=learner)
    env.close()
    return res


def _assert_same(a, b, skip=()):
    for f, s_ in zip(a["outs"], b["outs"]):
        for k, (x, y) in enumerate(zip(f, s_)):
            if NAMES[k] in skip:
                continue
            if torch.is_tensor(x):
                assert torch.equal(x, y), (NAMES[k], (x != y).sum().item())
            else:
                assert x == y, NAMES[k]
    for x, y in zip(a["states"], b["states"]):
        assert torch.equal(x, y)
    for p, q in zip(a["engine"], b["engine"]):
        for x, y in zip(p, q):
            assert np.array_equal(x, y)
    for k in ("forward", "newton", "contacts", "efc", "dropped", "diverged", "rollout_aborts"):
        assert a["stats"][k] == b["stats"][k], k


@pytest.mark.parametrize("N,T,groups,pool_k,chunk", [(32, 9, 1, 0, 4), (48, 14, 1, 0, 0), (64, 10, 2, 3, 0)])
def test_fused_reuse_rollout_matches_stepwise_path(N, T, groups, pool_k, chunk, monkeypatch):
    calls = {"n": 0}
    orig = SumoVecEnv.rollout_steps_lstm_reuse_group

    def counted(self, g, ro):
        calls["n"] += 1
        return orig(self, g, ro)
    monkeypatch.setattr(SumoVecEnv, "rollout_steps_lstm_reuse_group", counted)
    fused = _run_pair(N, T, groups, pool_k, True, chunk=chunk)
    assert calls["n"] == 2 * groups * (-(-T // chunk) if chunk else 1)          # the reuse launch, not sumo_rollout_steps_lstm
    step = _run_pair(N, T, groups, pool_k, False)
    assert calls["n"] == 2 * groups * (-(-T // chunk) if chunk else 1)
    _assert_same(fused, step)
    assert torch.equal(fused["shadow"], step["shadow"]) and fused["shadow"].any()
    for x, y in zip(fused["starts"], step["starts"]):
        assert torch.equal(x, y)
    assert not fused["starts"][0].any() and torch.equal(fused["starts"][1], _run_pair(N, T, groups, pool_k, True, chunk=chunk, runs=1)["shadow"])
    outs = fused["outs"]
    assert outs[0][2].any() and outs[0][2][1].any() and len(outs[0][11]) > 0     # done flags occurred (agent 1's too)
    assert torch.isfinite(outs[1][4]).all() and torch.isfinite(outs[1][5]).all() and fused["stats"]["diverged"] == 0


def test_reuse_disturbs_nothing_else():
    """Step-by-step path, same seeds, reuse on against off: bitwise equal but for agent 1's values / neglogp, the returns V-trace
    computes from them and the three ratios."""
    on = _run_pair(32, 9, 1, 0, False, reuse=True)
    off = _run_pair(32, 9, 1, 0, False, reuse=False)
    _assert_same(on, off, skip=tuple(MOVED))
    for f, s_ in zip(on["outs"], off["outs"]):
        for name in ("returns", "values", "neglogpacs"):
            k = MOVED[name]
            assert torch.equal(f[k][0], s_[k][0]), name                       # agent 0's rows
        assert not torch.equal(f[4][1], s_[4][1]) and not torch.equal(f[5][1], s_[5][1])
    assert off["starts"] == [None, None] and not off["shadow"].any()          # the shadow state is advanced in this mode only


def _replay(learner, start, obs, done, act, T):
    """The oracle's recurrent step + neglogp along one agent's recorded stream [N * T, ...] (env-major) from ``start`` [N, 2H]:
    -> (neglogp [N * T], value [N * T], final state)."""
    pl = [p.astype(np.float32) for p in learner.get_param_list()]
    N = start.shape[0]
    o, d, a = (x.cpu().numpy().reshape(N, T, *x.shape[1:]) for x in (obs, done, act))
    state = start.cpu().numpy().copy()
    nlp, val = np.zeros((N, T), np.float64), np.zeros((N, T), np.float64)
    for t in range(T):
        h, state = po.lstm_step_baselines(pl[0], pl[1], pl[2], o[:, t], state, d[:, t].astype(np.float32))
        nlp[:, t] = po.neglogp(h @ pl[3] + pl[4], pl[5], a[:, t])
        val[:, t] = (h @ pl[6] + pl[7])[:, 0]
    return nlp.reshape(-1), val.reshape(-1), state


def test_recorded_agent1_numbers_are_the_learners_along_agent1s_stream():
    """Replay obs[1], done[1], actions[1] through oracle.ppo_oracle.lstm_step_baselines + neglogp from the shadow start state: the
    recorded neglogpacs[1], values[1] and the final shadow state within rtol 1e-5 / atol 1e-5 (the tolerance of
    tests/test_gpu_lstm_train.py for action_probability against these oracle functions); T = 9, two consecutive rollouts.  Measured
    worst error over tolerance: agent 1 (the new path) neglogp 0.036 / value 0.117, agent 0 (the parent's path, same replay) neglogp
    0.040 / value 0.089 -- both an order of magnitude inside, so the bound stands as it is for both."""
    T = 9
    res = _run_pair(32, T, 1, 0, True)
    worst = {}
    for k, (out, start) in enumerate(zip(res["outs"], res["starts"])):
        obs, masks, actions, values, nlp = out[0], out[2], out[3], out[4], out[5]
        for g, st in ((0, out[10]), (1, start)):
            n_ref, v_ref, S_ref = _replay(res["learner"], st, obs[g], masks[g], actions[g], T)
            e_n = np.abs(nlp[g].cpu().numpy() - n_ref) / (1e-5 + 1e-5 * np.abs(n_ref))
            e_v = np.abs(values[g].cpu().numpy() - v_ref) / (1e-5 + 1e-5 * np.abs(v_ref))
            worst[(k, g)] = (float(e_n.max()), float(e_v.max()))
            print("rollout %d agent %d: worst error / tolerance  neglogp %.3f  value %.3f" % (k, g, e_n.max(), e_v.max()))
            assert e_n.max() <= 1.0 and e_v.max() <= 1.0, (k, g, worst[(k, g)])
    final = res["shadow"].cpu().numpy()
    assert np.allclose(final, S_ref, rtol=1e-5, atol=1e-5), np.abs(final - S_ref).max()


def test_c_abi_refuses_what_the_recurrent_launch_refuses():
    env = SumoVecEnv("RoboSumo-Ant-vs-Ant-v0", num_envs=16, seed=2)
    z = torch.zeros(16 * 4 * 2 * 121, dtype=torch.float32, device="cuda")

    def struct(H):
        m = lstm_model.LstmPPOModel(policy=lstm_model.LstmSpec(121, 8, H), nbatch_act=16, nsteps=4, trainable=False)
        ro = capi.RolloutLstmReuse()
        ro.learner = C.addressof(m._net)
        for f in ("opponents_dev", "state0", "state1", "state2", "noise0", "noise1", "obs", "act", "rew", "val", "nlp", "onlp", "done", "ep_done",
                  "ep_r", "ep_l"):
            setattr(ro, f, z.data_ptr())
        ro.npool, ro.T, ro.Ntot, ro.env_offset, ro.s0, ro.K, ro.alpha = 1, 4, 16, 0, 0, 4, 0.5
        return m, ro
    m64, ro = struct(64)
    with pytest.raises(capi.SumoHipError, match="hidden 128"):
        env.rollout_steps_lstm_reuse_group(0, ro)
    m128, ro = struct(128)
    ro.K = 5
    with pytest.raises(capi.SumoHipError, match="outside the rollout buffers"):
        env.rollout_steps_lstm_reuse_group(0, ro)
    ro.K, ro.env_offset = 4, 1
    with pytest.raises(capi.SumoHipError, match="outside the rollout buffers"):
        env.rollout_steps_lstm_reuse_group(0, ro)
    ro.env_offset, ro.state2 = 0, None
    with pytest.raises(capi.SumoHipError, match="state2"):
        env.rollout_steps_lstm_reuse_group(0, ro)
    assert env.stats()["rollout_aborts"] == 0
    env.close()
