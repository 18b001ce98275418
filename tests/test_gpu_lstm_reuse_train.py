"""Training a recurrent learner on reused opponent samples, on the GPU: LstmPPOModel.loss_and_grads / train with a row mask against the
float64 masked reference (tests/lstm_reuse_ref.py, verified on the CPU against the oracle function and finite differences), the point
of the shadow state (agent 1's recorded neglogp is the trained function's own: ratio 1 before the first step), and
learn(network='lstm', use_opponent_data=...) end to end."""
import numpy as np
import pytest

import lstm_reuse_ref as R
from conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch
    from robosumo_selfplay_amd import alg_ppo, lstm_model
    from robosumo_selfplay_amd.vec_env import SumoVecEnv
    from oracle import ppo_oracle as po
    from test_gpu_lstm_train import _batch


def _problem(H, seed=0, T=5, n=6, D=121, A=8):
    """n = 6 sequences of T = 5 rows; mixed masks, sequence 3 without a valid row, weights != 1; the per-row inputs of invalid rows
    are NaN (they must reach nothing)."""
    rng = np.random.default_rng(seed)
    np.random.seed(1)
    m = lstm_model.LstmPPOModel(policy=lstm_model.LstmSpec(D, A, H), ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5, nbatch_act=n, nsteps=T)
    pl = [p + rng.normal(0, 0.05, p.shape).astype(np.float32) for p in m.get_param_list()]
    pl[5] = rng.normal(-0.3, 0.1, (1, A)).astype(np.float32)
    m.set_param_list(pl)
    obs, masks, actions, returns, values, S0 = _batch(rng, T, n, D, A, H)
    tm = lambda x: np.swapaxes(x, 0, 1)
    state = S0.copy()
    old = np.zeros((T, n), np.float32)
    for t in range(T):
        h, state = po.lstm_step_baselines(pl[0], pl[1], pl[2], tm(obs)[t], state, tm(masks)[t].astype(np.float32))
        old[t] = po.neglogp(h @ pl[3] + pl[4], pl[5], tm(actions)[t])
    old = np.swapaxes((old + rng.normal(0, 0.25, (T, n))).astype(np.float32), 0, 1)          # [n, T], some ratios clipped
    w = rng.uniform(0.5, 1.5, (n, T)).astype(np.float32)
    valid = (rng.random((n, T)) < 0.6).astype(np.float32)
    valid[3] = 0.0
    valid[0, 0], valid[0, 1] = 1.0, 0.0
    bad = valid == 0
    returns_m, old_m, w_m = (np.where(bad, np.float32("nan"), x) for x in (returns, old, w))
    return dict(m=m, pl=pl, obs=obs, masks=masks, actions=actions, returns=returns_m, values=values, S0=S0, old=old_m, w=w_m, valid=valid,
                T=T, n=n)


@pytest.mark.parametrize("H", [64, 128])
def test_masked_loss_and_grads_match_the_float64_reference(H):
    """Tolerances of tests/test_gpu_lstm_train.py::test_bptt_gradients_match_oracle (the unmasked comparison)."""
    p = _problem(H)
    m, T, n = p["m"], p["T"], p["n"]
    rng = np.random.default_rng(9)
    advs = rng.normal(0, 1, (n, T)).astype(np.float32)
    advs = np.where(p["valid"] == 0, np.float32("nan"), advs)
    flat = lambda x: np.ascontiguousarray(x).reshape(n * T, *x.shape[2:])
    tm = lambda x: np.swapaxes(x, 0, 1)
    nv = int(p["valid"].sum())
    m.moments[2] = float(nv)                 # what ppo_adv_moments_masked_ws leaves there in a training step
    m.loss_and_grads(0.2, flat(p["obs"]), flat(p["returns"]), flat(p["masks"]), flat(p["actions"]), flat(advs), flat(p["old"]), flat(p["w"]),
                     p["S0"], T, valid=flat(p["valid"]))
    torch.cuda.synchronize()
    loss, stats, grads, _, cnt = R.masked_loss_and_grads(p["pl"], tm(p["obs"]), tm(p["masks"]), tm(p["actions"]), tm(advs), tm(p["returns"]),
                                                          tm(p["old"]), tm(p["w"]), tm(p["valid"]), p["S0"], 0.2, 0.01, 0.5)
    s = m.stats.cpu().numpy()
    assert s[6] == cnt == nv and 0 < nv < n * T and np.isfinite(s).all()
    assert np.allclose([s[0] / s[6], s[1] / s[6], s[3] / s[6], s[4] / s[6]], [stats[0], stats[1], stats[3], stats[4]], rtol=2e-4, atol=2e-5)
    for name, gv, go in zip(lstm_model.policies.LSTM_PARAM_NAMES, m.gviews, grads):
        g = gv.cpu().numpy().astype(np.float64)
        scale = np.abs(go).max() + 1e-8
        assert np.isfinite(g).all() and np.abs(g - go.reshape(g.shape)).max() < 3e-4 * scale + 1e-7, (name, np.abs(g - go.reshape(g.shape)).max(), scale)


@pytest.mark.parametrize("H", [64, 128])
def test_masked_graph_replay_matches_eager_steps(H):
    """Criterion of tests/test_gpu_lstm_train.py::test_graph_replay_matches_eager_recurrent_steps: same parameters and statistics
    over several steps with changing inputs -- here the mask changes too (one graph, the count is read on the device), down to a
    minibatch without a valid row, which steps on the entropy term's gradient alone."""
    p = _problem(H, seed=4)
    T, n = p["T"], p["n"]
    flat = lambda x: np.ascontiguousarray(x).reshape(n * T, *x.shape[2:])
    dev = lambda x, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(x)).to("cuda", dt)
    base = [dev(flat(p["obs"])), dev(flat(p["returns"])), dev(flat(p["masks"]).astype(np.float32)), dev(flat(p["actions"])), dev(flat(p["values"]))]
    old, w, S = dev(flat(p["old"])), dev(flat(p["w"])), dev(p["S0"])
    rng = np.random.default_rng(2)
    valids = [flat(p["valid"]), (rng.random(n * T) < 0.5).astype(np.float32), np.zeros(n * T, np.float32), np.ones(n * T, np.float32)]
    res = []
    for use_graph in (True, False):
        np.random.seed(3)
        m = lstm_model.LstmPPOModel(policy=lstm_model.LstmSpec(121, 8, H), ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5, nbatch_act=n, nsteps=T)
        m.set_param_list(p["pl"])
        m.use_graph = use_graph
        outs = []
        for k, v in enumerate(valids):
            # (rows that are NaN under the first mask are filled in: the other masks make them valid)
            fill = lambda x: torch.nan_to_num(x, nan=0.5)
            outs.append(m.train(1e-3, 0.2, base[0] + 0.01 * k, fill(base[1]), base[2], base[3], base[4], fill(old), None, fill(w),
                                states=S, valid=dev(v))[:5])
            assert all(np.isfinite(float(x)) for x in outs[-1])
        assert (len(m._graphs) == 1) == use_graph
        assert m.t == len(valids)
        assert [float(x) for x in outs[2][:2]] + [float(outs[2][3]), float(outs[2][4])] == [0.0] * 4        # no valid row: zero statistics
        res.append((m.params.clone(), np.asarray(outs, np.float64)))
    assert torch.equal(res[0][0], res[1][0])
    assert np.array_equal(res[0][1], res[1][1])


def _rollout(reuse, N=32, T=8):
    from test_gpu_lstm_reuse_rollout import _run_pair
    return _run_pair(N, T, 1, 0, True, reuse=reuse, runs=1)


def test_shadow_state_makes_agent1_rows_on_policy():
    """A reuse rollout (N = 32, T = 8), then ``train`` with lr = 0 on agent 1's sequences alone -- start states ``shadow_state0``, masks
    ``masks[1]``, old neglogp ``neglogpacs[1]``, every row valid: |approxkl| < 1e-4 and clipfrac == 0 at cliprange 0.2, the bound
    tests/test_gpu_lstm_train.py puts on a learner's own rows.  The counter-example (printed, not asserted): the same call with the
    neglogp a rollout WITHOUT the mode records for agent 1 -- the learner's from a zero state at every step -- as "old"; measured on
    this shape: approxkl 1.52 and clipfrac 0.75 against 2.1e-07 and 0 with the shadow state's neglogp, i.e. three quarters of the
    reused rows would start outside the clip range."""
    N, T = 32, 8
    on, off = _rollout(True, N, T), _rollout(False, N, T)
    out = on["outs"][0]
    obs, returns, masks, actions, values, nlp = out[0], out[1], out[2], out[3], out[4], out[5]
    assert torch.equal(actions[1], off["outs"][0][3][1])               # same stream: only what is recorded about it differs

    def step(old):
        np.random.seed(0)
        m = lstm_model.LstmPPOModel(policy=on["learner"].spec, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, nbatch_act=N, nsteps=T)
        m.set_param_list(on["learner"].get_param_list())
        ones = torch.ones(N * T, dtype=torch.float32, device="cuda")
        o = m.train(0.0, 0.2, obs[1].contiguous(), returns[1], masks[1], actions[1].contiguous(), values[1], old, None, ones,
                    states=on["starts"][0], nsteps=T, valid=ones)
        return float(o[3]), float(o[4])
    kl, cf = step(nlp[1])
    kl0, cf0 = step(off["outs"][0][5][1])
    print("agent 1's rows, lr = 0: shadow-state neglogp -> approxkl %.3g clipfrac %.3g; zero-state neglogp -> approxkl %.3g clipfrac %.3g"
          % (kl, cf, kl0, cf0))
    assert abs(kl) < 1e-4 and cf == 0.0


@pytest.mark.parametrize("mode", ["direct", "both"])
def test_learn_lstm_with_opponent_data_reuse(mode, tmp_path, monkeypatch):
    calls = {"n": 0}
    orig = SumoVecEnv.rollout_steps_lstm_reuse_group

    def counted(self, g, ro):
        calls["n"] += 1
        return orig(self, g, ro)
    monkeypatch.setattr(SumoVecEnv, "rollout_steps_lstm_reuse_group", counted)
    params = []
    for fused in ("1", "0"):
        monkeypatch.setenv("SUMO_FUSED_ROLLOUT", fused)
        env = SumoVecEnv("RoboSumo-Ant-vs-Ant-v0", num_envs=32, seed=8)
        model = alg_ppo.learn(network="lstm", env=env, seed=3, total_timesteps=32 * 8 * 3, nagent=2, log_dir=str(tmp_path / fused), verbose=False,
                              nsteps=8, nminibatches=2, noptepochs=1, lr=3e-4, gamma=0.995, lam=0.95, rho_bar=1.0, c_bar=1.0,
                              opponent_mode="latest", nlstm=128, anneal_bound=1000, use_opponent_data=mode)
        assert calls["n"] == 3                                          # (cumulative) three updates through the reuse launch, none step by step
        assert all(np.isfinite(l).all() for l in model.history["lossvals"]) and torch.isfinite(model.params).all()
        assert len(model.history["useful_ratio"]) == 3 and all(0.0 < u <= 1.0 for u in model.history["useful_ratio"])
        assert model.t == 3 * 2
        params.append(model.params.clone())
        env.close()
    assert torch.equal(params[0], params[1])
