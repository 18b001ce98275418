"""GPU tests of the A2C learner: ppo_a2c_grad / ppo_a2c_loss_stats against the float64 restatement (tests/a2c_ref.py),
ActorCriticModel's optimiser step, checkpoint interchange with PPOModel, and alg_ac.learn end to end on the real env."""
import os

import numpy as np
import pytest

from conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch
    from a2c_ref import a2c_loss_and_grads, a2c_train_step
    from oracle import ppo_oracle as po
    from robosumo_selfplay_amd import model as model_mod, policies, ppo_capi
    from robosumo_selfplay_amd.a2c_model import ActorCriticModel

    DEV = torch.device("cuda:0")


def _spec(ob=121, ac=8):
    return policies.PolicySpec(ob, ac, value_network="copy", activation="relu")


def _perturb(m, rng, scale=0.1):
    pl = [p + rng.normal(0, scale, p.shape).astype(np.float32) for p in m.get_param_list()]
    m.set_param_list(pl)
    return pl


def _batch(rng, NB, ob, ac, pl):
    obs = rng.normal(0, 1, (NB, ob)).astype(np.float32)
    mean, _, _ = po.forward(pl, obs)
    act = (mean + np.exp(pl[10].astype(np.float64)) * rng.normal(0, 1, (NB, ac))).astype(np.float32)
    ret = rng.normal(0, 2, NB).astype(np.float32)
    val = rng.normal(0, 2, NB).astype(np.float32)
    w = rng.uniform(0.25, 3.0, NB).astype(np.float32)
    return obs, act, ret, val, w


def _a2c_grad(m, d, idx, n, ent_coef, vf_coef):
    """adv moments + normalise + ppo_a2c_grad + ppo_a2c_loss_stats; returns (grads, stats[8], out3) as numpy."""
    L = ppo_capi.lib()
    ob, ac = m.spec.ob_dim, m.spec.ac_dim
    d_obs, d_act, d_ret, d_val, d_w = d
    ip = ppo_capi.ptr(idx)
    mom = torch.zeros(3, dtype=torch.float64, device=DEV)
    ppo_capi.chk(L.ppo_adv_moments(d_ret.data_ptr(), d_val.data_ptr(), ip, n, mom.data_ptr(), None))
    adv = torch.empty(n, dtype=torch.float32, device=DEV)
    ppo_capi.chk(L.ppo_adv_normalize(d_ret.data_ptr(), d_val.data_ptr(), ip, n, mom.data_ptr(), adv.data_ptr(), None))
    g = torch.zeros(m.P, dtype=torch.float32, device=DEV)
    st = torch.zeros(8, dtype=torch.float64, device=DEV)
    ppo_capi.chk(L.ppo_a2c_grad(m.params.data_ptr(), d_obs.data_ptr(), ob, ob, ac, d_act.data_ptr(), adv.data_ptr(), d_ret.data_ptr(),
                                d_w.data_ptr(), ip, n, 1.0 / n, ent_coef, vf_coef, g.data_ptr(), st.data_ptr(), m.workspace.data_ptr(), None))
    out3 = torch.empty(3, dtype=torch.float64, device=DEV)
    off = m.P - 1 - policies.HIDDEN - ac
    ppo_capi.chk(L.ppo_a2c_loss_stats(st.data_ptr(), m.params.data_ptr() + 4 * off, ac, out3.data_ptr(), None))
    torch.cuda.synchronize()
    return g.cpu().numpy(), st.cpu().numpy(), out3.cpu().numpy()


@pytest.mark.parametrize("n", [1, 17, 512, 20480])
def test_a2c_gradients_match_restatement(n):
    """Kernel vs float64 restatement, ob 121 / ac 8, rows gathered through idx from 2n data rows, IS weights in [0.25, 3]: relative
    error of every parameter tensor < 2e-4 (as test_gpu_ppo's ppo_grad check); loss sums and sum of weights; deterministic."""
    rng = np.random.RandomState(11 + n)
    ob, ac = 121, 8
    m = ActorCriticModel(policy=_spec(ob, ac), ent_coef=0.01, vf_coef=0.5)
    pl = _perturb(m, rng)
    NB = 2 * n
    obs, act, ret, val, w = _batch(rng, NB, ob, ac, pl)
    idx = rng.permutation(NB)[:n].astype(np.int32)
    advs = po.normalize_advantages(ret[idx], val[idx])
    _, stats, sums, grads = a2c_loss_and_grads(pl, obs[idx], act[idx], advs, ret[idx], w[idx], 0.01, 0.5)
    up = lambda x: torch.as_tensor(x).to(DEV)
    d = tuple(up(x) for x in (obs, act, ret, val, w))
    d_idx = up(idx)
    g, s, out3 = _a2c_grad(m, d, d_idx, n, 0.01, 0.5)
    gl = policies.unflatten_params(g, ob, ac)
    for k, (a, b) in enumerate(zip(gl, grads)):
        b = np.asarray(b).reshape(a.shape)
        err = np.abs(a - b).max() / (np.abs(b).max() + 1e-12)
        assert err < 2e-4, (policies.PARAM_NAMES[k], err)
    assert s[6] == n and s[3] == 0 and s[4] == 0
    assert s[0] == pytest.approx(sums[0], rel=1e-4, abs=1e-6 * n) and s[1] == pytest.approx(sums[1], rel=1e-4)
    assert s[5] == pytest.approx(sums[2], rel=1e-6)
    assert out3[0] == pytest.approx(stats[0], rel=1e-4, abs=1e-6) and out3[1] == pytest.approx(stats[1], rel=1e-4)
    assert out3[2] == pytest.approx(stats[2], rel=1e-6)
    g2, s2, _ = _a2c_grad(m, d, d_idx, n, 0.01, 0.5)
    assert np.array_equal(g, g2) and np.array_equal(s, s2), "ppo_a2c_grad must be deterministic"


def test_a2c_train_step_matches_restatement():
    """ActorCriticModel.train: one whole-batch step from fresh Adam state vs restatement + clip_by_global_norm + TF1 Adam, within
    the tolerances of test_gpu_ppo's PPOModel step check; the returned [pg, vf, entropy] as well."""
    rng = np.random.RandomState(4)
    ob, ac, n = 121, 8, 512
    m = ActorCriticModel(policy=_spec(ob, ac), ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5)
    pl = _perturb(m, rng, 0.05)
    obs, act, ret, val, w = _batch(rng, n, ob, ac, pl)
    out = m.train(1e-3, obs, ret, np.zeros(n, bool), act, val, np.zeros(n, np.float32), ret, w)
    assert len(out) == 3 and m.loss_names == ["policy_loss", "value_loss", "policy_entropy"]
    newp, stats = a2c_train_step(pl, obs, act, ret, val, w, 1e-3)
    for k, (a, b) in enumerate(zip(m.get_param_list(), newp)):
        assert np.allclose(a, b, rtol=0, atol=5e-6), (policies.PARAM_NAMES[k], np.abs(a - b).max())
    assert float(out[0]) == pytest.approx(stats[0], rel=1e-3, abs=1e-5) and float(out[1]) == pytest.approx(stats[1], rel=1e-4)
    assert float(out[2]) == pytest.approx(stats[2], rel=1e-6)


def test_a2c_graph_replay_matches_eager():
    """The HIP-graph path of ActorCriticModel (captured on the second step of a batch size) gives the eager launches' results bit
    for bit, across a change of batch size."""
    rng = np.random.RandomState(8)
    ob, ac = 121, 8
    ma = ActorCriticModel(policy=_spec(ob, ac))
    mb = ActorCriticModel(policy=_spec(ob, ac))
    mb.use_graph = False
    mb.set_param_list(ma.get_param_list())
    up = lambda x: torch.as_tensor(x).to(DEV)
    for step, n in enumerate([640, 640, 640, 333, 333, 333]):
        obs, act, ret, val, w = (up(x) for x in _batch(rng, n, ob, ac, ma.get_param_list()))
        oa = ma.train_device(3e-4, obs, ret, act, val, w)
        ob_ = mb.train_device(3e-4, obs, ret, act, val, w)
        assert torch.equal(oa, ob_) and torch.equal(ma.params, mb.params), step
    assert len(ma._graphs) == 2


def test_ppo_checkpoint_loads_into_a2c_and_back(tmp_path):
    np.random.seed(1)
    ppo = model_mod.PPOModel(policy=_spec(), trainable=False)
    np.random.seed(2)
    a2c = ActorCriticModel(policy=_spec())
    assert not torch.equal(ppo.params, a2c.params)
    ppo.save(str(tmp_path / "ppo"))
    a2c.load(str(tmp_path / "ppo"))
    assert torch.equal(ppo.params, a2c.params)
    a2c.train(1e-3, *[np.random.normal(0, 1, s).astype(np.float32) for s in ((64, 121), (64,), (64,), (64, 8), (64,), (64,), (64,))],
              np.ones(64, np.float32))
    a2c.save(str(tmp_path / "a2c"))
    back = model_mod.PPOModel(policy=_spec(), trainable=False)
    back.load(str(tmp_path / "a2c"))
    assert back.params.cpu().numpy().tobytes() == a2c.params.cpu().numpy().tobytes()
    assert not torch.equal(back.params, ppo.params)


@pytest.mark.parametrize("mode,opp_data,nupd", [("ours", None, 40), ("latest", None, 40), ("random", "direct", 12)])
def test_learn_a2c_end_to_end(mode, opp_data, nupd, tmp_path):
    """alg_ac.learn on Ant-vs-Ant, 256 envs, nsteps 5: finite losses, checkpoints 00000 .. last, no aborted rollouts, weights moved."""
    from robosumo_selfplay_amd import alg_ac, defaults
    from robosumo_selfplay_amd.vec_env import SumoVecEnv
    env = SumoVecEnv("RoboSumo-Ant-vs-Ant-v0", num_envs=256, seed=7)
    kw = defaults.get_default_params("RoboSumo-Ant-vs-Ant-v0", "ac")
    kw.update(save_interval=4, log_interval=10)
    model = alg_ac.learn(network="mlp", env=env, seed=7, total_timesteps=256 * 5 * nupd, nagent=2, log_dir=str(tmp_path), verbose=False,
                         opponent_mode=mode, use_opponent_data=opp_data, **kw)
    h = model.history
    p0 = policies.flatten_params(__import__("joblib").load(os.path.join(str(tmp_path), "checkpoints", "00000")))
    env.close()
    assert len(h["lossvals"]) == nupd and all(np.isfinite(l).all() for l in h["lossvals"]) and model.t == nupd
    ck = sorted(os.listdir(os.path.join(str(tmp_path), "checkpoints")))
    assert ck[0] == "00000" and "00001" in ck and ck[-1] == "%.5i" % nupd and len(ck) == 2 + nupd // 4
    assert sum(h["env_rollout_aborts"]) == 0 and len(h["env_rollout_aborts"]) == nupd
    assert torch.isfinite(model.params).all() and not np.array_equal(model.params.cpu().numpy(), p0)
    if mode == "ours":
        assert all(v == [0] for v in h["opponent_versions"])
    elif mode == "latest":
        assert h["opponent_versions"][1] == [1] and h["opponent_versions"][-1] == [nupd - nupd % 4 if nupd % 4 else nupd - 4]
    else:
        assert all(0 < u <= 1 for u in h["useful_ratio"])
