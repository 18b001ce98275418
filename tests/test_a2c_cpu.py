"""CPU checks of the A2C learner (--algo ac): defaults, CLI routing, the C ABI exports, the float64 restatement of the loss
gradient (tests/a2c_ref.py) against finite differences, and the configurations learn() refuses before touching the GPU."""
import ctypes
import os

import numpy as np
import pytest

from a2c_ref import a2c_loss_and_grads
from oracle import ppo_oracle as po

REFERENCE_AC = dict(nsteps=5, lam=0.95, gamma=0.995, log_interval=1000, save_interval=3000, ent_coef=0.0, lr=3e-4,
                    value_network="copy", anneal_bound=1000, num_hidden=64, activation="relu")     # reference defaults.py:49-62


def test_default_params_ac_match_reference():
    from robosumo_selfplay_amd import defaults
    assert defaults.get_default_params("RoboSumo-Ant-vs-Ant-v0", "ac") == REFERENCE_AC
    assert defaults.get_default_params("RoboSumo-Ant-vs-Ant-v0", "ppo")["nsteps"] == 8192


def test_default_params_td3_not_ported():
    from robosumo_selfplay_amd import defaults
    with pytest.raises(NotImplementedError, match="td3"):
        defaults.get_default_params("RoboSumo-Ant-vs-Ant-v0", "td3")


class _FakeEnv(object):
    agents = (0, 1)

    def close(self):
        self.closed = True


def _run_main(monkeypatch, tmp_path, argv):
    import run
    from robosumo_selfplay_amd import alg_ac, alg_ppo, vec_env
    calls = []
    monkeypatch.setattr(vec_env, "make_vec_env", lambda *a, **k: _FakeEnv())
    monkeypatch.setattr(alg_ac, "learn", lambda **kw: calls.append(("ac", kw)) or "ac-model")
    monkeypatch.setattr(alg_ppo, "learn", lambda **kw: calls.append(("ppo", kw)) or "ppo-model")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    out = run.main(argv + ["--log_path", str(tmp_path)])
    return out, calls


def test_run_routes_algo_ac(monkeypatch, tmp_path):
    out, calls = _run_main(monkeypatch, tmp_path, ["--algo", "ac", "--num_env", "8", "--num_timesteps", "80", "--save_interval=7"])
    assert out == "ac-model" and len(calls) == 1 and calls[0][0] == "ac"
    kw = calls[0][1]
    assert kw["nsteps"] == 5 and kw["lam"] == 0.95 and kw["save_interval"] == 7 and kw["nagent"] == 2 and kw["comm"] is None
    out, calls = _run_main(monkeypatch, tmp_path, ["--num_env", "8", "--num_timesteps", "80"])
    assert out == "ppo-model" and calls[0][0] == "ppo"


def test_run_algo_ac_refuses_several_ranks(monkeypatch, tmp_path):
    import run
    from robosumo_selfplay_amd import dist as sdist, vec_env
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(sdist, "init_process_group", lambda *a, **k: pytest.fail("process group started"))
    monkeypatch.setattr(vec_env, "make_vec_env", lambda *a, **k: pytest.fail("env built"))
    with pytest.raises(SystemExit, match="single GPU"):
        run.main(["--algo", "ac", "--log_path", str(tmp_path)])


def test_library_exports_a2c_entries():
    from robosumo_selfplay_amd import build, ppo_capi
    build.build_all()
    L = ctypes.CDLL(build.lib_path("libsumo_ppo.so"))
    for n in ("ppo_a2c_grad", "ppo_a2c_loss_stats"):
        assert hasattr(L, n) and n in ppo_capi.EXPORTS


def test_a2c_restatement_gradient_matches_finite_differences():
    """Central differences on a tiny net (ob 5, ac 2, 7 rows, non-unit IS weights, ent_coef > 0): every parameter entry."""
    rng = np.random.RandomState(0)
    ob, ac, n = 5, 2, 7
    params = [p.astype(np.float64) + rng.normal(0, 0.1, p.shape) for p in po.init_params(rng, ob, ac, hidden=64)]
    obs = rng.normal(0, 1, (n, ob))
    act = rng.normal(0, 1, (n, ac))
    ret, val = rng.normal(0, 2, n), rng.normal(0, 2, n)
    adv = po.normalize_advantages(ret, val)
    w = rng.uniform(0.3, 2.5, n)
    ent_coef, vf_coef = 0.01, 0.5
    loss, stats, sums, grads = a2c_loss_and_grads(params, obs, act, adv, ret, w, ent_coef, vf_coef)
    assert stats[0] * n == pytest.approx(sums[0]) and stats[1] * n == pytest.approx(sums[1]) and sums[2] == pytest.approx(w.sum())
    f = lambda ps: a2c_loss_and_grads(ps, obs, act, adv, ret, w, ent_coef, vf_coef)[0]
    eps = 1e-6
    for k, p in enumerate(params):
        g = np.asarray(grads[k]).reshape(p.shape)
        fd = np.zeros_like(p)
        for j in range(p.size):
            hi = [q.copy() for q in params]; hi[k].flat[j] += eps
            lo = [q.copy() for q in params]; lo[k].flat[j] -= eps
            fd.flat[j] = (f(hi) - f(lo)) / (2 * eps)
        assert np.allclose(g, fd, rtol=1e-5, atol=1e-8), (po.PARAM_NAMES[k], np.abs(g - fd).max())


def test_a2c_value_gradient_is_weighted():
    """Where A2C differs from the PPO loss: doubling every IS weight doubles the value-net gradient."""
    rng = np.random.RandomState(1)
    params = po.init_params(rng, 6, 2)
    obs, act = rng.normal(0, 1, (9, 6)), rng.normal(0, 1, (9, 2))
    ret, val = rng.normal(0, 2, 9), rng.normal(0, 2, 9)
    adv, w = po.normalize_advantages(ret, val), rng.uniform(0.5, 2.0, 9)
    g1 = a2c_loss_and_grads(params, obs, act, adv, ret, w, 0.0, 0.5)[3]
    g2 = a2c_loss_and_grads(params, obs, act, adv, ret, 2 * w, 0.0, 0.5)[3]
    for k in (4, 5, 6, 7, 11, 12):
        assert np.allclose(np.asarray(g2[k]), 2 * np.asarray(g1[k]))


@pytest.mark.parametrize("kw,match", [(dict(use_opponent_data="off_policy"), "off_policy"), (dict(use_opponent_data="both"), "both"),
                                      (dict(network="lstm"), "lstm"), (dict(comm=object()), "single GPU")])
def test_learn_refuses_unsupported_configurations(kw, match):
    from robosumo_selfplay_amd import alg_ac
    args = dict(network="mlp", env=None, total_timesteps=10)
    args.update(kw)
    with pytest.raises(NotImplementedError, match=match):
        alg_ac.learn(**args)
