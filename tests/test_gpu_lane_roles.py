"""The lane role words (csrc/sumo_engine.hip: Ctx::role0 / role1) on the kernel variants no static layout covers, at the smallest
shapes where a wrong role shows: 8 envs, 3 env steps (60 forward evaluations) from reset.

Mixed scenes (two different trees in one env, dynamic layout): the per-step kernel against oracle.OracleSim with fixed seeded
actions and the bounds of tests/test_gpu_env_parity.py.  The fused rollout launch takes homogeneous match-ups only (sumo_rollout_steps
refuses the others), so on Ant-vs-Bug and Bug-vs-Spider the per-step kernel is the only one there is; the fused launch's dynamic-layout
variant is held against the per-step kernel, bit for bit, on Bug-vs-Bug (nv 36), where it runs, and that scene goes through the same
oracle comparison.  Wrestling: Ant-vs-Ant with the agents placed leg to leg (the placement of test_step_parity_when_agents_wrestle),
which takes the dense Newton path: oracle parity of the per-step kernel and fused == per-step from the placed state."""
import numpy as np
import pytest

from conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch
    from robosumo_selfplay_amd.runner import Runner
    from robosumo_selfplay_amd.vec_env import SumoVecEnv
    from test_gpu_env_parity import Pair, relerr
    from test_gpu_ppo import _model, _perturb

N, STEPS = 8, 3
NAMES = ["obs", "returns", "masks", "actions", "values", "neglogpacs", "rewards", "opp_neglogpacs", "opp_obs", "opp_actions", "states",
         "epinfos", "off_policy_ratio", "off_env_ratio", "total_ratio"]


def _wrestle(m, q, v, seed=5):
    """Torsos 0.55 .. 0.95 apart so that the legs overlap (test_step_parity_when_agents_wrestle's placement)."""
    a0, a1 = int(m.agent_qposadr[0]), int(m.agent_qposadr[1])
    rng = np.random.default_rng(seed)
    for e in range(q.shape[0]):
        ang = rng.uniform(0, 2 * np.pi)
        d = rng.uniform(0.55, 0.95)
        ctr = rng.uniform(-0.3, 0.3, 2)
        q[e, a0:a0 + 2] = ctr + 0.5 * d * np.array([np.cos(ang), np.sin(ang)])
        q[e, a1:a1 + 2] = ctr - 0.5 * d * np.array([np.cos(ang), np.sin(ang)])
    v[:] *= 0.5
    return rng


# test_step_parity_with_resync's bound for every scene with a Bug or a Spider in it (Ant-vs-Ant alone holds 1e-9)
@pytest.mark.parametrize("env_id,tol", [("RoboSumo-Ant-vs-Bug-v0", 1e-6), ("RoboSumo-Bug-vs-Spider-v0", 1e-6), ("RoboSumo-Bug-vs-Bug-v0", 1e-6)])
def test_step_kernel_matches_oracle_from_reset(env_id, tol):
    p = Pair(env_id, N)
    g, o = p.reset()
    assert np.array_equal(g, o)
    rng = np.random.default_rng(1)
    for t in range(STEPS):
        a = (rng.standard_normal((N, 2, p.eng.act_stride)) * (1.0 if t % 3 else 2.5)).astype(np.float32)
        (gobs, ginfo, gdone, gr, gdr, gl), (oobs, oinfo, odone, orr, odr, ol) = p.step(a)
        assert np.array_equal(gdone, odone) and np.array_equal(gl, ol)
        assert np.abs(gobs - oobs).max() < 1e-5
        assert relerr(ginfo, oinfo) < tol and relerr(gr, orr) < tol and relerr(gdr, odr) < tol
        gs, os_ = p.eng.get_state(), p.ora.get_state()
        assert relerr(gs[0], os_[0]) < tol and relerr(gs[1], os_[1]) < tol and relerr(gs[2], os_[2]) < 1e3 * tol
        assert np.array_equal(gs[3], os_[3])
        p.eng.set_state(*os_)
    gst, ost = p.eng.stats(), p.ora.stats()
    assert gst["dropped"] == 0 and ost["dropped"] == 0 and gst["diverged"] == 0
    assert gst["max_ncon"] == ost["max_ncon"] > 0


def _rollouts(env_id, fused, place=False):
    env = SumoVecEnv(env_id, num_envs=N, seed=11)
    assert not place or env.engine.static_layout()
    D, A = env.observation_space[0].shape[0], env.action_space[0].shape[0]
    learner, opp = _model(D, A, seed=3, trainable=False), _model(D, A, seed=4, trainable=False)
    _perturb(learner, np.random.RandomState(3)); _perturb(opp, np.random.RandomState(4))
    learner.act_model.seed(101); opp.act_model.seed(202)
    r = Runner(env=env, models=[learner, opp], nsteps=STEPS, nagent=2, gamma=0.995, lam=0.95, rho_bar=1.0, c_bar=1.0, anneal_bound=500)
    r.fused_rollout = fused
    if place:
        q, v, w, c = env.engine.get_state()
        _wrestle(env.model, q, v)
        env.engine.set_state(q, v, w, c)
    out = r.run(250)
    torch.cuda.synchronize()
    st, stats = env.engine.get_state(), env.stats()
    env.close()
    return out, st, stats


@pytest.mark.parametrize("env_id,place", [("RoboSumo-Bug-vs-Bug-v0", False), ("RoboSumo-Ant-vs-Ant-v0", True)], ids=["bug-dynamic", "ant-wrestling"])
def test_fused_launch_equals_step_kernel(env_id, place):
    (fo, fs, fstat), (so, ss, sstat) = _rollouts(env_id, True, place), _rollouts(env_id, False, place)
    for k, (x, y) in enumerate(zip(fo, so)):
        if torch.is_tensor(x):
            assert torch.equal(x, y), NAMES[k]
        else:
            assert x == y, NAMES[k]
    for x, y in zip(fs, ss):
        assert np.array_equal(x, y)
    for k in ("forward", "newton", "contacts", "efc", "dropped", "diverged"):
        assert fstat[k] == sstat[k], k
    assert fstat["forward"] >= 20 * N * STEPS and fstat["diverged"] == 0 and np.isfinite(fs[0]).all() and np.isfinite(fs[1]).all()


def test_step_kernel_matches_oracle_when_agents_wrestle():
    """test_step_parity_when_agents_wrestle at 8 envs x 3 steps, with its bounds (Ant-vs-Ant: 1e-8 on qpos, 1e-6 on qvel, 2e-5 on the
    float32 observations)."""
    tol = 1e-8
    p = Pair("RoboSumo-Ant-vs-Ant-v0", N)
    p.reset()
    q, v, w, c = p.ora.get_state()
    rng = _wrestle(p.m, q, v)
    p.ora.set_state(q, v, w, c)
    p.eng.set_state(q, v, w, c)
    gb = p.m.tables["geom_bodyid"]
    two_body = 0
    for t in range(STEPS):
        a = (rng.standard_normal((N, 2, p.eng.act_stride)) * 0.7).astype(np.float32)
        (gobs, ginfo, gdone, gr, gdr, gl), (oobs, oinfo, odone, orr, odr, ol) = p.step(a)
        assert np.array_equal(gdone, odone) and np.array_equal(gl, ol)
        assert np.abs(gobs - oobs).max() < 2e-5
        gs, os_ = p.eng.get_state(), p.ora.get_state()
        assert relerr(gs[0], os_[0]) < tol and relerr(gs[1], os_[1]) < 1e2 * tol, (t, relerr(gs[0], os_[0]), relerr(gs[1], os_[1]))
        for e in range(N):
            p.ora.forward(e)
            con = p.ora.array("contacts", e).reshape(-1, 9)
            two_body += int(any(gb[int(cc[7])] != 0 and gb[int(cc[8])] != 0 for cc in con))
        p.eng.set_state(*os_)
    gst, ost = p.eng.stats(), p.ora.stats()
    assert gst["dropped"] == ost["dropped"] and gst["max_ncon"] == ost["max_ncon"]
    assert two_body >= 1, two_body          # contacts between two moving bodies did occur: the dense path ran
