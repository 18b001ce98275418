"""The tree-sparse linear solve of the HIP engine (``tree_rows`` + ``tree_factor_solve`` of csrc/sumo_engine.hip: qacc_smooth and the
Newton step of every forward whose contacts touch one moving body each) on all nine match-ups: nv from 28 to 44, unequal agents in six
of the nine (the Schur complement of a root block takes its agent's base and leg count per entry), Spider-vs-Spider on the
512-register variant.  Four envs per scene (reset seeds 5 .. 8), ctrl ~ U(-1.5, 1.5), three families of states:

    lifted   the reset pose with both roots raised 1 m: no contact; the reset pose leaves limit rows active in eight scenes,
             Spider-vs-Spider has no row at all
    limits   lifted, every limited hinge 0.05 rad past its lower (even joint id) or upper (odd joint id) limit, qvel ~ N(0, 1)
    floor    60 oracle steps of 0.3 N(0, 1) actions from reset

Oracle sensitivity (CPU, oracle alone, one forward, qpos perturbed by 1e-13 relative; ``oracle_sensitivity`` of
test_gpu_contact_edges), maximum over the nine scenes, and the row counts of the oracle:

    lifted   <= 1.6e-14   ncon 0             nefc 0 to 12
    limits   <= 1.3e-12   ncon 0             nefc 16 to 32, all equal within a scene
    floor    <= 4.8e-12   ncon 0 to 6 / env  nefc 0 to 33 / env

No env exceeds test_gpu_contact_edges' bound of 1e-11, so none is left out of a comparison; every test asserts that first.  (The
floor family sits closest to the bound: of the action seeds 0 .. 3, seeds 0 and 1 each put one env of one scene at 2e-11; the file
uses seed 2.)
"""
import numpy as np
import pytest

from conftest import has_gpu
from robosumo_selfplay_amd import mjcf

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch
    from robosumo_selfplay_amd import capi
    from test_gpu_env_parity import Pair, relerr
    from test_gpu_contact_edges import oracle_sensitivity

ALL = ["RoboSumo-%s-vs-%s-v0" % (a, b) for a in ("Ant", "Bug", "Spider") for b in ("Ant", "Bug", "Spider")]
FAMILIES = ("lifted", "limits", "floor")
N, SEED0 = 4, 5
REL = 1e-9              # the tolerance of test_forward_dynamics_parity
SENS_MAX = 1e-11        # test_gpu_contact_edges' bound on the oracle's own sensitivity
STEP_TOL = {"RoboSumo-Ant-vs-Ant-v0": 1e-9}       # 1e-6 for scenes with a Spider or a Bug: test_step_parity_from_placed_states' tolerances
HINGE = 3


# ---------------------------------------------------------------------------------------------------------------------------------
# states (oracle side: runs without a GPU)
# ---------------------------------------------------------------------------------------------------------------------------------
def family_state(m, ora, family):
    """(qpos, qvel, warm, counters) [N, .] of one family, from an oracle of N envs; leaves the oracle in that state"""
    ora.reset(seeds=np.arange(N, dtype=np.uint64) + SEED0)
    if family == "floor":
        rng = np.random.default_rng(2)
        for _ in range(60):
            ora.step((0.3 * rng.standard_normal((N, 2, ora.act_stride))).astype(np.float32), nthreads=4)
        return ora.get_state()
    q, v, w, c = ora.get_state()
    for a in range(2):
        q[:, int(m.agent_qposadr[a]) + 2] += 1.0
    if family == "limits":
        for j in range(m.njnt):
            if int(m.jnt_type[j]) == HINGE and int(m.jnt_limited[j]):
                lo, hi = float(m.jnt_range[j][0]), float(m.jnt_range[j][1])
                q[:, int(m.jnt_qposadr[j])] = hi + 0.05 if j % 2 else lo - 0.05
        v = np.random.default_rng(61).standard_normal(v.shape)
    ora.set_state(q, v, w, c)
    return q, v, w, c


def oracle_forward(ora, q, v, ctrl):
    """One forward of every env from (q, v), zero warm start: qacc [N, nv], counts [N, 3] = {ncon, nefc, dropped by this forward}"""
    ora.set_state(q, v, np.zeros_like(v), np.zeros((len(q), 2), np.int32))
    qacc, counts = np.zeros((len(q), ora.nv)), np.zeros((len(q), 3), np.int64)
    for e in range(len(q)):
        d0 = ora.array("counts", e)[2]
        ora.forward(e, ctrl[e])
        qacc[e] = ora.array("qacc", e)
        oc = ora.array("counts", e)
        counts[e] = (oc[0], oc[1], oc[2] - d0)
    return qacc, counts


def _ctrl(nu, seed):
    return np.random.default_rng(seed).uniform(-1.5, 1.5, (N, nu))


def _insensitive(ora, q, v, ctrl, seed):
    sens = oracle_sensitivity(ora, q, v, ctrl, np.random.default_rng(seed))
    print("oracle sensitivity: max %.2e" % sens.max())
    assert (sens <= SENS_MAX).all(), sens


# ---------------------------------------------------------------------------------------------------------------------------------
# engine against oracle, and against its own general factorisation
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("env_id", ALL)
def test_forward_against_oracle_and_general_factorisation(monkeypatch, env_id, family):
    """One mj_forward from the family's states: ncon, nefc and dropped equal the oracle's, qacc within REL of it; and within REL of
    the qacc of a second engine created with SUMO_NO_TREE=1, which solves the same systems with the general factorisation."""
    p = Pair(env_id, N, seed0=SEED0)
    q, v, _, _ = family_state(p.m, p.ora, family)
    ctrl = _ctrl(p.eng.nu, 1)
    _insensitive(p.ora, q, v, ctrl, 2)
    oq, oc = oracle_forward(p.ora, q, v, ctrl)
    z, cz = np.zeros_like(v), np.zeros((N, 2), np.int32)
    p.eng.set_state(q, v, z, cz)
    qacc, counts = p.eng.debug_forward(ctrl)
    monkeypatch.setenv("SUMO_NO_TREE", "1")
    gen = capi.Engine(p.m, N)
    monkeypatch.delenv("SUMO_NO_TREE")
    gen.set_state(q, v, z, cz)
    gq, gcounts = gen.debug_forward(ctrl)
    gen.close()
    print("%s %s: ncon %s nefc %s newton %s; qacc relerr oracle %.2e, general %.2e" % (
        env_id, family, counts[:, 0], counts[:, 1], counts[:, 2], max(relerr(qacc[e], oq[e]) for e in range(N)),
        max(relerr(qacc[e], gq[e]) for e in range(N))))
    for e in range(N):
        assert (counts[e, 0], counts[e, 1], counts[e, 3]) == tuple(oc[e]), (e, counts[e], oc[e])
        assert (gcounts[e, 0], gcounts[e, 1], gcounts[e, 3]) == tuple(oc[e]), (e, gcounts[e], oc[e])
        assert relerr(qacc[e], oq[e]) < REL, (e, relerr(qacc[e], oq[e]))
        assert relerr(qacc[e], gq[e]) < REL, (e, relerr(qacc[e], gq[e]))
    if family != "floor":
        assert (counts[:, 0] == 0).all()
    if family == "limits":
        assert (counts[:, 1] >= 16).all() and (counts[:, 1] == counts[0, 1]).all()


@pytest.mark.parametrize("env_id", ALL)
def test_env_step_from_floor_states(env_id):
    """One full env step (20 forwards with warm starts and Newton loops) from the floor states against the oracle, compared the way
    test_step_parity_from_placed_states compares."""
    tol = STEP_TOL.get(env_id, 1e-6)
    p = Pair(env_id, N, seed0=SEED0)
    q, v, w, c = family_state(p.m, p.ora, "floor")
    _insensitive(p.ora, q, v, _ctrl(p.eng.nu, 1), 2)
    p.ora.set_state(q, v, w, c)
    p.eng.set_state(q, v, w, c)
    dropped0 = p.ora.stats()["dropped"]
    a = np.random.default_rng(7).standard_normal((N, 2, p.eng.act_stride)).astype(np.float32)
    (gobs, ginfo, gdone, gr, gdr, gl), (oobs, oinfo, odone, orr, odr, ol) = p.step(a)
    gs, os_ = p.eng.get_state(), p.ora.get_state()
    print("%s: obs %.2e, info %.2e, qpos %.2e, qvel %.2e, warm %.2e" % (env_id, np.abs(gobs - oobs).max(), relerr(ginfo, oinfo),
                                                                       relerr(gs[0], os_[0]), relerr(gs[1], os_[1]), relerr(gs[2], os_[2])))
    assert np.array_equal(gdone, odone) and np.array_equal(ginfo[:, :, 7], oinfo[:, :, 7]) and np.array_equal(gl, ol)
    if tol <= 1e-9:
        assert np.array_equal(gobs, oobs), np.abs(gobs - oobs).max()
    else:
        assert np.abs(gobs - oobs).max() < 1e-5
    assert relerr(ginfo, oinfo) < tol and relerr(gr, orr) < tol and relerr(gdr, odr) < tol
    assert relerr(gs[0], os_[0]) < tol and relerr(gs[1], os_[1]) < tol and relerr(gs[2], os_[2]) < 1e3 * tol
    assert np.array_equal(gs[3], os_[3])
    assert p.eng.stats()["dropped"] == p.ora.stats()["dropped"] - dropped0      # (the oracle's counters include its 60 steps to the floor)


SAME = [e for e in ALL if e.split("-")[1] == e.split("-")[3]]


@pytest.mark.parametrize("env_id", SAME)
def test_fused_equals_stepwise_from_floor_states(env_id):
    """Two rollout steps from the floor states through the fused launch and through the per-step launches: every returned array and
    the engine state bitwise equal.  The three scenes of equal agents (nv 28, 36, 44): the fused launches evaluate both policies
    inside the engine and refuse a scene whose agents differ in their observation and action widths (runner.py, zoo_pairs.py), so
    the six mixed scenes have no fused launch to compare; they run the same step kernel's solver in the two tests above."""
    from robosumo_selfplay_amd import policies
    from robosumo_selfplay_amd.model import PPOModel
    from robosumo_selfplay_amd.runner import Runner
    from robosumo_selfplay_amd.vec_env import SumoVecEnv
    from oracle.oracle import OracleSim
    m = mjcf.load_model(env_id)
    T = 2
    outs = []
    for fused in (True, False):
        env = SumoVecEnv(env_id, num_envs=N, seed=SEED0, model=m)
        spec = policies.PolicySpec(env.observation_space[0].shape[0], env.action_space[0].shape[0], value_network="copy", activation="relu")
        np.random.seed(3)
        models = [PPOModel(policy=spec, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, trainable=False) for _ in range(2)]
        rng = np.random.RandomState(1)
        for m_ in models:
            m_.set_param_list([x + rng.normal(0, 0.1, x.shape).astype(np.float32) for x in m_.get_param_list()])
        models[0].act_model.seed(7); models[1].act_model.seed(8)
        r = Runner(env=env, models=models, nsteps=T, nagent=2, gamma=0.995, lam=0.95, rho_bar=1.0, c_bar=1.0, anneal_bound=500)
        r.fused_rollout = fused
        assert r.fused_ok() == fused
        E = env.engines[0]
        if not outs:
            ora = OracleSim(m, N, maxcon=E.maxcon, jbcap=E.jbcap)
            state = family_state(m, ora, "floor")
        E.set_state(*state)
        out = r.run(250)
        torch.cuda.synchronize()
        arrays = [x.cpu().numpy() for x in out if torch.is_tensor(x)] + [env.obs_dev.cpu().numpy(), env.done_dev.cpu().numpy()]
        arrays += list(E.get_state())
        outs.append(arrays)
        st = env.stats()
        assert st["rollout_aborts"] == 0 and st["diverged"] == 0
        env.close()
    assert len(outs[0]) == len(outs[1]) and len(outs[0]) >= 10
    for k, (a, b) in enumerate(zip(*outs)):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), k
