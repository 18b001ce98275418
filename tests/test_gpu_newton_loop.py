"""The Newton loop of the HIP engine (``newton_solve`` of csrc/sumo_engine.hip: warm start, gradient and its threshold test, tree
solve, line search, improvement test) with the loop cut at every early exit, against the CPU oracle.  What it covers of the engine:
the gradient test as ``gn <= grad_thresh`` (the threshold sumo_create bisects from the scene's own options, so also at the changed
tolerances), the tree-path contact forms (``24 * ci`` addressing in the gradient and ``tree_rows``, the 8-slot ``contact_Jx`` /
``contact_Jx3``) against the general forms, and the iteration count.  The loop's order of work is the one it had before: rotating
it was tried and dropped.

Scenes: Ant-vs-Ant (static flagship layout), Ant-vs-Bug (nv 32, dynamic layout, unequal agents), Spider-vs-Spider (512-register
variant, three contact rows per lane).  Four envs, reset seeds 5 .. 8, the three state families of test_gpu_tree_schur (lifted, limits,
floor), models that are copies of the scene tables with ``opt`` changed: iterations in {1, 2, 3, shipped} at the shipped tolerance,
tolerance in {1e-4, 1e-1} at the shipped iterations.  Per case the oracle-sensitivity bound of test_gpu_contact_edges is asserted
first (no env is left out), then ncon / nefc / dropped equal the oracle's, qacc within REL of it, the Newton count at most
``iterations``; floor states also against an engine created with SUMO_NO_TREE=1 (the general factorisation and contact forms).

That the ``iterations`` cases can see an off-by-one iteration is checked on the CPU by test_iteration_cases_discriminate: the oracle's
qacc at iterations 1, 2 and the shipped value must differ pairwise by more than 1e-6 relative on ``limits`` and ``floor``.  With the
ctrl seed of test_gpu_tree_schur (1) the oracle is converged after two iterations on Ant-vs-Ant (both families) and on Ant-vs-Bug
``limits``, so the seeds here are chosen by the oracle alone: ctrl seed 3 for ``limits`` (2 vs shipped: 7.3e-2 Ant, 1.7e-2 Ant-vs-Bug,
1.3e-1 Spider) and ctrl seed 2 for ``floor`` (3.8e-2, 7.1e-1, 4.1e-2); 1 vs 2 is above 0.3 everywhere.  Oracle sensitivity with these
seeds: at most 1.4e-12 on ``limits`` and 8.0e-12 on ``floor`` (Ant-vs-Ant), under the bound of 1e-11.

Contacts of the floor states (oracle): Ant-vs-Bug env 1 has five contacts, three on the bodies of agent 0 and two on agent 1 -- its
root dofs lie under three and two contacts, so the tree-path gradient's loop over a dof's contact mask runs more than once
(test_floor_contacts_cover_shared_dofs asserts >= 4 contacts in an env and a dof under >= 2).  The gradient takes its contacts one
after the other: requesting three at once changed result bits and was dropped."""
import copy

import numpy as np
import pytest

from robosumo_selfplay_amd import mjcf

ANT, ANT_BUG, SPIDER = "RoboSumo-Ant-vs-Ant-v0", "RoboSumo-Ant-vs-Bug-v0", "RoboSumo-Spider-vs-Spider-v0"
SCENES = (ANT, ANT_BUG, SPIDER)
FAMILIES = ("lifted", "limits", "floor")
CTRL_SEED = {"lifted": 1, "limits": 3, "floor": 2}
REL = 1e-9
SENS_MAX = 1e-11
OPT_TOLERANCE, OPT_ITERATIONS = 4, 7
N = 4
ITERATIONS = (1, 2, 3, None)       # None: the shipped value
TOLERANCES = (1e-4, 1e-1)
OPTS = [("iterations", it) for it in ITERATIONS] + [("tolerance", t) for t in TOLERANCES]


def changed_model(m, what, value):
    """a copy of the scene's tables with one solver option replaced (value None: the shipped model)"""
    m2 = copy.copy(m)
    m2.tables = {k: np.array(t) for k, t in m.tables.items()}
    if value is not None:
        m2.tables["opt"][OPT_ITERATIONS if what == "iterations" else OPT_TOLERANCE] = value
    return m2


def relerr(a, b):
    return np.abs(a - b).max() / (1.0 + np.abs(b).max())


_STATES = {}


def family_case(env_id, family):
    """(model, q, v, ctrl) of one scene and family, computed once with the oracle (CPU)"""
    import test_gpu_tree_schur as ts
    from oracle.oracle import OracleSim
    assert ts.N == N and ts.SEED0 == 5
    key = (env_id, family)
    if key not in _STATES:
        m = mjcf.load_model(env_id)
        ora = OracleSim(m, N)
        q, v, _, _ = ts.family_state(m, ora, family)
        _STATES[key] = (m, q, v, ts._ctrl(ora.nu, CTRL_SEED[family]))
    return _STATES[key]


def oracle_qacc(m, q, v, ctrl, what, value, maxcon=None, jbcap=None):
    import test_gpu_tree_schur as ts
    from oracle.oracle import OracleSim
    ora = OracleSim(changed_model(m, what, value), N, maxcon=maxcon, jbcap=jbcap)
    return ora, ts.oracle_forward(ora, q, v, ctrl)


@pytest.mark.parametrize("family", ("limits", "floor"))
@pytest.mark.parametrize("env_id", SCENES)
def test_iteration_cases_discriminate(oracle_lib, env_id, family):
    """CPU: the oracle's qacc at iterations 1, 2 and the shipped value differ pairwise by more than 1e-6 relative in some env."""
    m, q, v, ctrl = family_case(env_id, family)
    res = {it: oracle_qacc(m, q, v, ctrl, "iterations", it)[1][0] for it in (1, 2, None)}
    d = lambda a, b: max(relerr(res[a][e], res[b][e]) for e in range(N))
    print("%s %s: 1 vs 2 %.1e, 2 vs shipped %.1e, 1 vs shipped %.1e" % (env_id, family, d(1, 2), d(2, None), d(1, None)))
    assert d(1, 2) > 1e-6 and d(2, None) > 1e-6 and d(1, None) > 1e-6


def test_floor_contacts_cover_shared_dofs(oracle_lib):
    """CPU: the Ant-vs-Bug floor states hold an env with four or more contacts and a dof under two or more contacts (two contacts on
    bodies of one agent share its six root dofs)."""
    import test_gpu_tree_schur as ts
    m, q, v, ctrl = family_case(ANT_BUG, "floor")
    ora, (_, counts) = oracle_qacc(m, q, v, ctrl, "iterations", None)
    gb, b1 = np.asarray(m.geom_bodyid), int(m.agent_bodyadr[1])
    most, shared = 0, 0
    for e in range(N):
        ora.set_state(q, v, np.zeros_like(v), np.zeros((N, 2), np.int32))
        ora.forward(e, ctrl[e])
        con = ora.array("contacts", e).reshape(-1, 9)
        agents = [int(max(gb[int(c[7])], gb[int(c[8])]) >= b1) for c in con]
        most = max(most, len(con))
        shared = max([shared] + [agents.count(a) for a in (0, 1)])
    assert most >= 4 and shared >= 2, (most, shared)


@pytest.mark.gpu
@pytest.mark.parametrize("what,value", OPTS)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("env_id", SCENES)
def test_forward_at_every_early_exit(monkeypatch, env_id, family, what, value):
    from robosumo_selfplay_amd import capi
    from test_gpu_contact_edges import oracle_sensitivity
    m, q, v, ctrl = family_case(env_id, family)
    m2 = changed_model(m, what, value)
    eng = capi.Engine(m2, N)
    ora, (oq, oc) = oracle_qacc(m, q, v, ctrl, what, value, maxcon=eng.maxcon, jbcap=eng.jbcap)
    sens = oracle_sensitivity(ora, q, v, ctrl, np.random.default_rng(2))
    print("oracle sensitivity: max %.2e" % sens.max())
    assert (sens <= SENS_MAX).all(), sens
    z, cz = np.zeros_like(v), np.zeros((N, 2), np.int32)
    eng.set_state(q, v, z, cz)
    qacc, counts = eng.debug_forward(ctrl)
    eng.close()
    maxiter = int(m2.opt[OPT_ITERATIONS])
    err = max(relerr(qacc[e], oq[e]) for e in range(N))
    print("%s %s %s=%s: ncon %s nefc %s newton %s; qacc relerr oracle %.2e" % (env_id, family, what, value, counts[:, 0], counts[:, 1], counts[:, 2], err))
    for e in range(N):
        assert (counts[e, 0], counts[e, 1], counts[e, 3]) == tuple(oc[e]), (e, counts[e], oc[e])
        assert relerr(qacc[e], oq[e]) < REL, (e, relerr(qacc[e], oq[e]))
        assert 0 <= counts[e, 2] <= maxiter, (e, counts[e, 2], maxiter)
    if family == "floor":
        monkeypatch.setenv("SUMO_NO_TREE", "1")
        gen = capi.Engine(m2, N)
        monkeypatch.delenv("SUMO_NO_TREE")
        gen.set_state(q, v, z, cz)
        gq, gcounts = gen.debug_forward(ctrl)
        gen.close()
        gerr = max(relerr(qacc[e], gq[e]) for e in range(N))
        print("general factorisation: qacc relerr %.2e, newton %s" % (gerr, gcounts[:, 2]))
        for e in range(N):
            assert relerr(qacc[e], gq[e]) < REL, (e, relerr(qacc[e], gq[e]))
            assert gcounts[e, 2] <= maxiter
