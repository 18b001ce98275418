"""The set-up of the constraint solve in the HIP engine (``newton_solve`` of csrc/sumo_engine.hip, from its top to the first
iteration) against the oracle: one pass over the contact Jacobians serves aref of the contact rows and the costs of both starting
points -- qacc_warmstart and qacc_smooth -- of which the cheaper one is kept; ``make_constraint`` evaluates a hinge's limit row once,
for the side that is active.

The other forward tests give both sides a zero warm start, which pins the choice between the two starts only loosely.  Here engine and
oracle get the same NON-ZERO warm start, chosen so that one named start wins, and the oracle's own two costs (recomputed in numpy
from its M, qfrc_smooth, qacc_smooth, efc_J, efc_aref and efc_R) say which start a converged solver takes.  Then the row-count edges of
the pass (no row at all, limit rows only, one contact, 4 ncon on both sides of a wave's 64 lanes, a full contact list, a contact
between two moving bodies), hinges past their lower and upper limits within one env, both sides of one hinge active at once, and the
fused launch against the per-step launches.

Both sides of one hinge: a side is active when the hinge is within its margin of that end of its range.  Every hinge of every
shipped scene has margin 0 (the 0.01 in jnt_margin belongs to the free joints), so a side is active only past its limit and no
shipped model can have both at once.  test_both_sides_of_one_hinge therefore runs a model copy (the tables of Ant-vs-Ant, changed in
memory) in which two hinges get a margin of 0.01 and a range 0.01 wide: that is the only run of the second evaluation.

Half of the placed envs of test_both_starts_win keep the reset's hinge angles (many past a limit: limit rows in both costs), the
other half get angles inside their ranges; with the former alone the limit rows make qacc_smooth so expensive on Ant that the
perturbed warm start still wins in all but 13 of 96 envs.

Oracle sensitivity (CPU, oracle alone, one forward, qpos perturbed by 1e-13 relative with the warm start held; relerr of qacc as in
test_gpu_env_parity), maximum over the envs of each case and how many envs exceed 1e-11 (left out of the qacc comparison, never
out of the count comparisons; at most 5 % of a case's envs may be), and how many envs take the named start by the oracle's costs:

    Ant-vs-Ant        converged qacc  2.4e-12 (0), 93 of 93 with rows    + 1e3 U(-1, 1)  6.2e-12 (0), 43 of 93
    Spider-vs-Spider  converged qacc  4.7e-12 (0), 92 of 92              + 1e3 U(-1, 1)  1.4e-11 (1), 80 of 92
    row-count edges (Ant)  1.0e-11 (1)      limits (Ant)  3.3e-12 (0)      both sides (Ant copy)  1.2e-12 (0)
"""
import copy

import numpy as np
import pytest

import contact_ref as cr
from conftest import has_gpu
from robosumo_selfplay_amd import mjcf

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch
    from robosumo_selfplay_amd import capi
    from oracle.oracle import OracleSim
    from test_gpu_env_parity import Pair, relerr
else:
    def relerr(a, b):
        return np.abs(a - b).max() / (1.0 + np.abs(b).max())

ANT, SPIDER = "RoboSumo-Ant-vs-Ant-v0", "RoboSumo-Spider-vs-Spider-v0"
REL = 1e-9              # test_gpu_contact_edges' tolerance, and its exclusion rule:
SENS_MAX = 1e-11        # envs whose oracle sensitivity exceeds this are left out of the qacc comparison ...
SENS_SHARE = 0.05       # ... at most this share of a case's envs
HINGE = 3


# ---------------------------------------------------------------------------------------------------------------------------------
# oracle side (runs without a GPU)
# ---------------------------------------------------------------------------------------------------------------------------------
def oracle_forward(ora, q, v, w, ctrl):
    """One forward of every env from (q, v) with warm start w.  Returns qacc [N, nv] and counts [N, 3] = {ncon, nefc, dropped by this forward}."""
    N = len(q)
    ora.set_state(q, v, w, np.zeros((N, 2), np.int32))
    qacc, counts = np.zeros((N, ora.nv)), np.zeros((N, 3), np.int64)
    for e in range(N):
        d0 = ora.array("counts", e)[2]
        ora.forward(e, ctrl[e])
        qacc[e] = ora.array("qacc", e)
        oc = ora.array("counts", e)
        counts[e] = (oc[0], oc[1], oc[2] - d0)
    return qacc, counts


def oracle_sensitivity(ora, q, v, w, ctrl, rng):
    """relerr of the oracle's qacc between q and q (1 + 1e-13 u), u ~ U(-1, 1), per env, the warm start held."""
    base, _ = oracle_forward(ora, q, v, w, ctrl)
    pert, _ = oracle_forward(ora, q * (1.0 + 1e-13 * rng.uniform(-1.0, 1.0, q.shape)), v, w, ctrl)
    return np.array([relerr(pert[e], base[e]) for e in range(len(q))])


def start_costs(ora, e, w):
    """(cost at the warm start w, cost at qacc_smooth, nefc) of env e after ``ora.forward(e, ...)``, as the solver's set-up forms them:
    cost(x) = 1/2 (M x - qfrc_smooth).(x - qacc_smooth) + sum over rows with jar < 0 of 1/2 jar^2 / R, jar = J x - aref."""
    nv = ora.nv
    nefc = int(ora.array("counts", e)[1])
    M = ora.array("M", e).reshape(nv, nv)
    qsm, asmo = ora.array("qfrc_smooth", e), ora.array("qacc_smooth", e)
    if nefc == 0:
        return 0.0, 0.0, 0
    J = ora.array("efc_J", e, cap=1 << 18).reshape(nefc, nv)
    aref, D = ora.array("efc_aref", e), 1.0 / ora.array("efc_R", e)

    def rows(x):
        jar = J @ x - aref
        return float((0.5 * D * jar * jar)[jar < 0].sum())
    return float(0.5 * (M @ w - qsm) @ (w - asmo)) + rows(w), rows(asmo), nefc


def two_moving(ora, m, e):
    """contacts of env e (after a forward) between two moving bodies"""
    con = ora.array("contacts", e).reshape(-1, 9)
    gb = np.asarray(m.geom_bodyid)
    return int(sum(gb[int(c[7])] != 0 and gb[int(c[8])] != 0 for c in con))


def hinges(m):
    """(qpos address, dof address, lower, upper) of every limited hinge"""
    out = []
    for j in range(m.njnt):
        if int(m.jnt_type[j]) == HINGE and int(m.jnt_limited[j]):
            out.append((int(m.jnt_qposadr[j]), int(m.jnt_dofadr[j]), float(m.jnt_range[j][0]), float(m.jnt_range[j][1])))
    return out


def lifted(m, q, e, rng=None):
    """env e: both agents clear of everything, every hinge at the middle of its range (no constraint row at all)"""
    for a in range(2):
        q[e, int(m.agent_qposadr[a]):int(m.agent_qposadr[a]) + 3] = [3.0 * a, 0.0, 5.0 + a]
    for qa, _, lo, hi in hinges(m):
        q[e, qa] = 0.5 * (lo + hi)


def placed_states(m, q0, v0, seed=11, in_range=False):
    """16 states of each placement family of contact_ref (96 envs); in_range: every other env gets hinge angles inside their ranges"""
    q, v = cr.place(m, q0, v0, cr.family_list(m, 16), seed)
    if in_range:
        rng = np.random.default_rng(seed + 1000)
        for e in range(1, len(q), 2):
            for qa, _, lo, hi in hinges(m):
                q[e, qa] = rng.uniform(lo, hi)
    return q, v


def past_limits(m, q, v, e, rng, lo_share=0.5):
    """env e: every hinge pushed past a limit, `lo_share` of them the lower one, the rest the upper one; hinge velocities N(0, 1)"""
    hs = hinges(m)
    low = rng.permutation(len(hs)) < lo_share * len(hs)
    for k, (qa, da, lo, hi) in enumerate(hs):
        q[e, qa] = lo - rng.uniform(0.0, 0.05) if low[k] else hi + rng.uniform(0.0, 0.05)
        v[e, da] = rng.standard_normal()
    return low


def edge_pool(m, q0, v0, seed):
    """Candidate states for the row-count edges (Ant): the embedded and piled families let down onto / lifted off the tatami in
    small steps, so that every contact count from none to the full list occurs.  q0 / v0: [n, .] reset states."""
    n = len(q0)
    rng = np.random.default_rng(seed)
    fams = (["embedded"] * 3 + ["piled"]) * (n // 4) + ["embedded"] * (n % 4)
    q, v = cr.place(m, q0, v0, fams, seed)
    a0, a1 = int(m.agent_qposadr[0]), int(m.agent_qposadr[1])
    for e, f in enumerate(fams):
        dz = rng.uniform(0.0, 0.9 if f == "embedded" else 0.4)
        q[e, a0 + 2] += dz
        if f == "piled":
            q[e, a1 + 2] += dz
    return q, v, fams


def edge_states(m, make_ora, q0, v0, ctrl_pool, want=(1, 16, 17), per=6, seed=5):
    """96 Ant states for the row-count edges, picked by the ORACLE's counts from edge_pool: `per` envs of each contact count in `want`
    and of ncon == maxcon, `per` with a contact between two moving bodies, 8 without any row, 8 with limit rows only; the rest placed
    states.  ``make_ora(n)``: an oracle of n envs.  Returns q, v, ctrl, tags (one string per env)."""
    N = 96
    reps = 6
    qp, vp, _ = edge_pool(m, np.tile(q0, (reps, 1)), np.tile(v0, (reps, 1)), seed)
    cp = np.tile(ctrl_pool, (reps, 1))
    pool = make_ora(len(qp))
    _, counts = oracle_forward(pool, qp, vp, np.zeros_like(vp), cp)
    mov = np.array([two_moving(pool, m, e) for e in range(len(qp))])
    maxcon = int(counts[:, 0].max())
    picks, tags = [], []
    for k in list(want) + [maxcon]:
        idx = np.nonzero((counts[:, 0] == k) & (mov == 0) & (counts[:, 2] == 0 if k != maxcon else True))[0][:per]
        picks += idx.tolist()
        tags += ["ncon%d" % k if k != maxcon else "full"] * len(idx)
    idx = np.nonzero((mov > 0) & (counts[:, 2] == 0))[0][:per]
    picks += idx.tolist()
    tags += ["moving"] * len(idx)
    q, v, ctrl = qp[picks], vp[picks], cp[picks]
    rng = np.random.default_rng(seed + 1)
    nfill = N - len(picks)
    qf, vf = placed_states(m, q0, v0)
    q, v, ctrl = np.concatenate([q, qf[:nfill]]), np.concatenate([v, vf[:nfill]]), np.concatenate([ctrl, ctrl_pool[:nfill]])
    tags += ["placed"] * nfill
    e0 = len(picks)
    for e in range(e0, e0 + 16):                      # the first 16 fill-ins become: no row at all / limit rows only
        lifted(m, q, e)
        tags[e] = "clear"
        if e >= e0 + 8:
            hs = hinges(m)
            for k in rng.choice(len(hs), 1 + (e % 4), replace=False):
                qa, da, lo, hi = hs[k]
                q[e, qa] = lo - 0.02 if k % 2 else hi + 0.02
            tags[e] = "limonly"
    return q, v, ctrl, tags


def reset_state(ora, n, seed0=100):
    ora.reset(seeds=np.arange(n, dtype=np.uint64) + seed0)
    q0, v0, _, _ = ora.get_state()
    return q0, v0


def narrowed_model(m):
    """A copy of the model in which two hinges (one per agent) have a margin of 0.01 and a range 0.01 wide around 0.3 / -0.2: near
    its middle both the lower and the upper side lie within the margin."""
    m2 = copy.copy(m)
    m2.tables = {k: np.array(t) for k, t in m.tables.items()}
    hj = [j for j in range(m.njnt) if int(m.jnt_type[j]) == HINGE and int(m.jnt_limited[j])]
    mids = {hj[1]: 0.3, hj[len(hj) // 2 + 2]: -0.2}
    for j, mid in mids.items():
        m2.tables["jnt_range"][j] = [mid - 0.005, mid + 0.005]
        m2.tables["jnt_margin"][j] = 0.01
    return m2, {int(m.jnt_qposadr[j]): mid for j, mid in mids.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# engine against oracle
# ---------------------------------------------------------------------------------------------------------------------------------
def _pair(env_id, N, model=None):
    """Pair of test_gpu_env_parity; with `model`, the same on a model that is no registered scene"""
    if model is None:
        p = Pair(env_id, N)
    else:
        p = Pair.__new__(Pair)
        p.m, p.N = model, N
        p.eng = capi.Engine(model, N)
        p.ora = OracleSim(model, N, maxcon=p.eng.maxcon, jbcap=p.eng.jbcap)
    return p


def _parity(p, q, v, w, ctrl, seed):
    """One mj_forward of both sides from (q, v), warm start w: per env ncon, nefc and dropped equal, qacc to REL outside the envs the
    sensitivity rule leaves out.  Returns the engine's counts [N, 4] = {ncon, nefc, newton, dropped}; the oracle is left after its
    forward of every env."""
    rng = np.random.default_rng(seed)
    sens = oracle_sensitivity(p.ora, q, v, w, ctrl, rng)
    out = sens > SENS_MAX
    print("oracle sensitivity: max %.2e, %d of %d envs above %.0e" % (sens.max(), out.sum(), p.N, SENS_MAX))
    assert out.sum() <= SENS_SHARE * p.N, (sens.max(), out.sum())
    p.eng.set_state(q, v, w, np.zeros((p.N, 2), np.int32))
    qacc, counts = p.eng.debug_forward(ctrl)
    oq, oc = oracle_forward(p.ora, q, v, w, ctrl)
    worst = 0.0
    for e in range(p.N):
        assert (counts[e, 0], counts[e, 1], counts[e, 3]) == tuple(oc[e]), (e, counts[e], oc[e])
        if not out[e]:
            err = relerr(qacc[e], oq[e])
            worst = max(worst, err)
            assert err < REL, (e, err, sens[e])
    print("qacc relerr: max %.2e over %d envs; ncon max %d" % (worst, p.N - out.sum(), counts[:, 0].max()))
    return counts


def warm_starts(ora, q, v, ctrl, kind, seed):
    """The oracle's own converged qacc of each state ('warm': the warm start wins), plus 1e3 U(-1, 1) ('smooth': qacc_smooth wins)"""
    w, _ = oracle_forward(ora, q, v, np.zeros_like(v), ctrl)
    if kind == "smooth":
        w = w + 1e3 * np.random.default_rng(seed).uniform(-1.0, 1.0, w.shape)
    return w


def branch_taken(ora, w, kind):
    """How many envs (with rows) take the start the case is named for, by the oracle's two costs, and how many have rows"""
    n = rows = 0
    for e in range(len(w)):
        cw, cs, nefc = start_costs(ora, e, w[e])
        if nefc:
            rows += 1
            n += (cw > cs) if kind == "smooth" else not (cw > cs)
    return n, rows


@pytest.mark.parametrize("kind", ["warm", "smooth"])
@pytest.mark.parametrize("env_id", [ANT, SPIDER])
def test_both_starts_win(env_id, kind):
    """96 placed states; Spider for three contact rows per lane, a contact pass that loops (3 ncon > 64) and one wave per SIMD."""
    p = _pair(env_id, 96)
    q0, v0 = reset_state(p.ora, p.N)
    q, v = placed_states(p.m, q0, v0, in_range=True)
    ctrl = np.random.default_rng(0).uniform(-1.5, 1.5, (p.N, p.eng.nu))
    w = warm_starts(p.ora, q, v, ctrl, kind, seed=21)
    counts = _parity(p, q, v, w, ctrl, seed=1)
    took, rows = branch_taken(p.ora, w, kind)
    print("%s: %d of %d envs with rows take the %s start; newton iterations mean %.2f" % (env_id, took, rows, kind, counts[:, 2].mean()))
    assert took >= p.N // 4, (took, rows)
    if env_id == SPIDER:
        assert (3 * counts[:, 0] > 64).sum() >= 8


def test_row_count_edges():
    """No row, limit rows only, one contact, 4 ncon = 64 and 68, the full contact list, a contact between two moving bodies (the
    dense-factorisation instance of the solver runs the same set-up): each asserted by count, with a non-zero warm start."""
    p = _pair(ANT, 96)
    q0, v0 = reset_state(p.ora, p.N)
    ctrl0 = np.random.default_rng(2).uniform(-1.5, 1.5, (p.N, p.eng.nu))
    q, v, ctrl, tags = edge_states(p.m, lambda n: OracleSim(p.m, n, maxcon=p.eng.maxcon, jbcap=p.eng.jbcap), q0, v0, ctrl0)
    tags = np.array(tags)
    w = warm_starts(p.ora, q, v, ctrl, "warm", seed=0) + 0.1 * np.random.default_rng(3).standard_normal(v.shape)
    counts = _parity(p, q, v, w, ctrl, seed=2)
    mov = np.array([two_moving(p.ora, p.m, e) for e in range(p.N)])
    ncon, nefc = counts[:, 0], counts[:, 1]
    print({t: int((tags == t).sum()) for t in np.unique(tags)}, "maxcon", p.eng.maxcon)
    assert ((nefc == 0) & (tags == "clear")).sum() >= 8
    assert ((ncon == 0) & (nefc > 0) & (tags == "limonly")).sum() >= 8
    for k in (1, 16, 17):
        assert (ncon == k).sum() >= 3, (k, np.bincount(ncon))
    assert (ncon == p.eng.maxcon).sum() >= 3
    assert (mov > 0).sum() >= 3


def test_hinges_past_both_limits():
    """Within one env some hinges past their lower and others past their upper limit (one evaluation per lane serves both kinds),
    velocities non-zero, on placed states and on lifted ones (limit rows only)."""
    p = _pair(ANT, 96)
    q0, v0 = reset_state(p.ora, p.N)
    q, v = placed_states(p.m, q0, v0, seed=12)
    rng = np.random.default_rng(4)
    nh = len(hinges(p.m))
    nlo = np.zeros(p.N, int)
    for e in range(p.N):
        if e % 3 == 0:
            lifted(p.m, q, e)
        nlo[e] = past_limits(p.m, q, v, e, rng, lo_share=(0.5, 0.25, 0.75, 0.0, 1.0)[e % 5]).sum()
    ctrl = rng.uniform(-1.5, 1.5, (p.N, p.eng.nu))
    w = warm_starts(p.ora, q, v, ctrl, "warm", seed=0) * 0.5
    counts = _parity(p, q, v, w, ctrl, seed=3)
    assert ((counts[:, 1] - 4 * counts[:, 0]) == nh).all()                 # every hinge has exactly one active side
    assert ((nlo > 0) & (nlo < nh)).sum() >= p.N // 2
    assert (counts[:, 0] == 0).sum() >= p.N // 3 and (counts[:, 0] > 0).sum() >= p.N // 4


def test_both_sides_of_one_hinge():
    """A model copy with two hinges whose range is narrower than twice their margin: both sides of those hinges are active at once
    (two rows of one dof), next to hinges with one side and with none."""
    base = mjcf.load_model(ANT)
    m2, mids = narrowed_model(base)
    p = _pair(None, 32, model=m2)
    q0, v0 = reset_state(p.ora, p.N)
    q, v = cr.place(m2, q0, v0, ["embedded", "floor"] * (p.N // 2), seed=14)
    rng = np.random.default_rng(5)
    nh = len(hinges(m2))
    expect = np.zeros(p.N, int)
    for e in range(p.N):
        if e % 4 == 0:
            lifted(m2, q, e)
        if e % 2:
            past_limits(m2, q, v, e, rng)
            expect[e] = nh - len(mids)
        else:
            for qa, _, lo, hi in hinges(m2):
                q[e, qa] = 0.5 * (lo + hi)
        for qa, mid in mids.items():
            q[e, qa] = mid + rng.uniform(-0.004, 0.004)
        expect[e] += 2 * len(mids)
    v[:, 6:] += rng.standard_normal(v[:, 6:].shape)
    ctrl = rng.uniform(-1.5, 1.5, (p.N, p.eng.nu))
    w = warm_starts(p.ora, q, v, ctrl, "warm", seed=0) * 0.5
    counts = _parity(p, q, v, w, ctrl, seed=4)
    assert ((counts[:, 1] - 4 * counts[:, 0]) == expect).all(), (counts[:, 1] - 4 * counts[:, 0], expect)


def test_fused_equals_stepwise():
    """Three rollout steps of 64 Ant envs from placed states through the fused launch and through the per-step launches: every returned
    array bitwise equal.  The kernels share the solver's code; this guards the hand-over of the set-up's state between them."""
    from robosumo_selfplay_amd import policies
    from robosumo_selfplay_amd.model import PPOModel
    from robosumo_selfplay_amd.runner import Runner
    from robosumo_selfplay_amd.vec_env import SumoVecEnv
    N, T = 64, 3
    outs = []
    for fused in (True, False):
        env = SumoVecEnv(ANT, num_envs=N, seed=5)
        D, A = env.observation_space[0].shape[0], env.action_space[0].shape[0]
        spec = policies.PolicySpec(D, A, value_network="copy", activation="relu")
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
        q0, v0, w0, cnt = E.get_state()
        fams = ["embedded", "floor", "edge", "piled"] * (N // 4)
        q, v = cr.place(env.model, q0, v0, fams, seed=15)
        a1 = int(env.model.agent_qposadr[1])
        for e, f in enumerate(fams):                      # the parked agent comes down beside the placed one: both in play
            if f != "piled":
                q[e, a1:a1 + 3] = [q[e, 0] * 0.3 - 0.8, q[e, 1] * 0.3 + 0.8, 0.6]
        E.set_state(q, v, w0, cnt)
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
