"""The HIP engine's narrow phase and contact bookkeeping (``collision()`` of csrc/sumo_engine.hip) against the oracle at PLACED states:
tatami edges and corners, inside the tatami, the floor plane, the border rods, one agent on top of a copy of itself, and contacts a
hair inside / outside their margin (tests/contact_ref.py has the families; tests/test_oracle_contacts.py pins the oracle's side of
these very branches against plain geometry).  A rollout from the reset pose reaches none of this: the episode ends first.

What each test reaches is asserted with the numpy classifier of contact_ref, so that a change of seeds cannot silently empty a family.

Oracle sensitivity (CPU, oracle alone, one forward, qpos perturbed by 1e-13 relative; relerr of qacc as in test_gpu_env_parity), maximum
over the 96 placed states of each match-up, and how many envs exceed 1e-11 (those are left out of the qacc comparison, never out of the
count comparisons; at most 5 % of a scene's envs may be):

    Ant-vs-Ant 1.0e-11 (1)    Ant-vs-Bug 6.6e-12 (0)    Ant-vs-Spider 8.3e-12 (0)
    Bug-vs-Ant 1.2e-11 (1)    Bug-vs-Bug 4.2e-12 (0)    Bug-vs-Spider 3.8e-12 (0)
    Spider-vs-Ant 7.4e-12 (0) Spider-vs-Bug 8.5e-12 (0) Spider-vs-Spider 4.3e-11 (1)

qvel after a full env step from the states of test_step_parity_from_placed_states, same perturbation: Ant-vs-Ant 2.3e-12, Ant-vs-Bug 2.6e-12,
Bug-vs-Ant 3.5e-12, Spider-vs-Ant 4.0e-12, Bug-vs-Spider 1.5e-12.  The engine's qacc differed from the oracle's by at most 1.0e-13 on these
states when the tests were written.
"""
import numpy as np
import pytest

import contact_ref as cr
from conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    from robosumo_selfplay_amd import mjcf
    from test_gpu_env_parity import Pair, relerr

ALL = ["RoboSumo-%s-vs-%s-v0" % (a, b) for a in ("Ant", "Bug", "Spider") for b in ("Ant", "Bug", "Spider")]
REL = 1e-9              # the tolerance of test_forward_dynamics_parity
SENS_MAX = 1e-11        # envs whose oracle sensitivity exceeds this are left out of the qacc comparison ...
SENS_SHARE = 0.05       # ... at most this share of a scene's envs


def _same(m):
    return int(m.agent_nq[0]) == int(m.agent_nq[1]) and int(m.agent_nbody[0]) == int(m.agent_nbody[1])


def _zeros(p, n=None):
    n = p.N if n is None else n
    return np.zeros((n, p.eng.nv)), np.zeros((n, 2), np.int32)


def _set_both(p, q, v):
    w, c = _zeros(p)
    p.ora.set_state(q, v, w, c)
    p.eng.set_state(q, v, w, c)


def _reset_state(p):
    p.reset()
    q0, v0, _, _ = p.ora.get_state()
    return q0, v0


def oracle_sensitivity(ora, q, v, ctrl, rng):
    """relerr of the oracle's qacc between q and q (1 + 1e-13 u), u ~ U(-1, 1), per env; leaves the oracle at (q, v)."""
    N = len(q)
    w, c = np.zeros_like(v), np.zeros((N, 2), np.int32)
    base = []
    ora.set_state(q, v, w, c)
    for e in range(N):
        ora.forward(e, ctrl[e])
        base.append(ora.array("qacc", e))
    ora.set_state(q * (1.0 + 1e-13 * rng.uniform(-1.0, 1.0, q.shape)), v, w, c)
    out = np.zeros(N)
    for e in range(N):
        ora.forward(e, ctrl[e])
        a = ora.array("qacc", e)
        out[e] = np.abs(a - base[e]).max() / (1.0 + np.abs(base[e]).max())
    ora.set_state(q, v, w, c)
    return out


def _forward_parity(p, q, v, seed, check_sensitivity=True):
    """One mj_forward of both sides from (q, v) with ctrl ~ U(-1.5, 1.5): per env ncon, nefc and dropped equal, qacc to REL.  Returns the
    engine's counts [N, 4] = {ncon, nefc, newton, dropped}."""
    rng = np.random.default_rng(seed)
    ctrl = rng.uniform(-1.5, 1.5, (p.N, p.eng.nu))
    sens = oracle_sensitivity(p.ora, q, v, ctrl, rng) if check_sensitivity else np.zeros(p.N)
    out = sens > SENS_MAX
    print("oracle sensitivity: max %.2e, %d of %d envs above %.0e" % (sens.max(), out.sum(), p.N, SENS_MAX))
    assert out.sum() <= SENS_SHARE * p.N, (sens.max(), out.sum())
    _set_both(p, q, v)
    qacc, counts = p.eng.debug_forward(ctrl)
    worst = 0.0
    for e in range(p.N):
        d0 = p.ora.array("counts", e)[2]
        p.ora.forward(e, ctrl[e])
        oc = p.ora.array("counts", e)
        assert (counts[e, 0], counts[e, 1], counts[e, 3]) == (oc[0], oc[1], oc[2] - d0), (e, counts[e], oc, d0)
        if not out[e]:
            err = relerr(qacc[e], p.ora.array("qacc", e))
            worst = max(worst, err)
            assert err < REL, (e, err, sens[e])
    print("qacc relerr: max %.2e over %d envs; ncon max %d, dropped in %d envs" % (worst, p.N - out.sum(), counts[:, 0].max(),
                                                                                  (counts[:, 3] > 0).sum()))
    return counts


def _placed(env_id, per_family=16, seed=11):
    p = Pair(env_id, 6 * per_family)
    fams = cr.family_list(p.m, per_family)
    q0, v0 = _reset_state(p)
    q, v = cr.place(p.m, q0, v0, fams, seed)
    return p, fams, q, v


def _coverage(m, q, need):
    cov = cr.coverage_keys(cr.SceneRef(m, q).class_counts())
    print("classes:", cov)
    for k, n in need.items():
        assert cov[k] >= n, (k, cov)
    return cov


# every placed batch holds each of these at least this often (a floor under the seeds, far below what they give)
NEED = {"plane": 10, "box1": 10, "box2": 5, "box2m": 3, "box3": 3, "box*i": 10, "cc_rod": 5, "sc_rod": 3}
NEED_SAME = {"cc": 10, "sc": 5, "cc_par": 5}
NO_PAR = "Spider"       # a spider's legs are thin (r = 0.04) and steep: at the overlapped family's shifts (>= 0.316) no copy of a leg touches its original


@pytest.mark.parametrize("env_id", ALL)
def test_forward_parity_at_placed_states(env_id):
    """(a) all nine match-ups, 16 states of each placement family (on a mixed match-up the overlapped family's share goes to edge and
    rods): contact, constraint-row and dropped counts equal per env, qacc to 1e-9.  (b) on the same-morphology match-ups the embedded
    family fills the contact list (ncon == maxcon, the rest dropped) and the overlapped family exhausts the Jacobian pool first
    (dropped > 0 with ncon < maxcon), each in at least 8 envs, with the oracle's counts."""
    p, fams, q, v = _placed(env_id)
    need = dict(NEED, **(NEED_SAME if _same(p.m) else {}))
    if NO_PAR in env_id:
        need.pop("cc_par", None)
    _coverage(p.m, q, need)
    counts = _forward_parity(p, q, v, seed=0)
    if _same(p.m):
        fam = np.array(fams)
        emb, ovl = counts[fam == "embedded"], counts[fam == "overlapped"]
        print("maxcon %d jbcap %d; embedded ncon %s dropped %s; overlapped ncon %s dropped %s" % (
            p.eng.maxcon, p.eng.jbcap, emb[:, 0].tolist(), emb[:, 3].tolist(), ovl[:, 0].tolist(), ovl[:, 3].tolist()))
        both = counts[(fam == "embedded") | (fam == "overlapped")]
        assert (both[:, 3] > 0).sum() >= 8
        assert (emb[:, 0] == p.eng.maxcon).sum() >= 8                                       # the contact cap
        assert ((ovl[:, 0] < p.eng.maxcon) & (ovl[:, 3] > 0)).sum() >= 8                    # the Jacobian-pool cap


def _maxcand(maxcon):
    return 192 if 8 * maxcon >= 192 else (8 * maxcon) // 64 * 64                            # as build_layout sizes the candidate window


@pytest.mark.parametrize("flag", ["1", "0"])
@pytest.mark.parametrize("env_id,family", [("RoboSumo-Spider-vs-Spider-v0", "overlapped"), ("RoboSumo-Ant-vs-Ant-v0", "piled")])
def test_candidate_window(monkeypatch, env_id, family, flag):
    """(c) the broad phase keeps `maxcand` candidates per window and runs its tests again for the next window.  Overlapped spiders have
    more agent-agent bounding-sphere candidates than one window holds (192), so the `do ... while (base < total)` loop really loops,
    in the static-Layout and in the runtime-Layout kernels.  An Ant scene cannot get there: its 413 pairs give at most 73 agent-agent
    candidates (agents coincident; 34..59 at the family's shifts) and a geom cannot be near the floor and a rod at once, so a little
    over 100 candidates (81..106 in this test's states) is what a state gets to, against a window of 128.  Its case takes the fullest queue the scene has -- the
    overlapped pair sunk into the tatami where two rods meet -- which still runs the 64-candidate narrow-phase batch loop twice and
    passes the contact cap inside a batch."""
    monkeypatch.setenv("SUMO_STATIC_LAYOUT", flag)
    p = Pair(env_id, 16)
    assert p.eng.static_layout() == (flag == "1")
    maxcand = _maxcand(p.eng.maxcon)
    if flag == "1":
        assert maxcand == (128 if "Ant" in env_id else 192)
    q0, v0 = _reset_state(p)
    q, v = cr.place(p.m, q0, v0, [family] * p.N, seed=3)
    ref = cr.SceneRef(p.m, q)
    cand = np.array([ref.broad_phase_candidates(e) for e in range(p.N)])
    print("maxcand %d; candidates (moving, world) per env: %s" % (maxcand, cand.tolist()))
    if family == "overlapped":
        assert (cand[:, 0] > maxcand).sum() >= 8
    else:
        assert (cand.sum(1) > 64).sum() >= 8
    counts = _forward_parity(p, q, v, seed=1)
    assert (counts[:, 3] > 0).sum() >= 8


SKIM_SEED = {"RoboSumo-Ant-vs-Ant-v0": 1, "RoboSumo-Spider-vs-Spider-v0": 2, "RoboSumo-Bug-vs-Bug-v0": 3, "RoboSumo-Spider-vs-Bug-v0": 4}   # test_oracle_contacts' states


@pytest.mark.parametrize("env_id", list(SKIM_SEED))
def test_skim_states(env_id):
    """(d) a contact at margin - delta exists, its twin at margin + delta does not, delta = 1e-6 and 1e-9, one twin pair of each class
    plane / box face / box edge / rod / capsule-capsule / sphere-capsule: the engine's broad phase (box-extent distance against a
    rounded-up float bound for pairs with a static geom) and its `dist < margin` agree with the oracle's on both sides of the margin."""
    from oracle.oracle import OracleSim
    m = mjcf.load_model(env_id)
    q, v, meta = cr.skim_set(m, OracleSim, seed=SKIM_SEED[env_id])
    p = Pair(env_id, len(q))
    p.reset()
    counts = _forward_parity(p, q, v, seed=2, check_sensitivity=False)
    assert (counts[:, 3] == 0).all()
    ref = cr.SceneRef(m, q)
    for i, (cls, delta, sign, pr) in enumerate(meta):
        assert abs(ref.dist[i, pr] - (ref.margin[pr] + sign * delta)) < 1e-12
        if sign > 0:
            assert counts[i, 0] == counts[i - 1, 0] - 1, (cls, delta, counts[i - 1], counts[i])


def test_through_box_sweep_parity():
    """The states of test_oracle_contacts.test_capsule_through_box_sweep: a spider ankle through the tatami's corner, lifted in 96 steps of
    1e-7.  The engine finds its breakpoints with fast_rcp where the oracle divides, so the coordinate that defines a breakpoint lands
    on its face, or an ulp beside it, at other steps than the oracle's -- the `skip` of the breakpoint call makes both settle on the
    same end of the zero-distance stretch all the same."""
    from test_oracle_contacts import _scene
    base = _scene("RoboSumo-Spider-vs-Spider-v0")
    e0 = base.fams.index("corner")
    p = Pair("RoboSumo-Spider-vs-Spider-v0", 96)
    p.reset()
    q, v = np.repeat(base.q[e0:e0 + 1], p.N, 0), np.repeat(base.v[e0:e0 + 1], p.N, 0)
    q[:, 2] += np.arange(p.N) * 1e-7
    _forward_parity(p, q, v, seed=4)


STEP_TOL = {"RoboSumo-Ant-vs-Ant-v0": 1e-9}       # 1e-6 for scenes with a Spider or a Bug: the tolerances of test_step_parity_with_resync


@pytest.mark.parametrize("env_id", ["RoboSumo-Ant-vs-Ant-v0", "RoboSumo-Ant-vs-Bug-v0", "RoboSumo-Bug-vs-Ant-v0", "RoboSumo-Spider-vs-Ant-v0",
                                    "RoboSumo-Bug-vs-Spider-v0"])
def test_step_parity_from_placed_states(env_id):
    """(e) two full env steps (zero actions, then N(0, 1)) from edge / embedded / overlapped (same morphology only) / rods states, the
    device re-synchronised to the oracle in between.  Many envs end at once, through the out-of-ring and height tests."""
    tol = STEP_TOL.get(env_id, 1e-6)
    m = mjcf.load_model(env_id)
    fams = cr.family_list(m, 16, ("edge", "embedded", "overlapped", "rods") if _same(m) else ("edge", "embedded", "rods"))
    p = Pair(env_id, len(fams))
    q0, v0 = _reset_state(p)
    q, v = cr.place(m, q0, v0, fams, seed=13)
    _coverage(m, q, {"box1": 5, "box2": 3, "box*i": 10, "cc_rod": 3})
    _set_both(p, q, v)
    rng = np.random.default_rng(6)
    ndone = 0
    for t in range(2):
        a = np.zeros((p.N, 2, p.eng.act_stride), np.float32) if t == 0 else rng.standard_normal((p.N, 2, p.eng.act_stride)).astype(np.float32)
        (gobs, ginfo, gdone, gr, gdr, gl), (oobs, oinfo, odone, orr, odr, ol) = p.step(a)
        assert np.array_equal(gdone, odone) and np.array_equal(ginfo[:, :, 7], oinfo[:, :, 7]) and np.array_equal(gl, ol)
        gs, os_ = p.eng.get_state(), p.ora.get_state()
        print("step %d: done %d, obs %.2e, info %.2e, qpos %.2e, qvel %.2e, warm %.2e" % (
            t, gdone[:, 0].sum(), np.abs(gobs - oobs).max(), relerr(ginfo, oinfo), relerr(gs[0], os_[0]), relerr(gs[1], os_[1]),
            relerr(gs[2], os_[2])))
        if tol <= 1e-9:
            assert np.array_equal(gobs, oobs), np.abs(gobs - oobs).max()
        else:
            assert np.abs(gobs - oobs).max() < 1e-5
        assert relerr(ginfo, oinfo) < tol and relerr(gr, orr) < tol and relerr(gdr, odr) < tol
        assert relerr(gs[0], os_[0]) < tol and relerr(gs[1], os_[1]) < tol and relerr(gs[2], os_[2]) < 1e3 * tol
        assert np.array_equal(gs[3], os_[3])
        ndone += int(gdone[:, 0].sum())
        p.eng.set_state(*os_)
    gst, ost = p.eng.stats(), p.ora.stats()
    print({k: (gst[k], ost[k]) for k in ("capsule_box_3", "rod_endcap", "dropped", "max_ncon")}, "done", ndone)
    for k in ("capsule_box_3", "rod_endcap", "dropped", "max_ncon"):
        assert gst[k] == ost[k], (k, gst[k], ost[k])
    assert gst["capsule_box_3"] > 0 and gst["rod_endcap"] > 0
    assert ndone >= 8


@pytest.mark.parametrize("env_id", ["RoboSumo-Ant-vs-Ant-v0", "RoboSumo-Ant-vs-Bug-v0"])
def test_cfrc_ext_at_edges_and_rods(env_id):
    """(f) cfrc_mode = 'rne_post' from edge and rods states, compared the way test_gpu_cfrc.test_cfrc_ext_matches_oracle compares."""
    m = mjcf.load_model(env_id)
    fams = ["edge"] * 16 + ["rods"] * 16
    p = Pair(env_id, len(fams))
    p.eng.set_cfrc_mode("rne_post")
    p.ora.set_cfrc_mode("rne_post")
    q0, v0 = _reset_state(p)
    q, v = cr.place(m, q0, v0, fams, seed=17)
    _coverage(m, q, {"box2": 2, "cc_rod": 3})
    _set_both(p, q, v)
    rng = np.random.default_rng(3)
    nb = p.eng.nbody
    seen = 0
    for t in range(2):
        a = (rng.standard_normal((p.N, 2, p.eng.act_stride)) * 0.8).astype(np.float32)
        (gobs, ginfo, gdone, *_), (oobs, oinfo, odone, *_) = p.step(a)
        assert np.array_equal(gdone, odone)
        g = p.eng.get_cfrc_ext()
        for e in range(p.N):
            if gdone[e, 0]:
                continue
            o = p.ora.array("cfrc_ext", e).reshape(nb, 6)
            scale = 1.0 + np.abs(o).max()
            assert np.abs(g[e] - o).max() < 1e-7 * scale, (t, e, np.abs(g[e] - o).max())
            seen += int(np.abs(o).max() > 1.0)
        assert np.abs(gobs - oobs).max() < 2e-5
        p.eng.set_state(*p.ora.get_state())
    assert seen >= 8, seen
