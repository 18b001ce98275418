"""The oracle's contact generation (``collision()`` of oracle/sumo_oracle.c) against elementary geometry (tests/contact_ref.py), at
states PLACED where a rollout from the reset pose never gets: tatami edges and corners, inside the tatami, on the floor, on the border
rods, one agent on top of the other, and contacts a hair inside / outside their margin.  The HIP engine's narrow phase was written as a
mirror of the oracle's, so a mistake the two share passes every engine-vs-oracle parity test; this module is what pins it.

Classes of a pair (contact_ref.SceneRef.cls): ``plane``; ``box<k>`` by the number k of clamped coordinates at the closest point of the
core to the tatami box (1 face, 2 edge, 3 corner), suffix ``i`` when the core touches or enters the box, ``m`` when the closest point
lies strictly inside a capsule's axis; ``ss`` / ``sc`` / ``cc`` / ``cc_par`` (parallel axes); suffix ``_rod`` with a border rod.

Every state is built once per scene (`_scene`) and shared by the tests below."""
import functools

import numpy as np
import pytest

import contact_ref as cr
from robosumo_selfplay_amd import mjcf

SCENES = ["RoboSumo-Ant-vs-Ant-v0", "RoboSumo-Spider-vs-Spider-v0", "RoboSumo-Bug-vs-Bug-v0", "RoboSumo-Spider-vs-Bug-v0"]
PER_FAMILY = 12                     # 6 families x 12 placed states + 6 skim classes x 4 twins = 96 envs per scene
SEED = {"RoboSumo-Ant-vs-Ant-v0": 1, "RoboSumo-Spider-vs-Spider-v0": 2, "RoboSumo-Bug-vs-Bug-v0": 3, "RoboSumo-Spider-vs-Bug-v0": 4}
FLOOR = 10                          # every class occurs at least this often over the module's states


class _Scene:
    pass


@functools.lru_cache(maxsize=None)
def _scene(env_id):
    from oracle import oracle
    oracle.build()
    s = _Scene()
    s.m = m = mjcf.load_model(env_id)
    s.fams = cr.family_list(m, PER_FAMILY)
    n = len(s.fams)
    sim = oracle.OracleSim(m, n)
    sim.reset(seeds=np.arange(n, dtype=np.uint64) + np.uint64(500))
    q0, v0, _, _ = sim.get_state()
    q, v = cr.place(m, q0, v0, s.fams, SEED[env_id])
    qs, vs, s.skim = cr.skim_set(m, oracle.OracleSim, SEED[env_id])
    s.nplaced = n
    s.q, s.v = np.concatenate([q, qs]), np.concatenate([v, vs])
    s.N = N = len(s.q)
    assert N <= 96
    sim = oracle.OracleSim(m, N)                          # default capacities: maxcon 128, no Jacobian-pool cap
    sim.set_state(s.q, s.v, np.zeros_like(s.v), np.zeros((N, 2), np.int32))
    s.con, s.counts = [], []
    for e in range(N):
        sim.forward(e, np.zeros(m.nu))
        s.counts.append(sim.array("counts", e))
        s.con.append(sim.array("contacts", e).reshape(-1, 9))
    s.stats = sim.stats()                                 # every env's single forward is one the fidelity counters sample
    s.ref = cr.SceneRef(m, s.q)
    return s


@pytest.mark.parametrize("env_id", SCENES)
def test_nothing_dropped_and_contacts_well_formed(env_id):
    s = _scene(env_id)
    assert s.stats["dropped"] == 0 and s.stats["forward"] == s.N
    for e in range(s.N):
        assert s.counts[e][2] == 0 and s.counts[e][0] == len(s.con[e])
        assert np.isfinite(s.con[e]).all()
        for c in s.con[e]:
            assert (int(c[7]), int(c[8])) in s.ref.pair_of
            assert abs(np.linalg.norm(c[4:7]) - 1.0) < 1e-12                      # unit normal
            assert c[0] < s.ref.margin[s.ref.pair_of[(int(c[7]), int(c[8]))]]      # active: inside the margin


@pytest.mark.parametrize("env_id", SCENES)
def test_completeness_and_distance(env_id):
    """Every pair the geometry puts inside its margin has a contact whose smallest distance is the geometric one to 1e-8; every pair
    the geometry puts outside has none.  Pairs within 1e-9 of the margin and pairs whose cores interpenetrate are not judged."""
    s = _scene(env_id)
    ref = s.ref
    judged = 0
    for e in range(s.N):
        by = cr.contacts_by_pair(s.con[e])
        for p in ref.in_contact(e):
            cls = ref.cls(e, p)
            if "i" in cls:
                continue
            key = (int(ref.g1[p]), int(ref.g2[p]))
            assert key in by, (e, p, cls, ref.dist[e, p])
            got = min(c[0] for c in by[key])
            assert abs(got - ref.dist[e, p]) < 1e-8, (e, p, cls, got, ref.dist[e, p])
            judged += 1
        for p in ref.clear(e):
            assert (int(ref.g1[p]), int(ref.g2[p])) not in by, (e, p, ref.cls(e, p), ref.dist[e, p])
    assert judged > 300


@pytest.mark.parametrize("env_id", SCENES)
def test_contact_point_and_normal(env_id):
    """For every contact whose cores do not interpenetrate (all contacts of the multi-contact generators included): stepping from the
    contact point by r + dist / 2 against / along the normal lands on the core of geom 1 / geom 2, and the normal points from geom 1 to
    geom 2.  (Plane contacts are checked even when an end point is below the plane: there the normal is the plane's.)"""
    s = _scene(env_id)
    m, ref = s.m, s.ref
    checked = 0
    for e in range(s.N):
        for c in s.con[e]:
            g1, g2 = int(c[7]), int(c[8])
            p = ref.pair_of[(g1, g2)]
            plane = ref.kind[p] == "plane"
            if not plane and ref.core[e, p] < cr.TOUCH:
                continue
            n = c[4:7]
            q1 = c[1:4] - n * (cr.radius(m, g1) + 0.5 * c[0])
            q2 = c[1:4] + n * (cr.radius(m, g2) + 0.5 * c[0])
            d1 = cr.core_distance_point(m, ref.ctr[e], ref.R[e], g1, q1)
            d2 = cr.core_distance_point(m, ref.ctr[e], ref.R[e], g2, q2)
            assert d1 < 1e-9 and d2 < 1e-9, (e, p, ref.cls(e, p), d1, d2)
            if plane:
                assert np.abs(n - ref.R[e, g1][:, 2]).max() < 1e-12
            else:
                sep = float(n @ (q2 - q1))                                        # = dist + r1 + r2 = the cores' separation, > 0
                assert sep > 0 and abs(sep - np.linalg.norm(q2 - q1)) < 1e-9, (e, p, ref.cls(e, p), sep)
            checked += 1
    assert checked > 300


def _inside_cases(s):
    """(env, pair, end centre, radius) of every sphere / capsule end sphere whose centre is strictly inside the tatami box."""
    m, ref = s.m, s.ref
    for p in range(m.npair):
        g1, g2 = int(ref.g1[p]), int(ref.g2[p])
        if cr.utype(m, g2) != cr.BOX:
            continue
        bs = np.asarray(m.geom_size[g2], np.float64)
        for e in range(s.N):
            a = cr.axis(m, ref.R[e], g1)
            for sg in ((0.0,) if cr.utype(m, g1) == cr.SPHERE else (1.0, -1.0)):
                c = ref.ctr[e, g1] + sg * a
                loc = ref.R[e, g2].T @ (c - ref.ctr[e, g2])
                if np.all(np.abs(loc) < bs - 1e-9):
                    yield e, p, c, loc, bs


@pytest.mark.parametrize("env_id", SCENES)
def test_inside_box_branch(env_id):
    """A sphere centre strictly inside the tatami is pushed out through the nearest face (the first minimum in the order x-, x+, y-,
    y+, z-, z+): the normal, which points from the sphere into the box, is minus that face's outward axis, and the distance is minus
    (depth to that face + radius)."""
    s = _scene(env_id)
    m, ref = s.m, s.ref
    seen = 0
    for e, p, c, loc, bs in _inside_cases(s):
        g1, g2 = int(ref.g1[p]), int(ref.g2[p])
        r = cr.radius(m, g1)
        depth = [abs(sg * bs[k] - loc[k]) for k in range(3) for sg in (-1.0, 1.0)]
        i = int(np.argmin(depth))                                                 # argmin returns the first minimum
        outward = np.zeros(3)
        outward[i // 2] = -1.0 if i % 2 == 0 else 1.0
        n = -(ref.R[e, g2] @ outward)
        dist = -depth[i] - r
        pos = c + n * (r + 0.5 * dist)
        rows = cr.contacts_by_pair(s.con[e]).get((g1, g2), [])
        hit = [row for row in rows if np.abs(row[1:4] - pos).max() < 1e-9]
        assert len(hit) >= 1, (e, p, loc, [row[:7] for row in rows])
        assert abs(hit[0][0] - dist) < 1e-9 and np.abs(hit[0][4:7] - n).max() < 1e-12, (e, p, hit[0][:7], dist, n)
        seen += 1
    assert seen >= FLOOR


def _through_cases(s):
    """(env, pair, exit point) of every capsule whose axis passes through the tatami with both ends outside: the axis is inside the box
    for t in [t_in, t_out], found by clipping against the three slabs."""
    m, ref = s.m, s.ref
    for p in range(m.npair):
        if ref.kind[p] != "cbox":
            continue
        g1, g2 = int(ref.g1[p]), int(ref.g2[p])
        bs = np.asarray(m.geom_size[g2], np.float64)
        for e in range(s.N):
            a = cr.axis(m, ref.R[e], g1)
            cl, al = ref.R[e, g2].T @ (ref.ctr[e, g1] - ref.ctr[e, g2]), ref.R[e, g2].T @ a
            if min(cr.point_box(cl + al, bs)[0], cr.point_box(cl - al, bs)[0]) < 1e-6:
                continue
            t0, t1 = -1.0, 1.0
            for k in range(3):
                if abs(al[k]) < 1e-12:
                    if abs(cl[k]) > bs[k]:
                        t0, t1 = 1.0, -1.0
                    continue
                ta, tb = (-bs[k] - cl[k]) / al[k], (bs[k] - cl[k]) / al[k]
                t0, t1 = max(t0, min(ta, tb)), min(t1, max(ta, tb))
            if t1 - t0 > 1e-6:
                yield e, p, ref.ctr[e, g1] + t1 * a


def _check_through(s):
    """Asserts that the third sphere of every capsule through the box sits where the axis leaves it; returns the number of cases."""
    m, ref = s.m, s.ref
    seen = 0
    for e, p, exit_point in _through_cases(s):
        g1, g2 = int(ref.g1[p]), int(ref.g2[p])
        rows = cr.contacts_by_pair(s.con[e]).get((g1, g2), [])
        centres = [row[1:4] - row[4:7] * (cr.radius(m, g1) + 0.5 * row[0]) for row in rows]
        assert any(np.abs(c - exit_point).max() < 1e-9 for c in centres), (e, p, exit_point, centres)
        seen += 1
    return seen


@pytest.mark.parametrize("env_id", SCENES)
def test_capsule_through_box_third_contact(env_id):
    """A capsule axis that passes through the tatami with both ends outside has distance zero on a whole stretch [t_in, t_out]: every
    point of it minimises, and the third contact's sphere must not sit at one that rounding picks (the engine's compilation would pick
    another).  The breakpoint search leaves the coordinate that sits on a face out of the derivative, which makes the derivative exactly
    zero at t_in and t_out, and settles on t_out: the sphere's centre is where the axis leaves the box."""
    assert _check_through(_scene(env_id)) >= 1


def test_capsule_through_box_sweep():
    """The same, on one state lifted through 96 steps of 1e-7: whether the coordinate that defines a breakpoint lands on its face
    exactly, or an ulp beside it, changes from step to step (the spider's first corner state has a long ankle capsule that leaves the
    tatami through its top face; about one step in 25 lands an ulp outside).  Without the `skip` of the breakpoint call those steps
    put the sphere where the axis ENTERS the box."""
    from oracle import oracle
    base = _scene("RoboSumo-Spider-vs-Spider-v0")
    e0 = base.fams.index("corner")
    s = _Scene()
    s.m, s.N = base.m, 96
    q, v = np.repeat(base.q[e0:e0 + 1], s.N, 0), np.repeat(base.v[e0:e0 + 1], s.N, 0)
    q[:, 2] += np.arange(s.N) * 1e-7
    sim = oracle.OracleSim(s.m, s.N)
    sim.set_state(q, v, np.zeros_like(v), np.zeros((s.N, 2), np.int32))
    s.con = []
    for e in range(s.N):
        sim.forward(e, np.zeros(s.m.nu))
        s.con.append(sim.array("contacts", e).reshape(-1, 9))
    s.ref = cr.SceneRef(s.m, q)
    assert _check_through(s) >= s.N


def _two_contact_parallel_pairs(s):
    """Parallel capsules make a contact at each end of capsule 1 that is within reach of capsule 2: asserts two contacts where both
    ends are, returns how many such pairs the scene's states hold."""
    m, ref = s.m, s.ref
    n = 0
    for e in range(s.N):
        by = cr.contacts_by_pair(s.con[e])
        for p in np.nonzero(ref.par[e])[0]:
            g1, g2 = int(ref.g1[p]), int(ref.g2[p])
            a1, a2 = cr.axis(m, ref.R[e], g1), cr.axis(m, ref.R[e], g2)
            reach = [cr.point_segment(ref.ctr[e, g1] + sg * a1, ref.ctr[e, g2], a2)[0] - cr.radius(m, g1) - cr.radius(m, g2)
                     for sg in (1.0, -1.0)]
            if all(d < ref.margin[p] - cr.TOUCH for d in reach) and ref.core[e, p] > cr.TOUCH:
                assert len(by.get((g1, g2), [])) == 2, (e, p, reach)
                n += 1
    return n


@pytest.mark.parametrize("env_id", SCENES)
def test_multiplicity_and_fidelity_counters(env_id):
    s = _scene(env_id)
    m, ref = s.m, s.ref
    cb3 = rodcap = 0
    for e in range(s.N):
        by = cr.contacts_by_pair(s.con[e])
        for (g1, g2), rows in by.items():
            p = ref.pair_of[(g1, g2)]
            if ref.kind[p] == "cbox":
                assert len(rows) <= 3
                cb3 += len(rows) == 3
            else:
                assert len(rows) <= (2 if ref.kind[p] in ("plane", "cc", "cc_rod") else 1), (e, p, ref.cls(e, p), len(rows))
            if int(m.geom_type[g2]) == cr.CYLINDER:                               # contact point beyond the rod's flat end: the capsule's cap
                ax = ref.R[e, g2][:, 2]
                rodcap += sum(abs((row[1:4] - ref.ctr[e, g2]) @ ax) > m.geom_size[g2][1] for row in rows)
    assert s.stats["capsule_box_3"] == cb3 and s.stats["rod_endcap"] == rodcap, (s.stats, cb3, rodcap)
    _two_contact_parallel_pairs(s)


@pytest.mark.parametrize("env_id", SCENES)
def test_skim_twins(env_id):
    """The chosen pair of a skim state sits at margin -+ delta by geometry; the oracle has the contact at - delta and not at + delta,
    and nothing else differs between the twins."""
    s = _scene(env_id)
    ref = s.ref
    for i, (cls, delta, sign, p) in enumerate(s.skim):
        e = s.nplaced + i
        assert abs(ref.dist[e, p] - (ref.margin[p] + sign * delta)) < 1e-12, (cls, delta, sign, ref.dist[e, p])
        has = (int(ref.g1[p]), int(ref.g2[p])) in cr.contacts_by_pair(s.con[e])
        assert has == (sign < 0), (cls, delta, sign)
        if sign > 0:
            assert len(s.con[e]) == len(s.con[e - 1]) - 1, (cls, delta)


def test_coverage_floor():
    """A condition, not a measurement: over the module's states every class of contact occurs at least FLOOR times, so that a change
    of seeds or families cannot silently empty one."""
    tot, skim, par2, through = {}, {}, 0, 0
    for env_id in SCENES:
        s = _scene(env_id)
        cov = cr.coverage_keys(s.ref.class_counts())
        for k, v in cov.items():
            tot[k] = tot.get(k, 0) + v
        for cls, delta, sign, p in s.skim:
            skim[(delta, sign)] = skim.get((delta, sign), 0) + 1
            skim[cls] = skim.get(cls, 0) + 1
        assert sum(1 for _ in _inside_cases(s)) >= FLOOR
        par2 += _two_contact_parallel_pairs(s)
        through += sum(1 for _ in _through_cases(s))
    print("contact classes over the module's states:", tot, skim, "two-contact parallel pairs:", par2)
    assert par2 >= 3                                      # (not one of the classes: that the two-contact case occurs at all)
    print("capsule axes through the tatami:", through)
    assert through >= FLOOR
    for k, v in tot.items():
        assert v >= FLOOR, (k, tot)
    for delta in cr.SKIM_DELTAS:
        for sign in (-1.0, 1.0):
            assert skim[(delta, sign)] >= FLOOR, skim
    for cls in cr.SKIM_CLASSES:
        assert skim[cls] >= 4 * len(SCENES)
