"""Contact geometry restated in plain numpy float64, for tests of the oracle's and the HIP engine's narrow phase.

Nothing here is taken from ``oracle/sumo_oracle.c`` or ``csrc/sumo_engine.hip``: the core distances are written differently from their
clamping cascades on purpose (exhaustive segment-segment, golden-section segment-box), so that a mistake the two mirrors share does not
hide here as well.  A geom is its *core* (point, axis segment, box solid, half space) inflated by a radius; cylinders (the four border
rods) count as capsules of the same radius and half length (DESIGN.md deviation).

Also the placement families that put an agent where a rollout from the reset pose never gets: tatami edges and corners, inside the
tatami, on the floor, on the border rods, on top of the other agent, and `skim` twins whose chosen contact sits a hair inside / outside
its margin."""
import numpy as np

from robosumo_selfplay_amd import mjcf

PLANE, SPHERE, CAPSULE, CYLINDER, BOX = mjcf.GEOM_PLANE, mjcf.GEOM_SPHERE, mjcf.GEOM_CAPSULE, mjcf.GEOM_CYLINDER, mjcf.GEOM_BOX
TOUCH = 1e-9            # cores closer than this touch / interpenetrate (class suffix 'i'); also the band around the margin left unjudged
FAMILIES = ("edge", "corner", "embedded", "floor", "overlapped", "rods")
SKIM_CLASSES = ("plane", "box1", "box2", "rod", "cc", "sc")
SKIM_DELTAS = (1e-6, 1e-9)


# ---------------------------------------------------------------------------------------------------------------------------------
# geom frames
# ---------------------------------------------------------------------------------------------------------------------------------
def geom_frames(m, qpos):
    """World centre [ngeom, 3] and orientation [ngeom, 3, 3] of every geom at ``qpos``."""
    xpos, xquat, _, _ = mjcf.kinematics_np(m, qpos)
    ctr = np.zeros((m.ngeom, 3))
    R = np.zeros((m.ngeom, 3, 3))
    for g in range(m.ngeom):
        b = int(m.geom_bodyid[g])
        ctr[g] = xpos[b] + mjcf.quat2mat(xquat[b]) @ m.geom_pos[g]
        R[g] = mjcf.quat2mat(mjcf.quat_mul(xquat[b], m.geom_quat[g]))
    return ctr, R


def utype(m, g):
    t = int(m.geom_type[g])
    return CAPSULE if t == CYLINDER else t


def radius(m, g):
    return 0.0 if utype(m, g) in (PLANE, BOX) else float(m.geom_size[g][0])


def axis(m, R, g):
    """Half axis of a capsule / cylinder (zero for a sphere), batched like ``R``."""
    if utype(m, g) != CAPSULE:
        return np.zeros(R.shape[:-3] + (3,))
    return R[..., g, :, 2] * float(m.geom_size[g][1])


# ---------------------------------------------------------------------------------------------------------------------------------
# core distances (every argument batched over leading axes)
# ---------------------------------------------------------------------------------------------------------------------------------
def _norm(v):
    return np.sqrt((v * v).sum(-1))


def point_segment(p, c, a):
    """Distance from p to the segment c + t a, t in [-1, 1], and the t of the closest point (0 for a degenerate segment)."""
    aa = (a * a).sum(-1)
    t = np.where(aa > 0, ((p - c) * a).sum(-1) / np.where(aa > 0, aa, 1.0), 0.0)
    t = np.clip(t, -1.0, 1.0)
    return _norm(p - c - t[..., None] * a), t


def point_box(pl, bs):
    """Distance from a point in box coordinates to the solid box of half sizes bs, and the number of clamped coordinates."""
    q = np.clip(pl, -bs, bs)
    return _norm(pl - q), (np.abs(pl) > bs).sum(-1)


def segment_box(cl, al, bs, iters=75):
    """Distance from the segment cl + t al (box coordinates) to the box: golden-section search over the convex t -> dist.  Returns
    (dist, t, clamped coordinates at the closest point)."""
    f = lambda t: point_box(cl + t[..., None] * al, bs)[0]
    gr = (np.sqrt(5.0) - 1.0) / 2.0
    lo = -np.ones(cl.shape[:-1])
    hi = np.ones(cl.shape[:-1])
    x1, x2 = hi - gr * (hi - lo), lo + gr * (hi - lo)
    f1, f2 = f(x1), f(x2)
    for _ in range(iters):                                   # 2 * 0.618^75 < 1e-15
        left = f1 <= f2
        hi = np.where(left, x2, hi)
        lo = np.where(left, lo, x1)
        nx1, nx2 = hi - gr * (hi - lo), lo + gr * (hi - lo)
        nf1 = np.where(left, f(nx1), f2)
        nf2 = np.where(left, f1, f(nx2))
        x1, x2, f1, f2 = nx1, nx2, nf1, nf2
    t = 0.5 * (lo + hi)
    # the ends are candidates of their own: the search never evaluates t = +-1 exactly
    cand_t = np.stack([t, -np.ones_like(t), np.ones_like(t)])
    cand_d = np.stack([f(c) for c in cand_t])
    k = cand_d.argmin(0)
    t = np.take_along_axis(cand_t, k[None], 0)[0]
    d, ncl = point_box(cl + t[..., None] * al, bs)
    return d, t, ncl


def segment_segment(c1, a1, c2, a2):
    """Distance between two segments, exhaustively: the interior stationary point if it lies in [-1, 1]^2, and each of the four end
    points against the other segment.  Returns (dist, s, t): the parameters on segments 1 and 2."""
    d = c1 - c2
    A, B, Cc = (a1 * a1).sum(-1), (a1 * a2).sum(-1), (a2 * a2).sum(-1)
    u, v = (a1 * d).sum(-1), (a2 * d).sum(-1)
    det = A * Cc - B * B
    ok = det > 1e-14 * np.maximum(A * Cc, 1e-300)
    sdet = np.where(ok, det, 1.0)
    s = (B * v - Cc * u) / sdet                              # minimise |d + s a1 - t a2|^2
    t = (A * v - B * u) / sdet
    ok &= (np.abs(s) <= 1.0) & (np.abs(t) <= 1.0)
    best = np.where(ok, _norm(d + s[..., None] * a1 - t[..., None] * a2), np.inf)
    bs_, bt = np.where(ok, s, 0.0), np.where(ok, t, 0.0)
    for sg in (1.0, -1.0):
        dd, tt = point_segment(c1 + sg * a1, c2, a2)
        take = dd < best
        best, bs_, bt = np.where(take, dd, best), np.where(take, sg, bs_), np.where(take, tt, bt)
        dd, ss = point_segment(c2 + sg * a2, c1, a1)
        take = dd < best
        best, bs_, bt = np.where(take, dd, best), np.where(take, ss, bs_), np.where(take, sg, bt)
    return best, bs_, bt


def core_distance_point(m, ctr, R, g, x):
    """Distance from the world point x to the core of geom g in one env (ctr [ngeom, 3], R [ngeom, 3, 3])."""
    t = utype(m, g)
    if t == SPHERE:
        return float(_norm(x - ctr[g]))
    if t == CAPSULE:
        return float(point_segment(x, ctr[g], axis(m, R, g))[0])
    if t == BOX:
        return float(point_box(R[g].T @ (x - ctr[g]), m.geom_size[g])[0])
    return float(abs((x - ctr[g]) @ R[g][:, 2]))            # plane


# ---------------------------------------------------------------------------------------------------------------------------------
# per-pair reference and classifier
# ---------------------------------------------------------------------------------------------------------------------------------
class SceneRef:
    """Reference distances and classes of every pair of the model's pair list at N states.

    ``dist`` [N, npair]: surface distance (core distance minus radii; for a plane the lower end's signed distance minus the radius).
    ``core`` the core distance, ``ncl`` the clamped coordinates at the closest point (box pairs), ``tpar`` the closest parameter on
    the capsule of a capsule-box pair, ``par`` parallel capsule axes."""

    def __init__(self, m, qpos):
        self.m = m
        qpos = np.atleast_2d(qpos)
        N, P = qpos.shape[0], m.npair
        fr = [geom_frames(m, q) for q in qpos]
        self.ctr = np.stack([f[0] for f in fr])
        self.R = np.stack([f[1] for f in fr])
        self.g1 = np.asarray(m.pair_geom1, np.int64)
        self.g2 = np.asarray(m.pair_geom2, np.int64)
        self.margin = np.asarray(m.pair_margin, np.float64)
        self.dist = np.full((N, P), np.inf)
        self.core = np.full((N, P), np.inf)
        self.ncl = np.zeros((N, P), np.int64)
        self.tpar = np.zeros((N, P))
        self.par = np.zeros((N, P), bool)
        self.kind = [None] * P
        for p in range(P):
            self._pair(p)
        self.pair_of = {(int(a), int(b)): p for p, (a, b) in enumerate(zip(self.g1, self.g2))}

    def _pair(self, p):
        m, ctr, R = self.m, self.ctr, self.R
        g1, g2 = int(self.g1[p]), int(self.g2[p])
        t1, t2 = utype(m, g1), utype(m, g2)
        rr = radius(m, g1) + radius(m, g2)
        rod = "_rod" if CYLINDER in (int(m.geom_type[g1]), int(m.geom_type[g2])) else ""
        c1, c2, a1, a2 = ctr[:, g1], ctr[:, g2], axis(m, R, g1), axis(m, R, g2)
        if t1 == PLANE:
            n = R[:, g1, :, 2]
            ends = np.stack([((c2 + s * a2 - c1) * n).sum(-1) for s in (1.0, -1.0)])
            self.core[:, p] = ends.min(0)
            self.kind[p] = "plane"
        elif t2 == BOX:
            Rb = R[:, g2]
            cl = np.einsum("nji,nj->ni", Rb, c1 - c2)
            al = np.einsum("nji,nj->ni", Rb, a1)
            bs = np.asarray(m.geom_size[g2], np.float64)
            if t1 == SPHERE:
                d, ncl = point_box(cl, bs)
                t = np.zeros_like(d)
            else:
                d, t, ncl = segment_box(cl, al, bs)
            self.core[:, p], self.ncl[:, p], self.tpar[:, p] = d, ncl, t
            self.kind[p] = "box" if t1 == SPHERE else "cbox"
        elif t1 == SPHERE and t2 == SPHERE:
            self.core[:, p] = _norm(c2 - c1)
            self.kind[p] = "ss" + rod
        elif t1 == SPHERE and t2 == CAPSULE:
            self.core[:, p] = point_segment(c1, c2, a2)[0]
            self.kind[p] = "sc" + rod
        elif t1 == CAPSULE and t2 == CAPSULE:
            self.core[:, p] = segment_segment(c1, a1, c2, a2)[0]
            cr = np.cross(a1, a2)
            self.par[:, p] = _norm(cr) < 1e-9 * _norm(a1) * _norm(a2)
            self.kind[p] = "cc" + rod
        else:
            raise AssertionError("pair %d: geom types %d, %d are not ordered as the narrow phase expects" % (p, t1, t2))
        self.dist[:, p] = self.core[:, p] - rr

    def cls(self, e, p):
        """Class name of pair p in env e (see the module docstring of tests/test_oracle_contacts.py)."""
        k = self.kind[p]
        if k == "plane":
            return k
        if k in ("box", "cbox"):
            s = "box%d" % self.ncl[e, p]
            if self.core[e, p] < TOUCH:
                s += "i"
            if k == "cbox" and abs(self.tpar[e, p]) < 1.0 - 1e-9:
                s += "m"
            return s
        if k.startswith("cc") and self.par[e, p]:
            return "cc_par" + k[2:]
        return k

    def in_contact(self, e):
        """Pairs whose reference distance is below the margin by more than the unjudged band."""
        return np.nonzero(self.dist[e] < self.margin - TOUCH)[0]

    def clear(self, e):
        return np.nonzero(self.dist[e] > self.margin + TOUCH)[0]

    def class_counts(self, envs=None):
        out = {}
        for e in (range(self.dist.shape[0]) if envs is None else envs):
            for p in self.in_contact(e):
                c = self.cls(e, p)
                out[c] = out.get(c, 0) + 1
        return out

    def broad_phase_candidates(self, e, slack=1e-6):
        """(moving, world): lower bounds of the pairs that survive the engine's broad phase in env e.  Pairs of moving geoms pass on
        bounding spheres, |c1 - c2| <= margin + rbound1 + rbound2; a pair with a static geom passes when the moving geom's centre is
        within margin + rbound (+ the rod's radius) of the static geom's core.  `slack` is taken off every bound, so a pair counted
        here passes whatever the rounding of the engine's (rounded-up, float) bounds."""
        m = self.m
        gb = np.asarray(m.geom_bodyid)
        rb = np.asarray(m.geom_rbound, np.float64)
        nmov = nworld = 0
        for p in range(m.npair):
            g1, g2 = int(self.g1[p]), int(self.g2[p])
            if gb[g1] != 0 and gb[g2] != 0:
                nmov += _norm(self.ctr[e, g2] - self.ctr[e, g1]) <= self.margin[p] + rb[g1] + rb[g2] - slack
                continue
            gw, ga = (g1, g2) if gb[g1] == 0 else (g2, g1)
            if gb[ga] == 0:
                continue
            if utype(m, gw) == PLANE:
                d = max(float((self.ctr[e, ga] - self.ctr[e, gw]) @ self.R[e, gw][:, 2]), 0.0)
            else:
                d = core_distance_point(m, self.ctr[e], self.R[e], gw, self.ctr[e, ga])
            nworld += d <= self.margin[p] + rb[ga] + radius(m, gw) - slack
        return int(nmov), int(nworld)


def coverage_keys(counts):
    """Fold a class-count dict into the coverage classes the tests put a floor under."""
    f = lambda pred: sum(v for k, v in counts.items() if pred(k))
    return {
        "plane": f(lambda k: k == "plane"),
        "box1": f(lambda k: k.startswith("box1") and "i" not in k),
        "box2": f(lambda k: k.startswith("box2") and "i" not in k),
        "box2m": f(lambda k: k.startswith("box2") and "i" not in k and k.endswith("m")),
        "box3": f(lambda k: k.startswith("box3") and "i" not in k),
        "box*i": f(lambda k: k.startswith("box") and "i" in k),
        "ss": f(lambda k: k == "ss"),
        "sc": f(lambda k: k == "sc"),
        "cc": f(lambda k: k == "cc"),
        "cc_par": f(lambda k: k == "cc_par"),
        "cc_rod": f(lambda k: k in ("cc_rod", "cc_par_rod")),
        "sc_rod": f(lambda k: k == "sc_rod"),
    }


# ---------------------------------------------------------------------------------------------------------------------------------
# placement families
# ---------------------------------------------------------------------------------------------------------------------------------
def _rand_quat(rng):
    q = rng.standard_normal(4)
    return q / np.linalg.norm(q)


def _end_spheres(m, ctr, R, agent):
    """(centre, radius) of every sphere and capsule end sphere of one agent."""
    out = []
    b0, nb = int(m.agent_bodyadr[agent]), int(m.agent_nbody[agent])
    for g in range(m.ngeom):
        if not b0 <= int(m.geom_bodyid[g]) < b0 + nb:
            continue
        if utype(m, g) == SPHERE:
            out.append((ctr[g], radius(m, g)))
        else:
            a = axis(m, R, g)
            out += [(ctr[g] + a, radius(m, g)), (ctr[g] - a, radius(m, g))]
    return out


def place(m, q0, v0, families, seed):
    """States for the placement families 1-6.  ``q0`` / ``v0`` [N, nq] / [N, nv] are a seeded reset (hinge angles and velocities are kept,
    velocities halved); ``families`` names the family of each env.  Returns (qpos, qvel)."""
    rng = np.random.default_rng(seed)
    q, v = np.array(q0, np.float64), 0.5 * np.array(v0, np.float64)
    a0, a1 = int(m.agent_qposadr[0]), int(m.agent_qposadr[1])
    same = int(m.agent_nq[0]) == int(m.agent_nq[1]) and int(m.agent_nbody[0]) == int(m.agent_nbody[1])
    margin = float(np.max(m.pair_margin))
    seen = {}
    for e, fam in enumerate(families):
        i = seen[fam] = seen.get(fam, -1) + 1                                    # index of this env within its family
        q[e, a1 + 2] = rng.uniform(5.0, 6.0)                                      # the other agent is parked high above
        pos, quat = q[e, a0:a0 + 3], q[e, a0 + 3:a0 + 7]                          # views
        sx, sy = (1.0, 1.0) if i % 4 < 2 else ((-1.0, 1.0) if i % 4 == 2 else (1.0, -1.0))   # half as stated, half mirrored
        if fam == "edge":
            pos[:] = [sx * rng.uniform(2.0, 2.7), rng.uniform(-1.0, 1.0), rng.uniform(0.4, 0.9)]
            quat[:] = _rand_quat(rng)
            if i % 2:                                                             # along the y edge as well
                pos[[0, 1]] = pos[[1, 0]]
        elif fam == "corner":
            pos[:] = [sx * rng.uniform(2.0, 2.6), sy * rng.uniform(2.0, 2.6), rng.uniform(0.4, 0.9)]
            quat[:] = _rand_quat(rng)
            if i % 4 != 0:
                # directed: shift the agent so that a chosen end sphere lies within r + margin of the corner point, in the octant
                # (i % 4 == 1, 2) or the quadrant (3: an edge, z below the top) where that many coordinates clamp
                ctr, R = geom_frames(m, q[e])
                ends = _end_spheres(m, ctr, R, 0)
                c, r = ends[int(rng.integers(len(ends)))]
                bs, bc = np.asarray(m.geom_size[1], np.float64), np.asarray(m.geom_pos[1], np.float64)
                corner = bc + bs * np.array([sx, sy, 1.0])
                u = np.abs(rng.standard_normal(3)) + 0.05
                if i % 4 == 3:
                    u[2] = 0.0
                u = u / np.linalg.norm(u) * np.array([sx, sy, 1.0])
                target = corner + u * rng.uniform(0.2, 0.95) * (r + margin)
                if i % 4 == 3:
                    target[2] = bc[2] + bs[2] * rng.uniform(-0.6, 0.9)
                pos += target - c
        elif fam == "embedded":
            pos[:] = [rng.uniform(-1.0, 1.0), rng.uniform(-1.0, 1.0), rng.uniform(0.1, 0.6)]
            quat[:] = _rand_quat(rng)
        elif fam == "floor":
            if i % 2 == 0:
                pos[:] = [sx * rng.uniform(2.8, 4.0), rng.uniform(-2.0, 2.0), rng.uniform(0.0, 0.5)]
            else:
                far = rng.uniform(4.0, 18.0) * sx
                oth = rng.uniform(-18.0, 18.0)
                pos[:] = [far, oth, rng.uniform(0.0, 0.5)] if i % 4 == 1 else [oth, far, rng.uniform(0.0, 0.5)]
            quat[:] = _rand_quat(rng)
        elif fam in ("overlapped", "piled"):
            assert same, "the overlapped family needs two agents of one morphology"
            if fam == "overlapped":
                pos[:] = [rng.uniform(-1.0, 1.0), rng.uniform(-1.0, 1.0), rng.uniform(0.9, 1.3)]
            else:
                # the overlapped pair sunk into the tatami where two border rods meet: every moving geom is a broad-phase candidate of
                # the tatami and the floor, many of the rods as well -- with the agent-agent candidates, more than one candidate window
                pos[:] = [sx * rng.uniform(1.8, 2.1), sy * rng.uniform(1.8, 2.1), rng.uniform(0.15, 0.3)]
            n = int(m.agent_nq[0])
            q[e, a1:a1 + n] = q[e, a0:a0 + n]
            q[e, a1:a1 + 3] += [rng.uniform(0.1, 0.3 if fam == "piled" else 0.6), 0.3 * (1.0 if rng.random() < 0.5 else -1.0), 0.0]
        elif fam == "near":                                                       # (base states of agent-agent skim twins, any match-up)
            ang, d = rng.uniform(0.0, 2.0 * np.pi), rng.uniform(0.45, 1.7)
            pos[:2] = rng.uniform(-0.5, 0.5, 2)
            q[e, a1:a1 + 2] = pos[:2] + d * np.array([np.cos(ang), np.sin(ang)])
            q[e, a1 + 2] = pos[2]
        elif fam == "rods":
            pos[:] = [sx * rng.uniform(1.7, 2.2), rng.uniform(-1.9, 1.9), rng.uniform(0.45, 0.8)]
            if i % 4 == 3:                                                        # past the rod's flat end: the capsule's cap that a cylinder lacks
                pos[1] = sy * rng.uniform(1.9, 2.15)
            quat[:] = _rand_quat(rng)
            if i % 2:
                pos[[0, 1]] = pos[[1, 0]]
        else:
            raise ValueError(fam)
    return q, v


def family_list(m, per_family, families=FAMILIES):
    """``per_family`` envs of each family in turn; on a mixed match-up the overlapped family's share goes to edge and rods."""
    same = int(m.agent_nq[0]) == int(m.agent_nq[1]) and int(m.agent_nbody[0]) == int(m.agent_nbody[1])
    out = []
    for f in families:
        if f == "overlapped" and not same:
            out += ["edge"] * (per_family // 2) + ["rods"] * (per_family - per_family // 2)
        else:
            out += [f] * per_family
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# skim twins
# ---------------------------------------------------------------------------------------------------------------------------------
def skim_class(ref, e, p):
    """The skim class (one of SKIM_CLASSES) pair p of env e belongs to, or None."""
    m = ref.m
    c = ref.cls(e, p)
    gb = m.geom_bodyid
    world = gb[ref.g1[p]] == 0 or gb[ref.g2[p]] == 0
    if c == "plane":
        return "plane"
    if c in ("box1", "box1m", "box2", "box2m"):
        return c[:4]
    if c in ("cc_rod", "sc_rod"):
        return "rod"
    if c in ("cc", "sc") and not world:
        a = [int(np.searchsorted(np.asarray(m.agent_bodyadr), gb[g], side="right")) for g in (ref.g1[p], ref.g2[p])]
        return c if a[0] != a[1] else None                   # between the two agents: moving agent 1 changes the distance
    return None


def contacts_by_pair(con):
    """Oracle contact rows {dist, pos3, normal3, geom1, geom2} grouped by (geom1, geom2)."""
    out = {}
    for c in np.asarray(con).reshape(-1, 9):
        out.setdefault((int(c[7]), int(c[8])), []).append(c)
    return out


def skim_set(m, oracle_cls, seed, per_class=1, max_ncon=8):
    """Skim twins of one scene.  Base states come from the floor / edge / corner / rods / near placements; for each class of
    SKIM_CLASSES the first `per_class` contacts the oracle reports (default capacities) that are the only contact of their pair, in an
    env with at most `max_ncon` contacts, are taken, and each yields four states: distance margin - delta, margin + delta for delta
    in SKIM_DELTAS, in that order.  Returns (qpos, qvel, meta) with meta[i] = (class, delta, sign, pair index)."""
    fams = ["floor"] * 6 + ["edge"] * 10 + ["corner"] * 10 + ["rods"] * 10 + ["near"] * 28
    N = len(fams)
    sim = oracle_cls(m, N)
    sim.reset(seeds=np.arange(N, dtype=np.uint64) + np.uint64(900 + seed))
    q0, v0, _, _ = sim.get_state()
    q, v = place(m, q0, v0, fams, seed)
    sim.set_state(q, v, np.zeros_like(v), np.zeros((N, 2), np.int32))
    ref = SceneRef(m, q)
    chosen = {c: [] for c in SKIM_CLASSES}
    for e in range(N):
        sim.forward(e, np.zeros(m.nu))
        con = sim.array("contacts", e).reshape(-1, 9)
        if not 0 < len(con) <= max_ncon:
            continue
        for key, rows in contacts_by_pair(con).items():
            p = ref.pair_of[key]
            c = skim_class(ref, e, p)
            if c is None or len(rows) != 1 or len(chosen[c]) >= per_class:
                continue
            # not one of several contacts at the same distance (end spheres of two capsules that meet in a joint coincide): those
            # would cross the margin together
            alone = sum(abs(o[0] - rows[0][0]) < 1e-5 for o in con) == 1
            if alone and rows[0][0] < ref.margin[p] - 10 * max(SKIM_DELTAS) and abs(rows[0][0] - ref.dist[e, p]) < 1e-9:
                chosen[c].append((e, rows[0], p))
    qs, vs, meta = [], [], []
    for c in SKIM_CLASSES:
        assert len(chosen[c]) == per_class, "no base state for the skim class %s (found %d)" % (c, len(chosen[c]))
        for e, row, p in chosen[c]:
            for delta in SKIM_DELTAS:
                for sign in (-1.0, 1.0):
                    qs.append(skim_states(m, q, e, row, sign * delta))
                    vs.append(v[e])
                    meta.append((c, delta, sign, p))
    return np.array(qs), np.array(vs), meta


def skim_states(m, q, e, contact, delta_signed):
    """qpos of env e moved so that ``contact`` (an oracle row {dist, pos3, normal3, g1, g2}) gets the distance margin + delta_signed:
    agent 0 moves away from a static geom, agent 1 away from agent 0, rigidly along the contact normal."""
    dist, n, g1, g2 = contact[0], contact[4:7], int(contact[7]), int(contact[8])
    gb = m.geom_bodyid
    p = [k for k in range(m.npair) if m.pair_geom1[k] == g1 and m.pair_geom2[k] == g2][0]
    s = float(m.pair_margin[p]) + delta_signed - dist
    out = np.array(q[e], np.float64)
    if gb[g1] == 0 or gb[g2] == 0:
        a = int(m.agent_qposadr[0])
        out[a:a + 3] += (n if gb[g1] == 0 else -n) * s
    else:
        b1 = int(m.agent_bodyadr[1])
        a = int(m.agent_qposadr[1])
        out[a:a + 3] += (n if gb[g2] >= b1 else -n) * s
    return out
