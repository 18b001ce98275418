"""The renderer's conventions restated in numpy float64, for tests of csrc/sumo_render.hip.

Written independently of the kernel: rays are intersected in WORLD space (the kernel works in each geom's frame), spheres and
cylinder walls through the plain quadratic (the kernel uses a closest-approach form), boxes face by face (the kernel uses slabs).
Geom frames come from ``contact_ref.geom_frames``; the shading constants are read from ``render.SHADING``, so they are inputs and
not numbers kept twice.

A pixel is *stable* when (a) the surface hit -- geom id and, where the normal jumps, the face: a box's six faces, a cylinder's wall
and two ends -- is the same at the pixel centre and at the four points 1/8 pixel away in x and in y, and (b) the hit is not grazing,
n . (-d) >= 0.05, or the pixel is sky.  On stable pixels float32 arithmetic cannot change what is hit; elsewhere it may.
"""
import numpy as np

import contact_ref
from robosumo_selfplay_amd import mjcf, render, render_capi

PLANE, SPHERE, CAPSULE, CYLINDER, BOX = mjcf.GEOM_PLANE, mjcf.GEOM_SPHERE, mjcf.GEOM_CAPSULE, mjcf.GEOM_CYLINDER, mjcf.GEOM_BOX
PROBES = ((0.0, 0.0), (0.125, 0.0), (-0.125, 0.0), (0.0, 0.125), (0.0, -0.125))
GRAZING = 0.05
UNSTABLE_CAP = 0.12

# the views of the GPU test: name -> (eye, target); sizes -> the views used at that size
VIEWS = {"arena": ((5.5, -5.5, 4.5), (0.0, 0.0, 0.6)), "close": ((1.5, -3.0, 1.6), (0.0, 0.0, 0.8)), "top": ((0.01, -0.02, 9.0), (0.0, 0.0, 0.5))}
SIZES = {(64, 48): ("arena", "close", "top"), (37, 21): ("arena", "top")}
SCENES = ("RoboSumo-Ant-vs-Ant-v0", "RoboSumo-Spider-vs-Bug-v0")


def view_camera(name):
    return render.Camera(*VIEWS[name])


def _dot(a, b):
    return (a * b).sum(-1)


def rays(cam, W, H, ox=0.0, oy=0.0):
    """(eye [3], unit directions [H][W][3]) of a float32 [16] camera record; (ox, oy) shifts every sample point, in pixels."""
    cam = np.asarray(cam, np.float64)
    eye, right, up, fwd, th = cam[0:3], cam[3:6], cam[6:9], cam[9:12], cam[12]
    x = np.arange(W)[None, :] + 0.5 + ox
    y = np.arange(H)[:, None] + 0.5 + oy
    u = (x / W * 2 - 1) * th * W / H
    v = (1 - y / H * 2) * th
    d = fwd + u[..., None] * right + v[..., None] * up
    return eye, d / np.sqrt(_dot(d, d))[..., None]


def _sphere(eye, d, c, r):
    oc = eye - c
    b = _dot(d, oc)
    disc = b * b - (_dot(oc, oc) - r * r)
    ok = disc >= 0
    t = -b - np.sqrt(np.where(ok, disc, 0.0))
    n = (oc + t[..., None] * d) / r
    return np.where(ok, t, np.inf), n


def _plane(eye, d, c, R):
    n = R[:, 2]
    denom = _dot(d, n)
    ok = (denom < 0) & (_dot(eye - c, n) > 0)
    t = _dot(c - eye, n) / np.where(ok, denom, 1.0)
    return np.where(ok, t, np.inf), np.broadcast_to(n, d.shape), np.zeros(d.shape[:-1], np.int64)


def _wall(eye, d, c, R, r, h):
    a = R[:, 2]
    oc = eye - c
    dp = d - _dot(d, a)[..., None] * a
    op = oc - _dot(oc, a) * a
    A, B, C = _dot(dp, dp), _dot(dp, op), _dot(op, op) - r * r
    disc = B * B - A * C
    ok = (A > 1e-24) & (disc >= 0)
    t = (-B - np.sqrt(np.where(ok, disc, 0.0))) / np.where(ok, A, 1.0)
    s = _dot(oc + t[..., None] * d, a)
    ok &= np.abs(s) <= h
    return np.where(ok, t, np.inf), (op + t[..., None] * dp) / r


def _capsule(eye, d, c, R, r, h):
    t, n = _wall(eye, d, c, R, r, h)
    a = R[:, 2]
    for sg in (1.0, -1.0):
        ce = c + sg * h * a
        ts, ns = _sphere(eye, d, ce, r)
        beyond = _dot(eye + np.where(np.isfinite(ts), ts, 0.0)[..., None] * d - ce, a) * sg >= 0
        ts = np.where(beyond, ts, np.inf)
        take = ts < t
        t, n = np.where(take, ts, t), np.where(take[..., None], ns, n)
    return t, n, np.zeros(d.shape[:-1], np.int64)


def _cylinder(eye, d, c, R, r, h):
    t, n = _wall(eye, d, c, R, r, h)
    face = np.zeros(d.shape[:-1], np.int64)
    a = R[:, 2]
    for k, sg in enumerate((1.0, -1.0)):
        ne, ce = sg * a, c + sg * h * a
        denom = _dot(d, ne)
        ok = (denom < 0) & (_dot(eye - ce, ne) > 0)
        te = _dot(ce - eye, ne) / np.where(ok, denom, 1.0)
        p = eye + te[..., None] * d - ce
        rad = p - _dot(p, a)[..., None] * a
        ok &= _dot(rad, rad) <= r * r
        te = np.where(ok, te, np.inf)
        take = te < t
        t, n, face = np.where(take, te, t), np.where(take[..., None], ne, n), np.where(take, k + 1, face)
    return t, n, face


def _box(eye, d, c, R, half):
    t = np.full(d.shape[:-1], np.inf)
    n = np.zeros(d.shape)
    face = np.zeros(d.shape[:-1], np.int64)
    for k in range(3):
        for j, sg in enumerate((1.0, -1.0)):
            nf = sg * R[:, k]
            denom = _dot(d, nf)
            ok = denom < 0
            tf = _dot(c + half[k] * nf - eye, nf) / np.where(ok, denom, 1.0)
            pl = (eye + tf[..., None] * d - c) @ R                        # the hit in the box's frame
            for o in range(3):
                if o != k:
                    ok &= np.abs(pl[..., o]) <= half[o]
            tf = np.where(ok, tf, np.inf)
            take = tf < t
            t, n, face = np.where(take, tf, t), np.where(take[..., None], nf, n), np.where(take, 2 * k + j, face)
    return t, n, face


def cast(m, ctr, R, eye, d):
    """Nearest hit with t > 0 of every ray: (id, face, depth, outward world normal).  On a tie the lower geom id wins; hits tie
    within ``render_capi.TIE_REL`` (an input, like the shading constants): capsules that meet at a joint share a hemisphere exactly,
    and there float64 noise would otherwise pick the id."""
    best = np.full(d.shape[:-1], np.inf)
    gid = np.full(d.shape[:-1], -1, np.int64)
    bface = np.zeros(d.shape[:-1], np.int64)
    bn = np.zeros(d.shape)
    for g in range(m.ngeom):
        ty, sz = int(m.geom_type[g]), m.geom_size[g]
        if ty == PLANE:
            t, n, face = _plane(eye, d, ctr[g], R[g])
        elif ty == SPHERE:
            t, n = _sphere(eye, d, ctr[g], sz[0])
            face = np.zeros(d.shape[:-1], np.int64)
        elif ty == CAPSULE:
            t, n, face = _capsule(eye, d, ctr[g], R[g], sz[0], sz[1])
        elif ty == CYLINDER:
            t, n, face = _cylinder(eye, d, ctr[g], R[g], sz[0], sz[1])
        elif ty == BOX:
            t, n, face = _box(eye, d, ctr[g], R[g], sz)
        else:
            raise ValueError("geom type %d" % ty)
        take = (t > 0) & (t * (1.0 + render_capi.TIE_REL) < best)
        best, gid, bface, bn = np.where(take, t, best), np.where(take, g, gid), np.where(take, face, bface), np.where(take[..., None], n, bn)
    return gid, bface, best, bn


def shade_rgb(gid, normal, colors, shading=None):
    s = render.SHADING if shading is None else shading
    k = s["ambient"] + s["diffuse"] * np.maximum(0.0, _dot(normal, np.asarray(s["light"], np.float64)))
    col = np.asarray(colors, np.float64)[np.maximum(gid, 0)] * k[..., None]
    col = np.where((gid >= 0)[..., None], col, np.asarray(s["sky"], np.float64))
    return np.rint(255.0 * np.clip(col, 0.0, 1.0)).astype(np.uint8)


def render_frames(m, ctr, R, cam, W, H, colors=None, shading=None):
    """One image of the geom frames (ctr [ngeom][3], R [ngeom][3][3]) through the camera record ``cam``: dict of id, depth, rgb,
    stable (bool) and probe_ids [5][H][W] (the id at the centre and at the four probe points)."""
    colors = render.default_colors(m) if colors is None else colors
    surf, ids = [], []
    for k, (ox, oy) in enumerate(PROBES):
        eye, d = rays(cam, W, H, ox, oy)
        gid, face, depth, n = cast(m, ctr, R, eye, d)
        surf.append(gid * 8 + face)
        ids.append(gid)
        if k == 0:
            out = dict(id=gid.astype(np.int32), depth=depth, rgb=shade_rgb(gid, n, colors, shading))
            facing = (gid < 0) | (-_dot(n, d) >= GRAZING)
    same = np.all(np.stack(surf[1:]) == surf[0], axis=0)
    out["stable"] = same & facing
    out["probe_ids"] = np.stack(ids).astype(np.int32)
    return out


def render_qpos(m, qpos, cam, W, H, colors=None):
    """The same from joint positions, with the geom poses rounded to float32 as the kernel receives them."""
    ctr, R = rounded_frames(m, qpos)
    return render_frames(m, ctr, R, cam, W, H, colors)


def rounded_frames(m, qpos):
    ctr, R = contact_ref.geom_frames(m, np.asarray(qpos, np.float64))
    return ctr.astype(np.float32).astype(np.float64), R.astype(np.float32).astype(np.float64)


def poses_array(m, qpos):
    """float64 [ngeom][12] in the layout of sumo_render_poses (centre, then the rotation row-major), not rounded."""
    ctr, R = contact_ref.geom_frames(m, np.asarray(qpos, np.float64))
    return np.concatenate([ctr, R.reshape(m.ngeom, 9)], axis=1)


# ---- the states of the tests -------------------------------------------------------------------------------------------------
def make_states(m, seed=0):
    """qpos [5][nq]: qpos0, random joint angles inside their ranges, every joint at its lower limit, every joint at its upper
    limit, and a state whose free joints carry random non-normalised quaternions (and moved positions)."""
    rng = np.random.default_rng(seed)
    q0 = np.asarray(m.qpos0, np.float64)
    hinge = [j for j in range(m.njnt) if int(m.jnt_type[j]) == mjcf.JNT_HINGE]
    adr = np.array([int(m.jnt_qposadr[j]) for j in hinge])
    lo, hi = m.jnt_range[hinge, 0], m.jnt_range[hinge, 1]
    rnd, low, upp, fre = q0.copy(), q0.copy(), q0.copy(), q0.copy()
    rnd[adr] = lo + (hi - lo) * rng.random(len(hinge))
    low[adr], upp[adr] = lo, hi
    fre[adr] = lo + (hi - lo) * rng.random(len(hinge))
    for j in range(m.njnt):
        if int(m.jnt_type[j]) == mjcf.JNT_FREE:
            a = int(m.jnt_qposadr[j])
            fre[a:a + 2] += rng.uniform(-0.3, 0.3, 2)
            fre[a + 2] += rng.uniform(0.0, 0.4)
            fre[a + 3:a + 7] = rng.standard_normal(4) * 1.7
    return np.stack([q0, rnd, low, upp, fre])


STATE_NAMES = ("qpos0", "random", "lower", "upper", "free")
FRAME_STATES = (0, 1, 4)      # the states the frame tests draw: one per env of an n = 3 launch


# ---- shared, computed once per session ---------------------------------------------------------------------------------------
_CACHE = {}


def model(scene):
    if scene not in _CACHE:
        _CACHE[scene] = mjcf.load_model(scene)
    return _CACHE[scene]


def states(scene):
    if ("states", scene) not in _CACHE:
        _CACHE["states", scene] = make_states(model(scene))
    return _CACHE["states", scene]


def reference(scene, state, view, W, H):
    """:func:`render_qpos` of state number ``state`` of ``scene`` through the named view; callers must not modify the result."""
    key = (scene, state, view, W, H)
    if key not in _CACHE:
        _CACHE[key] = render_qpos(model(scene), states(scene)[state], view_camera(view).record(), W, H)
    return _CACHE[key]


def all_cases():
    """Every (scene, state, view, W, H) the frame tests draw."""
    return [(sc, st, v, W, H) for sc in SCENES for st in FRAME_STATES for (W, H), views in SIZES.items() for v in views]
