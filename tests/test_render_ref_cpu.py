"""CPU checks of the renderer's numpy reference (tests/render_ref.py): analytic pins at the centre pixel of a camera aimed along an
axis, the share of unstable pixels of every image the GPU test draws (a condition: at most 12 %), and coverage -- every primitive
type and both agents own stable pixels, so the stable mask cannot hide a primitive."""
import math
import types

import numpy as np
import pytest

import render_ref as rr
from robosumo_selfplay_amd import render


def _scene(geoms):
    """A model stand-in of (type, size, centre, rotation) tuples: what ``render_ref.cast`` reads."""
    m = types.SimpleNamespace(ngeom=len(geoms), geom_type=np.array([g[0] for g in geoms]),
                              geom_size=np.array([g[1] for g in geoms], np.float64))
    ctr = np.array([g[2] for g in geoms], np.float64)
    R = np.array([np.eye(3) if len(g) < 4 else g[3] for g in geoms], np.float64)
    return m, ctr, R


def _centre(geoms, eye, target, up=(0.0, 0.0, 1.0), size=5):
    """(id, face, depth, normal) at the centre pixel of an odd-sized square image: the ray is the camera's forward axis."""
    m, ctr, R = _scene(geoms)
    e, d = rr.rays(render.Camera(eye, target, up=up).record(), size, size)
    gid, face, depth, n = rr.cast(m, ctr, R, e, d)
    c = size // 2
    return int(gid[c, c]), int(face[c, c]), float(depth[c, c]), n[c, c]


def test_centre_ray_is_the_forward_axis():
    e, d = rr.rays(render.Camera((1, 2, 3), (4, 2, 3)).record(), 7, 5)
    assert np.allclose(d[2, 3], (1, 0, 0), atol=1e-7) and np.allclose(e, (1, 2, 3))
    assert d[0, 0, 2] > 0 and d[4, 0, 2] < 0 and d[2, 0, 1] > 0 and d[2, 6, 1] < 0       # row 0 is the top, column 0 the left


def test_sphere_depth():
    r, D = 0.4, 6.0
    gid, _, depth, n = _centre([(rr.SPHERE, (r, 0, 0), (D, 0, 0))], (0, 0, 0), (1, 0, 0))
    assert gid == 0 and abs(depth - (D - r)) < 1e-6 and np.allclose(n, (-1, 0, 0), atol=1e-6)


@pytest.mark.parametrize("theta", [0.0, 0.5, 1.2])
def test_plane_depth(theta):
    h = 2.5
    gid, _, depth, n = _centre([(rr.PLANE, (20, 20, 0.1), (0, 0, 0))], (0, 0, h), (math.sin(theta), 0, h - math.cos(theta)), up=(1, 0, 0))
    assert gid == 0 and abs(depth - h / math.cos(theta)) < 1e-5 and np.allclose(n, (0, 0, 1))
    assert _centre([(rr.PLANE, (20, 20, 0.1), (0, 0, 0))], (0, 0, -h), (0, 0, 0), up=(1, 0, 0))[0] == -1      # seen from +z only


def test_box_face():
    D = 5.0
    gid, face, depth, n = _centre([(rr.BOX, (0.3, 0.5, 0.7), (D, 0, 0))], (0, 0, 0), (1, 0, 0))
    assert (gid, face) == (0, 1) and abs(depth - (D - 0.3)) < 1e-6 and np.allclose(n, (-1, 0, 0))
    gid, face, depth, n = _centre([(rr.BOX, (0.3, 0.5, 0.7), (D, 0, 0))], (D, 0, 4), (D, 0, 0), up=(1, 0, 0))
    assert (gid, face) == (0, 4) and abs(depth - (4 - 0.7)) < 1e-6 and np.allclose(n, (0, 0, 1))


def test_capsule_wall_against_cap():
    r, h, D = 0.2, 0.5, 4.0
    cap = [(rr.CAPSULE, (r, h, 0), (D, 0, 0))]
    gid, _, depth, n = _centre(cap, (0, 0, 0.3), (1, 0, 0.3))
    assert gid == 0 and abs(depth - (D - r)) < 1e-6 and np.allclose(n, (-1, 0, 0), atol=1e-6)               # the wall
    z = h + r / 2
    gid, _, depth, n = _centre(cap, (0, 0, z), (1, 0, z))
    assert gid == 0 and abs(depth - (D - math.sqrt(r * r - (r / 2) ** 2))) < 1e-6                           # the hemisphere
    assert np.allclose(n, (-math.sqrt(0.75), 0, 0.5), atol=1e-6)
    assert _centre(cap, (0, 0, h + 1.01 * r), (1, 0, h + 1.01 * r))[0] == -1


def test_cylinder_end_against_wall():
    r, h, D = 0.2, 0.5, 4.0
    cyl = [(rr.CYLINDER, (r, h, 0), (D, 0, 0))]
    gid, face, depth, n = _centre(cyl, (0, 0, 0.3), (1, 0, 0.3))
    assert (gid, face) == (0, 0) and abs(depth - (D - r)) < 1e-6 and np.allclose(n, (-1, 0, 0), atol=1e-6)
    gid, face, depth, n = _centre(cyl, (D + 0.1, 0, 5), (D + 0.1, 0, 0), up=(1, 0, 0))
    assert (gid, face) == (0, 1) and abs(depth - (5 - h)) < 1e-6 and np.allclose(n, (0, 0, 1))              # the flat end
    gid, face, depth, n = _centre(cyl, (D, 0.1, -5), (D, 0.1, 0), up=(1, 0, 0))
    assert (gid, face) == (0, 2) and abs(depth - (5 - h)) < 1e-6 and np.allclose(n, (0, 0, -1))
    z = h + r / 2
    assert _centre(cyl, (0, 0, z), (1, 0, z))[0] == -1                                                      # no hemisphere there


def test_ray_between_two_geoms_is_sky_and_nearest_wins():
    two = [(rr.SPHERE, (0.5, 0, 0), (4, 1, 0)), (rr.SPHERE, (0.5, 0, 0), (4, -1, 0))]
    gid, _, depth, _ = _centre(two, (0, 0, 0), (1, 0, 0))
    assert gid == -1 and depth == np.inf
    row = [(rr.SPHERE, (0.5, 0, 0), (6, 0, 0)), (rr.SPHERE, (0.5, 0, 0), (3, 0, 0)), (rr.SPHERE, (0.5, 0, 0), (3, 0, 0))]
    gid, _, depth, _ = _centre(row, (0, 0, 0), (1, 0, 0))
    assert gid == 1 and abs(depth - 2.5) < 1e-9                                    # the nearest; on an exact tie the lower id


def test_rotated_geom_frame():
    c, s = math.cos(0.5 * math.pi), math.sin(0.5 * math.pi)
    Ry = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])                               # local z -> world x
    gid, face, depth, n = _centre([(rr.CYLINDER, (0.2, 0.5, 0), (4, 0, 0), Ry)], (0, 0, 0), (1, 0, 0))
    assert (gid, face) == (0, 2) and abs(depth - 3.5) < 1e-6 and np.allclose(n, (-1, 0, 0), atol=1e-9)


def test_shading_reads_the_package_constants():
    s = render.SHADING
    rgb = rr.shade_rgb(np.array([0, -1]), np.array([s["light"], (0, 0, 1.0)]), np.array([[0.72, 0.41, 0.13]]))
    k = s["ambient"] + s["diffuse"]
    assert rgb[0].tolist() == [int(round(255 * min(1.0, c * k))) for c in (0.72, 0.41, 0.13)]
    assert rgb[1].tolist() == [int(round(255 * c)) for c in s["sky"]]
    assert abs(np.linalg.norm(s["light"]) - 1.0) < 1e-12


@pytest.mark.parametrize("case", rr.all_cases(), ids=lambda c: "%s-%s-%s-%dx%d" % (c[0].split("-")[1] + c[0].split("-")[3], rr.STATE_NAMES[c[1]], c[2], c[3], c[4]))
def test_unstable_share_is_capped(case):
    ref = rr.reference(*case)
    share = 1.0 - ref["stable"].mean()
    print("unstable share %.4f" % share)
    assert share <= rr.UNSTABLE_CAP
    assert (ref["id"] >= 0).mean() > 0.5                                            # the view looks at the scene, not past it


@pytest.mark.parametrize("scene", rr.SCENES)
@pytest.mark.parametrize("view", rr.SIZES[(64, 48)])
def test_every_primitive_and_both_agents_own_stable_pixels(scene, view):
    m = rr.model(scene)
    ref = rr.reference(scene, 0, view, 64, 48)
    own = np.unique(ref["id"][ref["stable"] & (ref["id"] >= 0)])
    assert set(int(m.geom_type[g]) for g in own) == {rr.PLANE, rr.SPHERE, rr.CAPSULE, rr.CYLINDER, rr.BOX}
    roots = set(int(m.body_rootid[int(m.geom_bodyid[g])]) for g in own)
    assert roots >= set(int(m.body_rootid[int(b)]) for b in m.agent_torso)
