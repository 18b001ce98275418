"""The Newton loop's gradient test as a threshold (csrc/engine_host_scene.h: grad_threshold, exported as sumo_debug_grad_threshold).  The
kernel breaks on ``scale * sqrt(gn) < tol``, gn the squared gradient norm; sumo_create bisects once per scene for the largest float64 G
for which that holds and the kernel tests ``gn <= G``.  Here, for the options of the nine scenes and two further tolerances, with the
test D evaluated in numpy float64: D(G) holds, D(nextafter(G, inf)) does not, and D is non-increasing over the 512 doubles on either
side of G -- so the two forms agree on every gn >= 0.  Host only: the export touches no device."""
import numpy as np
import pytest

from robosumo_selfplay_amd import capi, mjcf

NAMES = ("Ant", "Bug", "Spider")
ENV_IDS = ["RoboSumo-%s-vs-%s-v0" % (a, b) for a in NAMES for b in NAMES]
EXTRA_TOL = (1e-4, 1e-1)
WINDOW = 512
OPT_TOLERANCE, OPT_MEANINERTIA = 4, 5


def scene_scale_tol(env_id):
    """(scale, tol) as newton_solve forms them from the model's options"""
    m = mjcf.load_model(env_id)
    nv = int(m.nv)
    return 1.0 / (float(m.opt[OPT_MEANINERTIA]) * (nv if nv > 1 else 1)), float(m.opt[OPT_TOLERANCE])


def D(scale, tol, gn):
    with np.errstate(invalid="ignore"):
        return np.float64(scale) * np.sqrt(np.asarray(gn, np.float64)) < np.float64(tol)


def window(G, n=WINDOW):
    """the n doubles below G, G, the n doubles above G, ascending (G > 0 and far from the ends of the range)"""
    bits = np.float64(G).view(np.uint64)
    return (bits + np.arange(-n, n + 1, dtype=np.int64).astype(np.uint64)).view(np.float64)


CASES = [(e, None) for e in ENV_IDS] + [(ENV_IDS[0], t) for t in EXTRA_TOL]


@pytest.mark.parametrize("env_id,tol_override", CASES)
def test_threshold_is_the_last_passing_double(env_id, tol_override):
    scale, tol = scene_scale_tol(env_id)
    if tol_override is not None:
        tol = tol_override
    G = capi.grad_threshold(scale, tol)
    print("%s: scale %.17g tol %g -> G %.17g (%s)" % (env_id, scale, tol, G, np.float64(G).hex()))
    assert G > 0 and np.isfinite(G)
    assert D(scale, tol, G) and not D(scale, tol, np.nextafter(G, np.inf))
    w = window(G)
    d = D(scale, tol, w)
    assert w[WINDOW] == G and (np.diff(w) > 0).all()
    assert not (~d[:-1] & d[1:]).any()                   # monotone: never false and then true again
    assert d[:WINDOW + 1].all() and not d[WINDOW + 1:].any()
    assert np.array_equal(d, w <= G)


def test_edges_of_the_range():
    assert capi.grad_threshold(1.0, 0.0) == -1.0        # nothing passes, not even gn == 0
    assert capi.grad_threshold(1.0, -1.0) == -1.0
    assert capi.grad_threshold(1.0, np.inf) == np.finfo(np.float64).max     # every finite gn passes; +inf and NaN fail both forms
    assert capi.grad_threshold(1.0, 1e-300) == 0.0       # only gn == 0 passes
    Gs = capi.grad_threshold(1.0, 1e-160)                # a subnormal threshold: the bisection runs over bit patterns
    assert 0 < Gs < np.finfo(np.float64).tiny and D(1.0, 1e-160, Gs) and not D(1.0, 1e-160, np.nextafter(Gs, np.inf))
    G = capi.grad_threshold(1.0, 1.0)                    # sqrt(gn) < 1: the last double below 1
    assert G == np.nextafter(1.0, 0.0)
