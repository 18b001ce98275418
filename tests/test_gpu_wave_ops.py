"""The in-wave primitives of the engine kernels (csrc/sumo_engine.hip: wave_sum, wave_sum2 / wave_sum4 / wave_sum_n<6>, pair_swap_f64,
wave_excl_scan) and the two forms of the Newton loop's gradient test, on one wave of caller-given lanes (sumo_debug_wave_ops).

The sums run on DPP moves with bound_ctrl on and every row enabled; only lane 63 is read.  Expected value: the six stages in numpy
float64 -- in-row shifts by 1, 2, 4, 8 with zero fill, then lane 31 += lane 15 and lane 63 += lane 47 (both from the values before the
stage), then lane 63 += lane 31 -- compared bit for bit; the 2-, 4- and 6-fold forms against the single form; the pair swap against
x[i ^ 1]; the scan against cumsum in every lane.  The gradient test: the device's ``scale * sqrt(gn) < tol`` against ``gn <= G`` (G from
the host bisection, test_grad_threshold_cpu.py) around G, at the ends of the range and on 10 000 log-uniform values: the threshold
form rests on the device's sqrt rounding as IEEE's does, which is what this checks."""
import numpy as np
import pytest

from conftest import has_gpu
from robosumo_selfplay_amd import mjcf

pytestmark = pytest.mark.gpu

if has_gpu():
    from robosumo_selfplay_amd import capi

ANT, ANT_BUG, SPIDER = "RoboSumo-Ant-vs-Ant-v0", "RoboSumo-Ant-vs-Bug-v0", "RoboSumo-Spider-vs-Spider-v0"
WINDOW = 512


@pytest.fixture(scope="module")
def eng():
    e = capi.Engine(mjcf.load_model(ANT), 1)
    yield e
    e.close()


def emulated_sum(x):
    """lane 63 after the six stages, float64 adds in the kernel's order"""
    v = np.array(x, np.float64)
    pos = np.arange(64) % 16
    with np.errstate(invalid="ignore", over="ignore"):
        for sh in (1, 2, 4, 8):
            src = np.where(pos >= sh, np.roll(v, sh), 0.0)      # row_shr: a lane without a source in its row reads 0
            v = v + src
        t31, t63 = v[31] + v[15], v[63] + v[47]                # row_bcast:15, the lanes lane 63 depends on
        return t63 + t31                                        # row_bcast:31


def double_rows():
    rng = np.random.default_rng(11)
    rows = {"normal": rng.standard_normal(64),
            "mixed": rng.choice([-1.0, 1.0], 64) * 10.0 ** rng.uniform(-200, 200, 64),
            "zeros": np.zeros(64), "negzero": np.full(64, -0.0)}
    for l in (0, 31, 47, 63):
        r = np.zeros(64); r[l] = 1.0 + rng.random()
        rows["only%d" % l] = r
    for name, val in (("nan", np.nan), ("inf", np.inf)):
        r = rng.standard_normal(64); r[int(rng.integers(64))] = val
        rows[name] = r
    return rows


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def test_wave_sums_bit_for_bit(eng):
    rows = double_rows()
    names = list(rows)
    assert len(names) == 10
    ints = np.zeros(64, np.int32)
    for first in (0, 2):      # two launches of eight rows: rows 0 .. 7, then rows 2 .. 9 (every row passes through the n-fold forms' slots)
        block = np.stack([rows[n] for n in names[first:first + 8]])
        sums, swapped, _, _, _ = eng.debug_wave_ops(block, ints)
        want = np.array([emulated_sum(r) for r in block])
        for k in range(8):
            print("%-8s single %r expected %r" % (names[first + k], sums[k], want[k]))
        assert np.array_equal(bits(sums[:8]), bits(want))
        assert np.array_equal(bits(sums[8:10]), bits(sums[0:2]))        # wave_sum2
        assert np.array_equal(bits(sums[10:14]), bits(sums[0:4]))       # wave_sum4
        assert np.array_equal(bits(sums[14:20]), bits(sums[0:6]))       # wave_sum_n<6>
        assert np.array_equal(bits(swapped), bits(block[0][np.arange(64) ^ 1]))
    # the sum of the normal row is also the plain sum to rounding (the emulation itself is the kernel's order, not the value's check)
    assert abs(emulated_sum(rows["normal"]) - rows["normal"].sum()) < 1e-13


@pytest.mark.parametrize("row", ["normal", "mixed", "negzero", "nan", "inf"])
def test_pair_swap(eng, row):
    r = double_rows()[row]
    block = np.zeros((8, 64)); block[0] = r
    _, swapped, _, _, _ = eng.debug_wave_ops(block, np.zeros(64, np.int32))
    assert np.array_equal(bits(swapped), bits(r[np.arange(64) ^ 1]))


@pytest.mark.parametrize("kind", ["random", "zeros", "threes"])
def test_exclusive_scan(eng, kind):
    v = {"random": np.random.default_rng(3).integers(0, 4, 64), "zeros": np.zeros(64), "threes": np.full(64, 3)}[kind].astype(np.int32)
    _, _, scan, total, _ = eng.debug_wave_ops(np.zeros((8, 64)), v)
    assert np.array_equal(scan, np.cumsum(v) - v) and total == int(v.sum())


def _scale_tol(env_id):
    m = mjcf.load_model(env_id)
    nv = int(m.nv)
    return 1.0 / (float(m.opt[5]) * (nv if nv > 1 else 1)), float(m.opt[4])


GRAD_CASES = [(ANT, None), (ANT_BUG, None), (SPIDER, None), (ANT, 1e-4), (ANT, 1e-1)]


@pytest.mark.parametrize("env_id,tol_override", GRAD_CASES)
def test_gradient_test_forms_agree(eng, env_id, tol_override):
    scale, tol = _scale_tol(env_id)
    if tol_override is not None:
        tol = tol_override
    G = capi.grad_threshold(scale, tol)
    assert G > 0
    around = (np.float64(G).view(np.uint64) + np.arange(-WINDOW, WINDOW + 1, dtype=np.int64).astype(np.uint64)).view(np.float64)
    edge = np.array([0.0, np.nextafter(0.0, 1.0), 1e-320, np.inf, np.nan])
    logu = 10.0 ** np.random.default_rng(5).uniform(-30, 30, 10000)
    gn = np.concatenate([around, edge, logu])
    grad = eng.debug_wave_ops(np.zeros((8, 64)), np.zeros(64, np.int32), gn, scale, tol)[4]
    assert grad.shape == (len(gn), 2)
    differ = np.flatnonzero(grad[:, 0] != grad[:, 1])
    print("%s tol %g: G %r, %d of %d inputs pass, %d differ" % (env_id, tol, G, int(grad[:, 0].sum()), len(gn), len(differ)))
    assert len(differ) == 0, gn[differ][:8]
    # and both are what the host says: true up to G, false above, false for +inf and NaN
    with np.errstate(invalid="ignore"):
        assert np.array_equal(grad[:, 1], gn <= G)
    assert grad[:WINDOW + 1, 0].all() and not grad[WINDOW + 1:2 * WINDOW + 1, 0].any()
    assert grad[2 * WINDOW + 1:2 * WINDOW + 4, 0].all() and not grad[2 * WINDOW + 4:2 * WINDOW + 6, 0].any()
