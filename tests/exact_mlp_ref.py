"""Exact-arithmetic reference for the gradient kernels (ppo_a2c_grad, and the value net of ppo_grad).

An INTEGER problem: observations in {-2..2}, weights in {-1, 0, 1}, integer biases, actions, returns and advantages, IS weights
in {0, 1, 2}, logstd = 0 (std exactly 1), inv_count = 1, vf_coef = 1, ent_coef in {0, 1}.  Every product and every partial sum of the
forward and the backward pass is then an integer, so a float32 kernel whose partial sums stay below 2**24 in magnitude reproduces the
int64 result BIT FOR BIT -- whatever its summation order, tile split, slab count or reduction tree.  ``exact_grads`` returns, with
the gradients, the largest sum of absolute values over all reductions (|a| @ |b| of every matmul plus the bias, sum |.| of every
column sum): ``bound < 2**24`` is the condition for exactness (it bounds every partial sum of every order), not a tolerance.

Sparsity: the hidden-layer matrices have about 10 % nonzeros (at least about six per unit, so a 5-wide first layer is dense enough to
fire); the head matrices [64][nout] about three per hidden unit (nout = 1: all), so that nearly every hidden unit receives a delta.
Actions and returns are the net's own integer mean / value plus a small integer offset, which keeps the residuals -- and with them
every backward sum -- small.  Plain numpy, no GPU."""
import numpy as np

H = 64
EXACT_LIMIT = 2 ** 24


def _sparse(rng, shape, density):
    return (rng.randint(0, 2, shape) * 2 - 1) * (rng.uniform(size=shape) < density)


def make_problem(ob, ac, nb, seed):
    """Integer problem with ``nb`` data rows.  Returns a dict: params (13 float32 tensors in checkpoint order), obs [nb][ob], act
    [nb][ac], ret, adv, w [nb] -- all float32 holding integers; adv is per DATA row (gather it with idx for the kernel, which reads the
    advantage in minibatch order)."""
    rng = np.random.RandomState(seed)
    d0 = min(1.0, max(0.1, 6.0 / ob))
    dpi, dvf = min(1.0, max(0.1, 3.0 / ac)), 1.0
    p = [None] * 13
    for base in (0, 4):
        p[base] = _sparse(rng, (ob, H), d0)
        p[base + 1] = rng.randint(-1, 2, H)
        p[base + 2] = _sparse(rng, (H, H), 0.1)
        p[base + 3] = rng.randint(-1, 3, H)
    p[8], p[9] = _sparse(rng, (H, ac), dpi), rng.randint(-2, 3, ac)
    p[10] = np.zeros((1, ac), np.int64)
    p[11], p[12] = _sparse(rng, (H, 1), dvf), rng.randint(-2, 3, 1)
    p = [np.asarray(x, np.int64) for x in p]
    obs = rng.randint(-2, 3, (nb, ob)).astype(np.int64)
    mean, value, _ = _forward(p, obs)
    act = mean + rng.randint(-2, 3, (nb, ac))
    ret = value + rng.randint(-2, 3, nb)
    adv = rng.randint(-2, 3, nb)
    w = rng.randint(0, 3, nb)
    f = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    return dict(params=[f(x) for x in p], obs=f(obs), act=f(act), ret=f(ret), adv=f(adv), w=f(w))


def _forward(p, x):
    h1 = np.maximum(x @ p[0] + p[1], 0)
    h2 = np.maximum(h1 @ p[2] + p[3], 0)
    g1 = np.maximum(x @ p[4] + p[5], 0)
    g2 = np.maximum(g1 @ p[6] + p[7], 0)
    return h2 @ p[8] + p[9], (g2 @ p[11] + p[12])[:, 0], (h1, h2, g1, g2)


def _as_int(x):
    """float64 holding integers: numpy's float64 matmul is exact for them (every sum here is far below 2**53) and runs on BLAS."""
    a = np.asarray(x, np.float64)
    assert np.array_equal(np.rint(a), a), "exact_mlp_ref: inputs must hold integers"
    return a


class _Bound:
    def __init__(self):
        self.v = 0

    def mm(self, a, b, bias=None):
        s = np.abs(a) @ np.abs(b)
        if bias is not None:
            s = s + np.abs(bias)
        self.v = max(self.v, int(s.max()))
        return a @ b

    def colsum(self, a):
        self.v = max(self.v, int(np.abs(a).sum(0).max()))
        return a.sum(0)


def exact_grads(params, obs, act, adv, ret, w, ent_coef, weighted_value=True):
    """Gradient SUMS (inv_count = 1, vf_coef = 1) of the A2C loss over the given rows (already gathered, minibatch order), in exact integer arithmetic:
        sum_i w_i adv_i neglogp_i + sum_i 0.5 w_i (v_i - R_i)^2 - n ent_coef entropy          (weighted_value=True: ppo_a2c_grad)
    ``weighted_value=False`` drops w_i from the value term: the value net of ppo_grad.
    Returns (grads: 13 integer-valued float64 arrays in parameter shapes, dv [n] value residuals v - R, bound: int, frac: dict of the
    active fractions of the four hidden layers)."""
    p = [_as_int(x) for x in params]
    assert not p[10].any(), "logstd must be 0 (std exactly 1)"
    x, A, adv, R, w = (_as_int(v) for v in (obs, act, adv, ret, w))
    ent_coef = int(ent_coef)
    n = x.shape[0]
    B = _Bound()
    h1 = np.maximum(B.mm(x, p[0], p[1]) + p[1], 0)
    h2 = np.maximum(B.mm(h1, p[2], p[3]) + p[3], 0)
    g1 = np.maximum(B.mm(x, p[4], p[5]) + p[5], 0)
    g2 = np.maximum(B.mm(g1, p[6], p[7]) + p[7], 0)
    mean = B.mm(h2, p[8], p[9]) + p[9]
    value = (B.mm(g2, p[11], p[12]) + p[12])[:, 0]
    z = A - mean
    dnlp = w * adv
    dmean = dnlp[:, None] * (-z)
    g = [None] * 13
    g[8] = B.mm(h2.T, dmean)
    g[9] = B.colsum(dmean)
    B.colsum(np.abs(dnlp[:, None] * (1 - z * z)) + ent_coef)
    g[10] = (dnlp[:, None] * (1 - z * z) - ent_coef).sum(0, keepdims=True)
    dh2 = B.mm(dmean, p[8].T) * (h2 > 0)
    g[2] = B.mm(h1.T, dh2)
    g[3] = B.colsum(dh2)
    dh1 = B.mm(dh2, p[2].T) * (h1 > 0)
    g[0] = B.mm(x.T, dh1)
    g[1] = B.colsum(dh1)
    dv = value - R
    dvalue = (w * dv if weighted_value else dv)[:, None]
    g[11] = B.mm(g2.T, dvalue)
    g[12] = B.colsum(dvalue)
    dg2 = B.mm(dvalue, p[11].T) * (g2 > 0)
    g[6] = B.mm(g1.T, dg2)
    g[7] = B.colsum(dg2)
    dg1 = B.mm(dg2, p[6].T) * (g1 > 0)
    g[4] = B.mm(x.T, dg1)
    g[5] = B.colsum(dg1)
    B.v = max(B.v, int(np.abs(z * z).sum(1).max()), n)               # the row's sum of squares (neglogp), the row count
    frac = dict(h1=float((h1 > 0).mean()), h2=float((h2 > 0).mean()), g1=float((g1 > 0).mean()), g2=float((g2 > 0).mean()))
    return g, dv, B.v, frac


def flat(grads):
    """The 13 tensors as one float32 vector in checkpoint order (exact: every entry is an integer below 2**24)."""
    return np.concatenate([np.asarray(t, np.float64).ravel() for t in grads]).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# The cases of tests/test_gpu_grad_partition.py (built here so that tests/test_exact_mlp_ref_cpu.py checks the exactness condition and
# the coverage conditions on the very rows the GPU test uses).  (id, ob, ac, n, PPO_GRAD_BLOCKS or None, idx kind)
#   The gradient launch gives a net min(ceil(n / 16), cap) workgroups (cap = PPO_GRAD_BLOCKS, default 256); workgroup b walks the tiles
#   b, b + cap, ...; the reduction sums the slabs in G = ceil(workgroups / 16) groups of 16 and then the G partials 16 at a time.
# ---------------------------------------------------------------------------------------------------------------------------------
WIDTHS = [(5, 1), (121, 8), (128, 8), (165, 12), (176, 12), (209, 16), (224, 16)]   # every KT instantiation (8 / 11 / 14), D on and off 16
CASES = [("width-%d-%d" % (o, a), o, a, 117, 3, "perm") for (o, a) in WIDTHS]
CASES += [
    # tile loop: 117 rows = 7 full tiles + a 5-row tail; caps 1, 2, 3 -> workgroups of 8, 4 and 3/3/2 tiles (tail tile in an odd and an
    # even buffer); 112 rows under cap 7 = one full tile each, no tail; tiny batches (first tile is the tail tile)
    ("tiles-117-cap1", 121, 8, 117, 1, "perm"), ("tiles-117-cap2", 121, 8, 117, 2, "perm"), ("tiles-117-cap1-wide", 209, 16, 117, 1, "perm"),
    ("tiles-117-cap2-wide", 209, 16, 117, 2, "perm"), ("tiles-112-cap7", 121, 8, 112, 7, "perm"),
    ("tiny-1", 121, 8, 1, None, "perm"), ("tiny-15", 121, 8, 15, None, "perm"), ("tiny-16", 121, 8, 16, None, "perm"),
    ("tiny-17", 121, 8, 17, None, "perm"), ("tiny-1-wide", 209, 16, 1, None, "perm"),
    # slab reduction: 256 workgroups = a full 16-group pass; 258 tiles under the default cap (two workgroups take two tiles); the same
    # under cap 1024 = 258 workgroups, G = 17, second pass of the final loop; 17 workgroups = G 2 with a one-slab last group
    ("slab-g16", 121, 8, 16 * 256, None, "perm"), ("slab-two-tiles", 209, 16, 16 * 257 + 5, None, "perm"),
    ("slab-g17", 209, 16, 16 * 257 + 5, 1024, "perm"), ("slab-g17-ant", 121, 8, 16 * 257 + 5, 1024, "perm"),
    ("slab-g2", 121, 8, 16 * 16 + 5, None, "perm"),
    # gather: repeated rows; no idx at all (identity, dense rows)
    ("gather-repeat", 121, 8, 117, 3, "repeat"), ("gather-repeat-wide", 209, 16, 117, 2, "repeat"),
    ("identity", 121, 8, 117, 3, "identity"), ("identity-uncapped", 165, 12, 117, None, "identity"),
]
REUSE = [("reuse-4117", 209, 16, 16 * 257 + 5, None, "perm"), ("reuse-20", 209, 16, 20, None, "perm"), ("reuse-117-cap3", 209, 16, 117, 3, "perm")]
PROBLEM_ROWS = 4200
_PROBLEMS, _BUILT = {}, {}


def problem(ob, ac):
    if (ob, ac) not in _PROBLEMS:
        _PROBLEMS[(ob, ac)] = make_problem(ob, ac, PROBLEM_ROWS, seed=1000 * ob + ac)
    return _PROBLEMS[(ob, ac)]


def build_case(case):
    """The arrays of one case as the kernel is to see them, and the gathered rows for the reference.  Data arrays hold more rows than the
    minibatch uses; every unused row, the 7 padding columns of each observation row (obs_stride = ob + 7) and the tails of the
    minibatch-order arrays are NaN, and the entries of the idx buffer beyond n point at a NaN row: a stray read poisons the result
    instead of leaving the buffers.  kind 'identity': no idx, dense observation rows (obs_stride = ob).
    Returns dict(n, cap, ob, ac, obs_stride, obs, act, ret, w, old (an old neglogp near the row's own: ppo_grad needs one), idx (int32
    or None), adv_mb, rows=dict(obs, act, adv, ret, w) gathered in minibatch order).  Cached: do not modify."""
    if case in _BUILT:
        return _BUILT[case]
    name, ob, ac, n, cap, kind = case
    pr = problem(ob, ac)
    rng = np.random.RandomState((CASES + REUSE).index(case) + 77)
    if kind == "repeat":
        uniq = rng.permutation(PROBLEM_ROWS)[:n // 2 + 1]
        sel = uniq[rng.randint(0, len(uniq), n)]
    else:
        uniq = sel = rng.permutation(PROBLEM_ROWS)[:n]
    pad = 0 if kind == "identity" else 7
    nb = n + 3 if kind == "identity" else 2 * len(uniq) + 1
    pos = np.arange(len(uniq)) if kind == "identity" else rng.permutation(nb)[:len(uniq)]
    where = {int(r): int(q) for r, q in zip(uniq, pos)}
    idx = np.array([where[int(r)] for r in sel], np.int32)
    nan_row = int(np.setdiff1d(np.arange(nb), pos)[-1])
    d = dict(n=n, cap=cap, ob=ob, ac=ac, obs_stride=ob + pad)
    d["obs"] = np.full((nb, ob + pad), np.nan, np.float32)
    d["obs"][pos, :ob] = pr["obs"][uniq]
    for k, shape in (("act", (nb, ac)), ("ret", (nb,)), ("w", (nb,))):
        d[k] = np.full(shape, np.nan, np.float32)
        d[k][pos] = pr[k][uniq]
    d["rows"] = {k: pr[k][sel] for k in ("obs", "act", "adv", "ret", "w")}
    mean, _, _ = _forward([np.asarray(x, np.float64) for x in pr["params"]], pr["obs"][uniq].astype(np.float64))
    d["old"] = np.full(nb, np.nan, np.float32)
    d["old"][pos] = 0.5 * np.square(pr["act"][uniq] - mean).sum(1) + 0.5 * np.log(2.0 * np.pi) * ac
    d["adv_mb"] = np.concatenate([d["rows"]["adv"], np.full(16, np.nan, np.float32)])
    d["idx"] = None if kind == "identity" else np.concatenate([idx, np.full(48, nan_row, np.int32)])
    if kind != "identity":
        assert np.array_equal(d["obs"][idx, :ob], d["rows"]["obs"]) and np.array_equal(d["ret"][idx], d["rows"]["ret"])
    _BUILT[case] = d
    return d
