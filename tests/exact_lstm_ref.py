"""Exact-arithmetic references for the recurrent PPO training kernels (ppo_lstm_xproj, ppo_lstm_step_save(_z), ppo_lstm_seq_forward /
_backward, ppo_lstm_bwd_step, ppo_lstm_head_grad, ppo_lstm_wgrad); the companion of tests/exact_mlp_ref.py.  Plain numpy, no GPU.

The float64 restatements below (``forward_step``, ``head_rows``, ``bptt_sweep``, ``wgrad_ref``) are general: chained, they are the
gradient of oracle/ppo_oracle.lstm_ppo_loss_and_grads (tests/test_exact_lstm_ref_cpu.py).  Three constructions feed them inputs on which
a float32 kernel has no freedom left, and each comes with the CONDITION under which that holds:

(a) integer GEMM problems (``gemm_problem``; xproj and wgrad): observations, previous latents and deltas are integers in -2..2, wx in
    {-1, 0, 1}.  ``bound`` is the largest sum of absolute values over every reduction; with bound < 2**24 every partial sum of every
    summation order, chunk split and slab order is an exactly representable float32: bitwise equality.
(b) a dyadic BPTT problem (``bptt_problem``; bwd_step and seq_backward, which take the recorded gates as inputs): sigmoid gates in
    {0, 1/2, 1}, ug and tanhc in {-1, 0, 1} (optionally tanhc also +-1/2), cprev and dlatent integers in -2..2, mask in {0, 1}, wh in
    {-1, 0, 1} with about three nonzeros per row of wh^T.  Every value of the sweep is a dyadic rational.  ``bptt_sweep(track=True)``
    checks that every elementwise intermediate (in the kernels' order of operations) is a float32, and returns ``product`` = the maximum
    over the steps of (largest absolute-value sum of the contraction dz * wh^T) x (largest denominator in dz): with product < 2**24 every
    partial sum of the contraction, in any order and any split, is exact too.  Then the step kernel (four partial tiles) and the
    sequence kernel (one chain) must both equal the float64 sweep.
(c) a lattice forward problem (``lattice_problem``; one step of step_save / step_save_z): x, h, c integers in -2..2, wx / wh / b in
    {-1, 0, 1} / 8 at about 10 % density.  Every gate pre-activation is an exact multiple of 1/8 in float32 whatever the k order, so the
    only error of a correct kernel is that of expf / tanhf and the three or four operations after them, while a dropped, doubled or
    misplaced product moves a pre-activation by >= 1/8: a sigmoid by >= 4e-5 while |z + b| <= 8, a tanh by >= 1.6e-4 while |z + b| <= 4.
    ``marked`` flags the gate entries inside those ranges; the cap is that >= 90 % of each gate's entries are marked."""
import numpy as np

EXACT_LIMIT = 2 ** 24
STEP_TOL = 2.0 ** -20            # |got - ref| <= STEP_TOL + STEP_TOL |ref| for construction (c): 16 float32 ulp, 1/40 of the smallest lattice gap
MARK_CAP = 0.9


def _ternary(rng, shape, density):
    return ((rng.randint(0, 2, shape) * 2 - 1) * (rng.uniform(size=shape) < density)).astype(np.float64)


def _is_f32(x):
    x = np.asarray(x, np.float64)
    return bool(np.array_equal(x.astype(np.float32).astype(np.float64), x))


def f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 restatements
# ---------------------------------------------------------------------------------------------------------------------------------
def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def forward_step(wx, wh, b, x, c, h, mask):
    """One step of the baselines LSTM (a2c/utils.py:90-103), gate order i,f,o,u.  mask [n] or None.  Returns a dict: pre [n][4H]
    (z + b), gates [n][4H] (activated, the kernel's save_gates), cprev, hprev (masked), c, tanhc, h (the new state; h is the latent)."""
    wx, wh, b, x, c, h = (np.asarray(v, np.float64) for v in (wx, wh, b, x, c, h))
    H = wh.shape[0]
    keep = 1.0 if mask is None else (1.0 - np.asarray(mask, np.float64))[:, None]
    cp, hp = c * keep, h * keep
    pre = x @ wx + hp @ wh + b
    gates = np.concatenate([_sigmoid(pre[:, :3 * H]), np.tanh(pre[:, 3 * H:])], axis=1)
    cn = gates[:, H:2 * H] * cp + gates[:, :H] * gates[:, 3 * H:]
    tc = np.tanh(cn)
    return dict(pre=pre, gates=gates, cprev=cp, hprev=hp, c=cn, tanhc=tc, h=gates[:, 2 * H:3 * H] * tc)


class _Track:
    """checks that every intermediate handed to it is exactly a float32"""

    def __init__(self, on):
        self.on, self.ok = on, True

    def __call__(self, x):
        if self.on and not _is_f32(x):
            self.ok = False
        return x


def _denominator(x):
    """smallest power of two d with d * x all integers (x dyadic)"""
    d = 1.0
    for _ in range(80):
        if np.array_equal(np.rint(x * d), x * d):
            return d
        d *= 2.0
    raise AssertionError("exact_lstm_ref: not a dyadic array")


def bptt_sweep(wh, dlatent, mask, gates, cprev, tanhc, track=False):
    """BPTT from zero carries, t = T-1 down to 0, in the kernels' order of operations (ppo_lstm_bwd_step / ppo_lstm_seq_backward;
    oracle/ppo_oracle.lstm_ppo_loss_and_grads:422-433).  dlatent, cprev, tanhc [T][n][H], gates [T][n][4H], mask [T][n] or None.
    Returns dict(dz [T][n][4H], dh, dc [n][H] the carries left after t = 0, and with track=True: elementwise_exact (every intermediate
    is a float32) and product (see the module docstring))."""
    wh = np.asarray(wh, np.float64)
    dl, g, cpv, tcv = (np.asarray(v, np.float64) for v in (dlatent, gates, cprev, tanhc))
    T, n, H = dl.shape
    K = _Track(track)
    dz = np.zeros((T, n, 4 * H))
    dh, dc = np.zeros((n, H)), np.zeros((n, H))
    product = 0.0
    for t in range(T - 1, -1, -1):
        ig, fg, og, ug, tc, cp = g[t][:, :H], g[t][:, H:2 * H], g[t][:, 2 * H:3 * H], g[t][:, 3 * H:], tcv[t], cpv[t]
        keep = 1.0 if mask is None else (1.0 - np.asarray(mask[t], np.float64))[:, None]
        dht = K(dl[t] + dh)
        dct = K(dc + K(K(dht * og) * K(1.0 - K(tc * tc))))
        dzi = K(K(K(dct * ug) * ig) * K(1.0 - ig))
        dzf = K(K(K(dct * cp) * fg) * K(1.0 - fg))
        dzo = K(K(K(dht * tc) * og) * K(1.0 - og))
        dzu = K(K(dct * ig) * K(1.0 - K(ug * ug)))
        dc = K(K(dct * fg) * keep)
        dz[t] = np.concatenate([dzi, dzf, dzo, dzu], axis=1)
        if track:
            product = max(product, float((np.abs(dz[t]) @ np.abs(wh.T)).max()) * _denominator(dz[t]))
        dh = K((dz[t] @ wh.T) * keep)
    out = dict(dz=dz, dh=dh, dc=dc)
    if track:
        out.update(elementwise_exact=K.ok, product=product)
    return out


def wgrad_ref(x, hprev, dz, latent, dmean, dvalue, dlogstd_rows, logstd_shift):
    """The eight gradient tensors of ppo_lstm_wgrad in checkpoint order (wx, wh, b, pi/w, pi/b, logstd [1][A], vf/w [H][1], vf/b [1]):
    [x | hprev | 1]^T dz and [latent | 1]^T [dmean | dvalue | dlogstd_rows] (+ logstd_shift on logstd).  Returns (grads, bound) with bound
    the largest absolute-value sum over all these reductions (the shift included)."""
    x, hp, dz, L, dm, dv, dls = (np.asarray(v, np.float64) for v in (x, hprev, dz, latent, dmean, dvalue, dlogstd_rows))
    rows = x.shape[0]
    A1 = np.concatenate([x, hp, np.ones((rows, 1))], axis=1)
    A2 = np.concatenate([L, np.ones((rows, 1))], axis=1)
    B2 = np.concatenate([dm, dv.reshape(rows, 1), dls], axis=1)
    G1, G2 = A1.T @ dz, A2.T @ B2
    bound = max(float((np.abs(A1).T @ np.abs(dz)).max()), float((np.abs(A2).T @ np.abs(B2)).max()) + abs(float(logstd_shift)))
    D, H, A = x.shape[1], hp.shape[1], dm.shape[1]
    grads = [G1[:D], G1[D:D + H], G1[D + H], G2[:H, :A], G2[H, :A], (G2[H, A + 1:] + float(logstd_shift))[None, :], G2[:H, A:A + 1], G2[H, A:A + 1]]
    return grads, bound


def flat(grads):
    return np.concatenate([np.asarray(t, np.float64).ravel() for t in grads])


LOG2PI = np.log(2.0 * np.pi)


def head_forward(latent, pw, pb, logstd, vw, vb, actions):
    """mean, value and neglogp of the heads on stored latents, float64 (policies.py:50,70; distributions.py:238-241)"""
    L, pw, pb, ls, vw, vb, A_ = (np.asarray(v, np.float64) for v in (latent, pw, pb, logstd, vw, vb, actions))
    mean = L @ pw + pb.ravel()
    value = L @ vw.ravel() + vb.ravel()[0]
    zz = (A_ - mean) / np.exp(ls.ravel())
    return mean, value, 0.5 * np.sum(zz * zz, axis=1) + 0.5 * LOG2PI * A_.shape[1] + ls.sum(), zz


def head_rows(latent, pw, pb, logstd, vw, vb, actions, adv, returns, old, w, inv_count, cliprange, vf_coef):
    """Per-row restatement of the head part of oracle/ppo_oracle.lstm_ppo_loss_and_grads:393-419 (model.py:65-111): what
    ppo_lstm_head_grad writes.  Returns dict(dlatent [rows][H], dmean [rows][A], dvalue [rows], dlogstd_rows [rows][A], nlp [rows], ratio,
    stats = {0: sum w max(l1, l2), 1: sum 0.5 (v - R)^2, 3: sum (nlp - old), 4: clipped rows, 6: rows})."""
    pw, vw, ls = np.asarray(pw, np.float64), np.asarray(vw, np.float64), np.asarray(logstd, np.float64).ravel()
    adv, R, old, w = (np.asarray(v, np.float64) for v in (adv, returns, old, w))
    mean, value, nlp, zz = head_forward(latent, pw, pb, logstd, vw, vb, actions)
    with np.errstate(invalid="ignore"):
        ratio = np.exp(old - nlp)
    nanmask = np.isnan(ratio)
    ratio = np.where(nanmask, 2.0, ratio)                                 # model.py:96
    l1, l2 = -adv * ratio, -adv * np.clip(ratio, 1.0 - cliprange, 1.0 + cliprange)
    in_clip = (ratio >= 1.0 - cliprange) & (ratio <= 1.0 + cliprange)
    d_l1 = (l1 >= l2).astype(np.float64)                                  # tf.maximum: ties go to the first argument
    dratio = np.where(nanmask, 0.0, w * inv_count * (d_l1 * (-adv) + (1.0 - d_l1) * (-adv) * in_clip))
    dnlp = -dratio * ratio
    dmean = dnlp[:, None] * (-(zz / np.exp(ls)))
    dls = dnlp[:, None] * (1.0 - zz * zz)
    dvalue = vf_coef * (value - R) * inv_count
    dlat = dmean @ pw.T + dvalue[:, None] * vw.ravel()[None, :]
    stats = {0: float(np.sum(w * np.maximum(l1, l2))), 1: float(0.5 * np.sum(np.square(value - R))), 3: float(np.sum(nlp - old)),
             4: float(np.sum(np.abs(ratio - 1.0) > cliprange)), 6: float(len(adv))}
    return dict(dlatent=dlat, dmean=dmean, dvalue=dvalue, dlogstd_rows=dls, nlp=nlp, ratio=ratio, value=value, stats=stats)


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) integer GEMM problems
# ---------------------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def gemm_problem(rows, D, H, A, seed=0):
    """Integer operands of ppo_lstm_xproj / ppo_lstm_wgrad as float32 arrays: x [rows][D], hprev, latent [rows][H], dz [rows][4H], dmean,
    dlogstd_rows [rows][A], dvalue [rows], all in -2..2; wx [D][4H] in {-1, 0, 1} (half nonzero).  Cached: do not modify."""
    def make():
        rng = np.random.RandomState(7919 * seed + 31 * rows + 7 * D + 3 * H + A)
        ri = lambda *s: f32(rng.randint(-2, 3, s))
        return dict(rows=rows, D=D, H=H, A=A, x=ri(rows, D), hprev=ri(rows, H), latent=ri(rows, H), dz=ri(rows, 4 * H), dmean=ri(rows, A),
                    dlogstd_rows=ri(rows, A), dvalue=ri(rows), wx=f32(_ternary(rng, (D, 4 * H), 0.5)))
    return _cached(("gemm", rows, D, H, A, seed), make)


def xproj_ref(x, wx):
    """z = x * wx in float64 and the largest absolute-value sum"""
    x, wx = np.asarray(x, np.float64), np.asarray(wx, np.float64)
    return x @ wx, float((np.abs(x) @ np.abs(wx)).max())


def wgrad_case(rows, D, H, A, logstd_shift, seed=0):
    """(problem, flat float64 reference, bound) of one ppo_lstm_wgrad case.  Cached."""
    def make():
        p = gemm_problem(rows, D, H, A, seed)
        g, bound = wgrad_ref(p["x"], p["hprev"], p["dz"], p["latent"], p["dmean"], p["dvalue"], p["dlogstd_rows"], logstd_shift)
        return p, flat(g), bound
    return _cached(("wgrad", rows, D, H, A, logstd_shift, seed), make)


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) the dyadic BPTT problem
# ---------------------------------------------------------------------------------------------------------------------------------
MASK_KINDS = ("none", "zero", "one", "first", "last", "random")


def mask_pattern(kind, T, n, seed=0):
    """done flags [T][n] float32 (None for 'none'): all zero / all one / done only at t = 0 / only at t = T-1 / 30 % at random"""
    if kind == "none":
        return None
    m = np.zeros((T, n), np.float32)
    if kind == "one":
        m[:] = 1.0
    elif kind == "first":
        m[0] = 1.0
    elif kind == "last":
        m[T - 1] = 1.0
    elif kind == "random":
        m[:] = np.random.RandomState(1000 * T + n + seed).uniform(size=(T, n)) < 0.3
    else:
        assert kind == "zero", kind
    return m


def dz_tiles_nonzero(dz_t, H):
    """every (16-row tile, 16-unit tile) of one step's dz [n][4H] holds a nonzero entry (any of the unit tile's four gates)"""
    n = dz_t.shape[0]
    nz = (np.asarray(dz_t).reshape(n, 4, H // 16, 16) != 0).any(axis=(1, 3))          # [n][unit tile]
    return all(nz[r0:r0 + 16].any(axis=0).all() for r0 in range(0, n, 16))


def bptt_problem(T, n, H, mask_kind, half_tanhc=False):
    """The dyadic BPTT inputs and their tracked float64 sweep: dict(wh [H][4H], dlatent, cprev, tanhc [T][n][H], gates [T][n][4H], mask
    ([T][n] or None), all float32; ref = bptt_sweep(..., track=True)).  The seed is the first for which every (row tile, unit tile) of
    dz at t = 0 holds a nonzero entry (a condition on the reference, so that no tile is compared as all zeros).  Cached."""
    def make():
        for seed in range(64):
            rng = np.random.RandomState(100003 * seed + 1009 * T + 17 * n + H + (5 if half_tanhc else 0))
            sg = lambda: rng.randint(0, 3, (T, n, H)) * 0.5
            tern = lambda: rng.randint(-1, 2, (T, n, H)).astype(np.float64)
            p = dict(wh=f32(_ternary(rng, (H, 4 * H), 3.0 / H)),
                     gates=f32(np.concatenate([sg(), sg(), sg(), tern()], axis=2)),
                     cprev=f32(rng.randint(-2, 3, (T, n, H))), dlatent=f32(rng.randint(-2, 3, (T, n, H))),
                     tanhc=f32(rng.randint(-2, 3, (T, n, H)) * 0.5 if half_tanhc else tern()),
                     mask=mask_pattern(mask_kind, T, n))
            p["ref"] = bptt_sweep(p["wh"], p["dlatent"], p["mask"], p["gates"], p["cprev"], p["tanhc"], track=True)
            if dz_tiles_nonzero(p["ref"]["dz"][0], H):
                p["seed"] = seed
                return p
        raise AssertionError("exact_lstm_ref: no seed fills every dz tile at t = 0")
    return _cached(("bptt", T, n, H, mask_kind, half_tanhc), make)


BPTT_N = (1, 15, 16, 17, 33)
BPTT_T = (1, 2, 5, 8)


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) the lattice forward problem
# ---------------------------------------------------------------------------------------------------------------------------------
STEP_H = (64, 128)
STEP_D = (1, 4, 5, 13, 17, 29, 33, 121, 512)
STEP_N = (1, 15, 16, 17, 33)
STEP_MASKS = ("none", "zero", "one", "mixed")


def lattice_problem(D, H, n=33):
    """wx [D][4H], wh [H][4H], b [4H] in {-1, 0, 1} / 8 at 10 % density; x [n][D], c, h [n][H] integers in -2..2; mixed: a done-flag
    vector [n] with both values among its first rows.  float32 arrays.  Cached: do not modify."""
    def make():
        rng = np.random.RandomState(65537 + 131 * D + H)
        mixed = (rng.uniform(size=n) < 0.4).astype(np.float32)
        mixed[0], mixed[min(1, n - 1)] = 1.0, 0.0 if n > 1 else 1.0
        ri = lambda *s: f32(rng.randint(-2, 3, s))
        return dict(D=D, H=H, n=n, wx=f32(_ternary(rng, (D, 4 * H), 0.1) / 8), wh=f32(_ternary(rng, (H, 4 * H), 0.1) / 8),
                    b=f32(_ternary(rng, (4 * H,), 0.1) / 8), x=ri(n, D), c=ri(n, H), h=ri(n, H), mixed=mixed)
    return _cached(("lattice", D, H, n), make)


def lattice_mask(p, kind, n):
    if kind == "none":
        return None
    return {"zero": np.zeros(n, np.float32), "one": np.ones(n, np.float32), "mixed": p["mixed"][:n].copy()}[kind]


def lattice_step(D, H, n, mask_kind):
    """forward_step of the first n rows of lattice_problem(D, H) plus: marked [n][4H] bool (|pre| <= 8 for the sigmoid gates, <= 4 for the
    tanh gate), lattice (every pre-activation is a multiple of 1/8 and a float32).  Cached."""
    def make():
        p = lattice_problem(D, H)
        r = forward_step(p["wx"], p["wh"], p["b"], p["x"][:n], p["c"][:n], p["h"][:n], lattice_mask(p, mask_kind, n))
        lim = np.concatenate([np.full(3 * H, 8.0), np.full(H, 4.0)])
        r["marked"] = np.abs(r["pre"]) <= lim[None, :]
        r["lattice"] = bool(np.array_equal(np.rint(r["pre"] * 8), r["pre"] * 8)) and _is_f32(r["pre"])
        # the largest absolute-value sum of a pre-activation, in units of 1/8: below 2**24 every partial sum of every k order is exact
        hp = np.abs(r["hprev"])
        r["bound8"] = float((np.abs(p["x"][:n].astype(np.float64)) @ np.abs(p["wx"] * 8.0) + hp @ np.abs(p["wh"] * 8.0) + np.abs(p["b"] * 8.0)).max())
        return r
    return _cached(("lstep", D, H, n, mask_kind), make)


# ---------------------------------------------------------------------------------------------------------------------------------
# head problems
# ---------------------------------------------------------------------------------------------------------------------------------
HEAD_ROWS = (1, 127, 128, 129, 257)


def head_value_problem(rows, H, A):
    """Integer latents / head weights, logstd 0, adv 0, actions = mean + small integers, returns = value + small integers, old neglogp
    the row's own (to float32): with inv_count = vf_coef = 1 dmean and dlogstd_rows are exactly zero and dvalue = value - R,
    dlatent = dvalue x vf_w, stats[1] and stats[6] exact.  Returns dict of float32 arrays + value, dvalue, dlatent, stat1 (float64) and
    bound (largest absolute-value sum of the two head products and of dlatent)."""
    def make():
        rng = np.random.RandomState(4099 + 257 * rows + 3 * H + A)
        L = rng.randint(-2, 3, (rows, H)).astype(np.float64)
        pw, pb = _ternary(rng, (H, A), min(1.0, max(0.1, 3.0 / A))), rng.randint(-2, 3, A).astype(np.float64)
        vw, vb = _ternary(rng, (H, 1), 0.7), rng.randint(-2, 3, 1).astype(np.float64)
        mean, value = L @ pw + pb, (L @ vw)[:, 0] + vb[0]
        act = mean + rng.randint(-2, 3, (rows, A))
        R = value + rng.randint(-2, 3, rows)
        R[0] = value[0] + 1.0                                              # (row 0 always has a residual: rows = 1 is not a zero problem)
        nlp = 0.5 * np.square(act - mean).sum(1) + 0.5 * LOG2PI * A
        dv = value - R
        bound = max(float((np.abs(L) @ np.abs(pw) + np.abs(pb)).max()), float((np.abs(L) @ np.abs(vw)).max() + abs(vb[0])),
                    float(np.abs(dv).max()), float(0.5 * np.sum(dv * dv)))
        return dict(latent=f32(L), pw=f32(pw), pb=f32(pb), logstd=np.zeros((1, A), np.float32), vw=f32(vw), vb=f32(vb), act=f32(act), ret=f32(R),
                    old=f32(nlp), adv=np.zeros(rows, np.float32), w=f32(rng.randint(0, 3, rows)), value=value, dvalue=dv,
                    dlatent=dv[:, None] * vw[:, 0][None, :], stat1=float(0.5 * np.sum(dv * dv)), bound=bound)
    return _cached(("headv", rows, H, A), make)


BRANCH_RATIOS = (0.7, 0.79, 0.81, 1.0, 1.19, 1.21, 1.5)


def head_branch_problem(rows, H, A, with_nan, cliprange=0.2):
    """Real-valued head problem whose rows sit on each side of both clip bounds for advantages of either sign, with adv = 0, w = 0 and
    (with_nan) NaN old-neglogp rows, inv_count = 1 / (3 rows).  The old neglogp is placed around the float64 neglogp of a clean forward:
    old = nlp + log(target ratio), the targets 1e-2 away from the bounds 1 -+ cliprange (float32 moves a ratio by 1e-6).  Returns dict of
    float32 inputs + kind (per-row label) + ref = head_rows(...) on the float32 inputs."""
    def make():
        rng = np.random.RandomState(977 + 13 * rows + H + A + (1 if with_nan else 0))
        L = rng.normal(0, 0.5, (rows, H))
        pw, pb = rng.normal(0, 0.15, (H, A)), rng.normal(0, 0.1, A)
        vw, vb = rng.normal(0, 0.15, (H, 1)), rng.normal(0, 0.1, 1)
        ls = rng.normal(-0.3, 0.1, (1, A))
        d = dict(latent=f32(L), pw=f32(pw), pb=f32(pb), logstd=f32(ls), vw=f32(vw), vb=f32(vb))
        mean, value, _, _ = head_forward(d["latent"], d["pw"], d["pb"], d["logstd"], d["vw"], d["vb"], np.zeros((rows, A)))
        d["act"] = f32(mean + np.exp(d["logstd"].astype(np.float64)) * rng.normal(0, 0.8, (rows, A)))
        d["ret"] = f32(value + rng.normal(0, 1, rows))
        nlp = head_forward(d["latent"], d["pw"], d["pb"], d["logstd"], d["vw"], d["vb"], d["act"])[2]
        k = np.arange(rows)
        target = np.asarray(BRANCH_RATIOS)[k % len(BRANCH_RATIOS)]
        adv = np.where((k // len(BRANCH_RATIOS)) % 2 == 0, 1.0, -1.0) * rng.uniform(0.5, 1.5, rows)
        w = rng.uniform(0.5, 1.5, rows)
        kind = np.array(["r%.2f%s" % (t, "+" if a > 0 else "-") for t, a in zip(target, adv)], dtype=object)
        special = rng.permutation(rows)
        for j, r in enumerate(special[:max(1, rows // 6)]):                # adv = 0, w = 0 and NaN rows, spread over the blocks
            which = j % (3 if with_nan else 2)
            if which == 0:
                adv[r], kind[r] = 0.0, "adv0"
            elif which == 1:
                w[r], kind[r] = 0.0, "w0"
            else:
                kind[r] = "nan"
        old = nlp + np.log(target)
        old[kind == "nan"] = np.nan
        d.update(adv=f32(adv), w=f32(w), old=f32(old), kind=kind, inv_count=1.0 / (3.0 * rows), cliprange=cliprange, vf_coef=0.5)
        d["ref"] = head_rows(d["latent"], d["pw"], d["pb"], d["logstd"], d["vw"], d["vb"], d["act"], d["adv"], d["ret"], d["old"], d["w"],
                             d["inv_count"], float(np.float32(cliprange)), d["vf_coef"])
        return d
    return _cached(("headb", rows, H, A, with_nan, cliprange), make)


# ---------------------------------------------------------------------------------------------------------------------------------
# the shapes of tests/test_gpu_lstm_kernel_edges.py (listed here so that tests/test_exact_lstm_ref_cpu.py checks the conditions on them)
# ---------------------------------------------------------------------------------------------------------------------------------
XPROJ_H = (64, 128)
XPROJ_D = (1, 3, 4, 5, 8, 9, 121, 512)
XPROJ_ROWS = (1, 15, 16, 17, 33)
WGRAD_ROWS = (1, 7, 8, 9, 16, 17, 255, 256, 257, 513, 16384, 16385, 16400)
WGRAD_WIDTHS = ((1, 64), (63, 64), (64, 64), (127, 128), (128, 128), (112, 128), (512, 128))
WGRAD_A = (1, 8, 16)
WGRAD_CASES = [(r, 121, 128, 8, (0.0, -0.5)[i % 2]) for i, r in enumerate(WGRAD_ROWS)]
WGRAD_CASES += [(257, D, H, A, (-0.5, 0.0)[(i + j) % 2]) for i, (D, H) in enumerate(WGRAD_WIDTHS) for j, A in enumerate(WGRAD_A)]
WGRAD_REUSE = [(16400, 121, 128, 8, -0.5), (9, 121, 128, 8, 0.0), (16385, 121, 128, 8, 0.0)]        # large, small, large on one workspace
HEAD_H = (64, 128)
HEAD_A = (1, 8, 16)
