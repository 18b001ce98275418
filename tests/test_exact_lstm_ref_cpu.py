"""CPU checks of tests/exact_lstm_ref.py, the reference of tests/test_gpu_lstm_kernel_edges.py: its float64 restatements chained are the
gradient of oracle/ppo_oracle.lstm_ppo_loss_and_grads, its forward step is lstm_step_baselines, and every shape the GPU test runs
satisfies the exactness / cap condition of its construction, so that no GPU test can silently run outside them."""
import numpy as np
import pytest

import exact_lstm_ref as X
from oracle import ppo_oracle as po


def _chain(T, n, D, H, A, with_nan, seed):
    """a real-valued recurrent PPO problem through forward_step -> head_rows -> bptt_sweep -> wgrad_ref, and through the oracle"""
    rng = np.random.RandomState(seed)
    params = [rng.normal(0, 0.3, s) for s in ((D, 4 * H), (H, 4 * H), (4 * H,), (H, A), (A,), (1, A), (H, 1), (1,))]
    params[5] = rng.normal(-0.3, 0.1, (1, A))
    obs, masks = rng.normal(0, 1, (T, n, D)), (rng.uniform(size=(T, n)) < 0.3).astype(np.float64)
    S0 = rng.normal(0, 0.5, (n, 2 * H))
    c, h, rec = S0[:, :H], S0[:, H:], []
    for t in range(T):
        r = X.forward_step(params[0], params[1], params[2], obs[t], c, h, masks[t])
        c, h = r["c"], r["h"]
        rec.append(r)
    N = T * n
    lat = np.concatenate([r["h"] for r in rec])
    act = rng.normal(0, 0.7, (N, A))
    nlp = X.head_forward(lat, params[3], params[4], params[5], params[6], params[7], act)[2]
    old = nlp + rng.normal(0, 0.25, N)
    if with_nan:
        old[::5] = np.nan
    adv, ret, w = rng.normal(0, 1, N), rng.normal(0, 1, N), rng.uniform(0.5, 1.5, N)
    adv[1], w[2] = 0.0, 0.0
    hd = X.head_rows(lat, params[3], params[4], params[5], params[6], params[7], act, adv, ret, old, w, 1.0 / N, 0.2, 0.5)
    stack = lambda k: np.stack([r[k] for r in rec])
    sw = X.bptt_sweep(params[1], hd["dlatent"].reshape(T, n, H), masks, stack("gates"), stack("cprev"), stack("tanhc"))
    g, _ = X.wgrad_ref(obs.reshape(N, D), stack("hprev").reshape(N, H), sw["dz"].reshape(N, 4 * H), lat, hd["dmean"], hd["dvalue"],
                       hd["dlogstd_rows"], -0.01)
    tn = lambda v: v.reshape(T, n, *v.shape[1:])
    with np.errstate(invalid="ignore"):
        _, stats, go, Sf = po.lstm_ppo_loss_and_grads(params, obs, masks, tn(act), tn(adv), tn(ret), tn(old), tn(w), S0, 0.2, 0.01, 0.5)
    return g, hd, go, stats, Sf, np.concatenate([c, h], axis=1), N


@pytest.mark.parametrize("T,n,D,H,A,with_nan", [(4, 5, 7, 16, 3, False), (3, 6, 5, 32, 2, True), (1, 3, 4, 16, 1, False)])
def test_restatements_chain_to_the_oracle_gradient(T, n, D, H, A, with_nan):
    g, hd, go, stats, Sf, S_mine, N = _chain(T, n, D, H, A, with_nan, seed=T + n)
    for k, (a, b) in enumerate(zip(g, go)):
        b = np.asarray(b).reshape(a.shape)
        assert np.abs(a - b).max() <= 1e-11 * max(1.0, np.abs(b).max()), k
    assert np.allclose(S_mine, Sf, rtol=0, atol=1e-13)
    s = hd["stats"]
    assert s[0] / N == pytest.approx(stats[0], rel=1e-11) and s[1] / N == pytest.approx(stats[1], rel=1e-11)
    assert s[4] / N == pytest.approx(stats[4], rel=1e-12) and s[6] == N
    assert np.isnan(s[3]) == np.isnan(stats[3]) == with_nan
    if not with_nan:
        assert s[3] / N == pytest.approx(stats[3], rel=1e-9, abs=1e-12)
    else:                                                                   # model.py:96: NaN rows push nothing into the policy head
        assert not hd["dmean"][::5].any() and not hd["dlogstd_rows"][::5].any() and hd["dmean"][1::5].any()


@pytest.mark.parametrize("H", X.STEP_H)
@pytest.mark.parametrize("D", X.STEP_D)
def test_lattice_steps_are_exact_and_inside_the_cap(D, H):
    """(c) at every shape of the GPU test: pre-activations are multiples of 1/8 and float32, the absolute-sum bound (in eighths) is below
    2**24, at least 90 % of each gate's entries are marked, and the step is the oracle's (float32, 2e-6)."""
    p = X.lattice_problem(D, H)
    for v in (p["wx"], p["wh"], p["b"]):
        assert np.array_equal(np.rint(v * 8), v * 8) and np.abs(v * 8).max() <= 1 and (v != 0).sum() >= 4
        assert v.size < 2000 or 0.07 < (v != 0).mean() < 0.13
    assert p["mixed"][0] == 1 and p["mixed"][1] == 0
    for n in X.STEP_N:
        for mk in X.STEP_MASKS:
            r = X.lattice_step(D, H, n, mk)
            assert r["lattice"] and r["bound8"] < X.EXACT_LIMIT
            for g in range(4):
                assert r["marked"][:, g * H:(g + 1) * H].mean() >= X.MARK_CAP, (n, mk, g)
            m = X.lattice_mask(p, mk, n)
            lat, S = po.lstm_step_baselines(p["wx"], p["wh"], p["b"], p["x"][:n], np.concatenate([p["c"][:n], p["h"][:n]], axis=1), m)
            assert np.abs(S[:, :H] - r["c"]).max() < 2e-6 * 4 and np.abs(lat - r["h"]).max() < 2e-6 and np.abs(S[:, H:] - r["h"]).max() < 2e-6
            if mk == "one":
                assert not r["cprev"].any() and not r["hprev"].any()
            if mk in ("none", "zero"):
                assert np.array_equal(r["cprev"], p["c"][:n]) and np.array_equal(r["hprev"], p["h"][:n])
    # the lattice gap the tolerance is measured against: one eighth moves a sigmoid by >= 4e-5 inside |z| <= 8, a tanh by >= 1.6e-4 inside 4
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    assert sig(8.0) - sig(7.875) > 4e-5 and np.tanh(4.0) - np.tanh(3.875) > 1.6e-4 and X.STEP_TOL * 2 < 4e-5 / 16


def _perm_contract(dz, whT, perm):
    """dz [n][K] x whT [K][H] accumulated in float32 over k in the order `perm`"""
    acc = np.zeros((dz.shape[0], whT.shape[1]), np.float32)
    for k in perm:
        acc = (acc + dz[:, k:k + 1] * whT[k][None, :]).astype(np.float32)
    return acc


@pytest.mark.parametrize("H", (64, 128))
@pytest.mark.parametrize("n", X.BPTT_N)
def test_dyadic_bptt_cases_are_exact(n, H):
    """(b) at every shape of the GPU test: every elementwise intermediate is a float32, (absolute-sum of the contraction) x (largest
    denominator of dz) < 2**24 at every step, every (row tile, unit tile) of dz at t = 0 holds a nonzero entry."""
    for T in X.BPTT_T:
        for mk in X.MASK_KINDS:
            p = X.bptt_problem(T, n, H, mk)
            r = p["ref"]
            assert r["elementwise_exact"] and r["product"] < X.EXACT_LIMIT, (T, mk, r["product"])
            assert X.dz_tiles_nonzero(r["dz"][0], H)
            assert X._is_f32(r["dz"]) and X._is_f32(r["dh"]) and X._is_f32(r["dc"])
            if p["mask"] is not None and p["mask"][0].all():                # done at t = 0: nothing flows out of the sequence
                assert not r["dh"].any() and not r["dc"].any()
            elif n >= 15:
                assert r["dh"].any() and r["dc"].any()
            assert (np.abs(p["wh"]) != 0).sum(0).mean() == pytest.approx(3.0, abs=0.6)       # about three nonzeros per row of wh^T


def test_dyadic_bptt_with_half_tanhc_holds_to_five_steps_only():
    """with tanhc also taking +-1/2 the denominators grow a step sooner: exact to T = 5, not to T = 6 -- hence the ternary set, which the
    GPU test runs to T = 8"""
    p = X.bptt_problem(5, 17, 128, "random", half_tanhc=True)
    assert p["ref"]["elementwise_exact"] and p["ref"]["product"] < X.EXACT_LIMIT
    assert X.bptt_problem(6, 17, 128, "random", half_tanhc=True)["ref"]["product"] >= X.EXACT_LIMIT


@pytest.mark.parametrize("T,n,H,mk", [(8, 17, 128, "random"), (5, 33, 64, "zero"), (8, 16, 128, "none")])
def test_permuted_float32_bptt_gives_the_same_bits(T, n, H, mk):
    """the whole sweep in float32 with the contraction summed in a shuffled k order, and split in four partial sums as the step kernel
    does: the bits of the float64 sweep"""
    p = X.bptt_problem(T, n, H, mk)
    ref = p["ref"]
    rng = np.random.RandomState(5)
    whT = np.ascontiguousarray(p["wh"].T)
    one = np.float32(1.0)
    for split in (1, 4):
        dh, dc = np.zeros((n, H), np.float32), np.zeros((n, H), np.float32)
        for t in range(T - 1, -1, -1):
            g = p["gates"][t]
            ig, fg, og, ug, tc, cp = g[:, :H], g[:, H:2 * H], g[:, 2 * H:3 * H], g[:, 3 * H:], p["tanhc"][t], p["cprev"][t]
            keep = one if p["mask"] is None else (one - p["mask"][t])[:, None]
            dht = p["dlatent"][t] + dh
            dct = dc + dht * og * (one - tc * tc)
            dz = np.concatenate([dct * ug * ig * (one - ig), dct * cp * fg * (one - fg), dht * tc * og * (one - og), dct * ig * (one - ug * ug)], axis=1)
            assert dz.dtype == np.float32 and np.array_equal(dz, ref["dz"][t])
            dc = dct * fg * keep
            parts = [_perm_contract(dz, whT, q) for q in np.array_split(rng.permutation(4 * H), split)]
            acc = parts[0]
            for q in parts[1:]:
                acc = acc + q
            dh = acc * keep
        assert dh.dtype == np.float32 and np.array_equal(dh, ref["dh"]) and np.array_equal(dc, ref["dc"])


def test_gemm_cases_are_exact():
    """(a) at every shape of the GPU test: bound < 2**24 (at 16400 rows with entries in -2..2 it is at most 65600), integer results"""
    for H in X.XPROJ_H:
        for D in X.XPROJ_D:
            p = X.gemm_problem(max(X.XPROJ_ROWS), D, H, 1)
            z, bound = X.xproj_ref(p["x"], p["wx"])
            assert bound < X.EXACT_LIMIT and np.array_equal(np.rint(z), z) and (z.any() or D == 1)
            assert (p["wx"] != 0).any()
    for case in X.WGRAD_CASES + X.WGRAD_REUSE:
        p, ref, bound = X.wgrad_case(*case)
        assert bound <= 4 * case[0] + 0.5 and bound < X.EXACT_LIMIT
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref) and np.array_equal(np.rint(2 * ref), 2 * ref)
        rows, D, H, A, _ = case
        assert ref.size == (D + H + 1) * 4 * H + H * A + 2 * A + H + 1
        if rows >= 7:
            assert (ref != 0).mean() > 0.5
    for H in X.HEAD_H:
        for A in X.HEAD_A:
            for rows in X.HEAD_ROWS:
                p = X.head_value_problem(rows, H, A)
                assert p["bound"] < X.EXACT_LIMIT and p["dvalue"][0] != 0 and X._is_f32(p["dlatent"])
                hd = X.head_rows(p["latent"], p["pw"], p["pb"], p["logstd"], p["vw"], p["vb"], p["act"], p["adv"], p["ret"], p["old"], p["w"],
                                 1.0, 0.2, 1.0)
                assert not hd["dmean"].any() and not hd["dlogstd_rows"].any()
                assert np.array_equal(hd["dvalue"], p["dvalue"]) and np.array_equal(hd["dlatent"], p["dlatent"]) and hd["stats"][1] == p["stat1"]


@pytest.mark.parametrize("rows,D,H,A", [(513, 5, 64, 3), (257, 64, 64, 16)])
def test_permuted_float32_gemm_gives_the_same_bits(rows, D, H, A):
    """(a) in float32, rows summed in a shuffled order and in chunks whose slabs are added afterwards: the bits of the float64 matmul"""
    p, ref, bound = X.wgrad_case(rows, D, H, A, -0.5)
    rng = np.random.RandomState(3)
    A1 = np.concatenate([p["x"], p["hprev"], np.ones((rows, 1), np.float32)], axis=1)
    A2 = np.concatenate([p["latent"], np.ones((rows, 1), np.float32)], axis=1)
    B2 = np.concatenate([p["dmean"], p["dvalue"][:, None], p["dlogstd_rows"]], axis=1)
    outs = []
    for Am, Bm in ((A1, p["dz"]), (A2, B2)):
        slabs = []
        for chunk in np.array_split(rng.permutation(rows), 5):
            acc = np.zeros((Am.shape[1], Bm.shape[1]), np.float32)
            for r in chunk:
                acc = acc + Am[r][:, None] * Bm[r][None, :]
            slabs.append(acc)
        tot = slabs[0]
        for s in slabs[1:]:
            tot = tot + s
        assert tot.dtype == np.float32
        outs.append(tot)
    G1, G2 = outs
    G2[H, A + 1:] += np.float32(-0.5)
    mine = np.concatenate([G1.ravel(), G2[:H, :A].ravel(), G2[H, :A], G2[H, A + 1:], G2[:H, A], G2[H, A:A + 1]])
    assert np.array_equal(mine.astype(np.float64), ref)
    z, zb = X.xproj_ref(p["x"], p["wx"])
    acc = np.zeros_like(z, dtype=np.float32)
    for k in rng.permutation(D):
        acc = acc + p["x"][:, k:k + 1] * p["wx"][k][None, :]
    assert acc.dtype == np.float32 and np.array_equal(acc, z) and zb < X.EXACT_LIMIT


@pytest.mark.parametrize("with_nan", (False, True))
def test_head_branch_rows_cover_both_sides_of_both_bounds(with_nan):
    for H in X.HEAD_H:
        for A in X.HEAD_A:
            d = X.head_branch_problem(257, H, A, with_nan)
            kinds = set(d["kind"])
            need = {"r%.2f%s" % (t, s) for t in X.BRANCH_RATIOS for s in "+-"} | {"adv0", "w0"} | ({"nan"} if with_nan else set())
            assert need <= kinds, need - kinds
            ref, reg = d["ref"], np.array([k.startswith("r") for k in d["kind"]])
            # the float64 ratios sit where they were placed: 1e-2 from the bounds, float32 rounding of `old` moves them by 1e-6
            tgt = np.array([float(k[1:5]) for k in d["kind"][reg]])
            assert np.abs(ref["ratio"][reg] - tgt).max() < 1e-5 and np.abs(np.abs(ref["ratio"][reg] - 1.0) - 0.2).min() > 5e-3
            # the clipped side of each bound gets no policy gradient, the other side does
            pos = np.array([k.endswith("+") for k in d["kind"]])
            dead = reg & ((pos & (ref["ratio"] > 1.2)) | (~pos & (ref["ratio"] < 0.8)))
            assert dead.any() and not ref["dmean"][dead].any() and ref["dmean"][reg & ~dead].any(axis=1).all()
            assert np.isnan(ref["stats"][3]) == with_nan
            if with_nan:
                nanr = d["kind"] == "nan"
                assert nanr.sum() >= 10 and not ref["dmean"][nanr].any() and not ref["dlogstd_rows"][nanr].any() and ref["dvalue"][nanr].all()
