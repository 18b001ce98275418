"""The eight recurrent PPO training kernels at their tile, chunk and mask edges, through the C ABI (every buffer, stride and row count is
the test's own) against tests/exact_lstm_ref.py:

  * ppo_lstm_xproj and ppo_lstm_wgrad on integer problems (bound < 2**24): bitwise, whatever the k pipeline, chunk split or slab order;
  * ppo_lstm_bwd_step and ppo_lstm_seq_backward on the dyadic BPTT problem: both bitwise equal to the float64 sweep;
  * one step of ppo_lstm_step_save / xproj + step_save_z on the lattice problem: the two paths bit for bit, and within 2**-20 (absolute
    plus relative: 16 float32 ulp, a fortieth of the smallest lattice gap) of float64 -- a dropped, doubled or misplaced product moves a
    pre-activation by an eighth, forty times the bound;
  * ppo_lstm_seq_forward against T calls of ppo_lstm_step_save_z, bit for bit, over the done-flag patterns;
  * ppo_lstm_head_grad: the value path exactly, the clip branches per row against the float64 restatement of the oracle's head part;
  * argument errors: negative code, text, nothing launched.

Output buffers carry guard rows (and pad columns where a stride leaves a gap) prefilled with NaN, input buffers NaN in every gap and
behind their last row: guards and gaps must be unchanged afterwards, data rows finite.  The conditions that make the comparisons exact
are asserted on this file's very shapes by tests/test_exact_lstm_ref_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import exact_lstm_ref as X
from conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch
    from robosumo_selfplay_amd import ppo_capi
    from robosumo_selfplay_amd.ppo_capi import LstmNet, fill_lstm_net_ifou

    DEV = torch.device("cuda:0")

GUARD = 3
NAN = float("nan")


def _up(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


def _in(x, pad=0):
    """input rows [rows][cols] as a device buffer [rows + GUARD][cols + pad] whose gaps and guard rows are NaN"""
    x = np.asarray(x, np.float32)
    x2 = x.reshape(x.shape[0], -1)
    buf = np.full((x2.shape[0] + GUARD, x2.shape[1] + pad), np.nan, np.float32)
    buf[:x2.shape[0], :x2.shape[1]] = x2
    return _up(buf)


def _out(rows, cols):
    return torch.full((rows + GUARD, cols), NAN, dtype=torch.float32, device=DEV)


def _take(buf, rows, cols=None):
    """the data part of an output / state buffer; guard rows and pad columns must still be NaN, the data finite"""
    a = buf.cpu().numpy()
    cols = a.shape[1] if cols is None else cols
    assert np.isnan(a[rows:]).all() and np.isnan(a[:, cols:]).all(), "guard rows / pad columns were written"
    d = a[:rows, :cols]
    assert np.isfinite(d).all(), "non-finite data rows"
    return d


def _net(D, H, A, wx=None, wh=None, b=None, pw=None, pb=None, logstd=None, vw=None, vb=None):
    """(LstmNet, keep-alive list).  Tensors not given are small zero buffers of the right size (never read by the kernel under test)."""
    shapes = [(D, 4 * H), (H, 4 * H), (4 * H,), (H, A), (A,), (1, A), (H, 1), (1,)]
    ts = [(_up(v) if v is not None else torch.zeros(int(np.prod(s)), dtype=torch.float32, device=DEV)) for v, s in
          zip((wx, wh, b, pw, pb, logstd, vw, vb), shapes)]
    assert all(t.data_ptr() % 16 == 0 for t in ts)
    return fill_lstm_net_ifou(LstmNet(), D, A, H, [t.data_ptr() for t in ts]), ts


def _close(got, ref, what):
    err = np.abs(got.astype(np.float64) - ref)
    lim = X.STEP_TOL + X.STEP_TOL * np.abs(ref)
    assert (err <= lim).all(), (what, float(err.max()), int((err > lim).sum()))
    return float((err / lim).max()) if err.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# ppo_lstm_xproj: integer GEMM, exact
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", X.XPROJ_H)
@pytest.mark.parametrize("D", X.XPROJ_D)
def test_xproj_integer_exact(D, H):
    """the two-stage pipeline (odd / even / single k-step counts), tail row tiles, padded observation rows"""
    L = ppo_capi.lib()
    p = X.gemm_problem(max(X.XPROJ_ROWS), D, H, 1)
    net, keep = _net(D, H, 1, wx=p["wx"])
    for rows in X.XPROJ_ROWS:
        ref, bound = X.xproj_ref(p["x"][:rows], p["wx"])
        assert bound < X.EXACT_LIMIT
        for pad in (0, 3):
            obs, z = _in(p["x"][:rows], pad), _out(rows, 4 * H)
            ppo_capi.chk(L.ppo_lstm_xproj(C.byref(net), obs.data_ptr(), rows, D + pad, z.data_ptr(), None))
            torch.cuda.synchronize()
            got = _take(z, rows)
            assert np.array_equal(got, ref.astype(np.float32)), (D, H, rows, pad, int((got != ref).sum()))


# ---------------------------------------------------------------------------------------------------------------------------------
# one forward step on the lattice problem
# ---------------------------------------------------------------------------------------------------------------------------------
def _state(c, h, H, stride):
    """(buffer(s), c pointer, h pointer) for a state stride of H (separate dense buffers), 2H (c | h interleaved) or 2H + 3 (NaN gap)"""
    if stride == H:
        cb, hb = _in(c), _in(h)
        return (cb, hb), cb.data_ptr(), hb.data_ptr()
    S = _in(np.concatenate([c, h], axis=1), stride - 2 * H)
    return (S,), S.data_ptr(), S.data_ptr() + 4 * H


def _read_state(bufs, n, H):
    if len(bufs) == 2:
        return _take(bufs[0], n), _take(bufs[1], n)
    S = _take(bufs[0], n, 2 * H)
    return S[:, :H], S[:, H:]


@pytest.mark.parametrize("H", X.STEP_H)
@pytest.mark.parametrize("D", X.STEP_D)
def test_single_step_lattice(D, H):
    """ppo_lstm_step_save from the observations and ppo_lstm_xproj + ppo_lstm_step_save_z: equal bit for bit in state and records, and
    within 2**-20 + 2**-20 |ref| of the float64 step on the marked gate entries, cprev, hprev, c, tanhc, h and latent_out.  D runs the
    weight ring through every residue of the chunk count modulo 3 with full and partial last chunks; n through tail tiles."""
    L = ppo_capi.lib()
    p = X.lattice_problem(D, H)
    net, keep = _net(D, H, 1, wx=p["wx"], wh=p["wh"], b=p["b"])
    worst = 0.0
    for n in X.STEP_N:
        obs = _in(p["x"][:n], 3)
        for mk in X.STEP_MASKS:
            ref = X.lattice_step(D, H, n, mk)
            m = X.lattice_mask(p, mk, n)
            mbuf = None if m is None else _in(m[:, None])
            for stride in (H, 2 * H, 2 * H + 3):
                res = []
                for path in ("obs", "z"):
                    sb, cptr, hptr = _state(p["c"][:n], p["h"][:n], H, stride)
                    rec = [_out(n, 4 * H), _out(n, H), _out(n, H), _out(n, H)]
                    lat = _out(n, H)
                    if path == "obs":
                        ppo_capi.chk(L.ppo_lstm_step_save(C.byref(net), obs.data_ptr(), n, D + 3, ppo_capi.ptr(mbuf), cptr, hptr, stride,
                                                          *[r.data_ptr() for r in rec], None))
                    else:
                        z = _out(n, 4 * H)
                        ppo_capi.chk(L.ppo_lstm_xproj(C.byref(net), obs.data_ptr(), n, D + 3, z.data_ptr(), None))
                        ppo_capi.chk(L.ppo_lstm_step_save_z(C.byref(net), z.data_ptr(), n, ppo_capi.ptr(mbuf), cptr, hptr, stride,
                                                            *[r.data_ptr() for r in rec], lat.data_ptr(), None))
                    torch.cuda.synchronize()
                    c, h = _read_state(sb, n, H)
                    res.append(dict(c=c, h=h, gates=_take(rec[0], n), cprev=_take(rec[1], n), hprev=_take(rec[2], n), tanhc=_take(rec[3], n),
                                    lat=_take(lat, n) if path == "z" else None))
                a, b = res
                for k in ("c", "h", "gates", "cprev", "hprev", "tanhc"):
                    assert np.array_equal(a[k], b[k]), (D, H, n, mk, stride, k, "the two paths differ")
                assert np.array_equal(b["lat"], b["h"])
                assert np.array_equal(a["cprev"], ref["cprev"].astype(np.float32)) and np.array_equal(a["hprev"], ref["hprev"].astype(np.float32))
                tag = (D, H, n, mk, stride)
                mk_ = ref["marked"]
                worst = max(worst, _close(a["gates"][mk_], ref["gates"][mk_], tag + ("gates",)), _close(a["c"], ref["c"], tag + ("c",)),
                            _close(a["tanhc"], ref["tanhc"], tag + ("tanhc",)), _close(a["h"], ref["h"], tag + ("h",)))
    print("single step D=%d H=%d: largest error / bound = %.3f" % (D, H, worst))


# ---------------------------------------------------------------------------------------------------------------------------------
# ppo_lstm_seq_forward against T calls of ppo_lstm_step_save_z
# ---------------------------------------------------------------------------------------------------------------------------------
_SEQ = {}


def _seq_problem():
    """random normal weights as tests/test_gpu_lstm_train.py uses; D = 13; z0 of the longest sequence of the widest batch, per (T, n) a
    slice of the observations"""
    if not _SEQ:
        rng = np.random.RandomState(11)
        D, H = 13, 128
        _SEQ.update(D=D, H=H, wx=rng.normal(0, 0.3, (D, 4 * H)), wh=rng.normal(0, 0.1, (H, 4 * H)), b=rng.normal(0, 0.1, 4 * H),
                    obs=rng.normal(0, 1, (8, 33, D)), S0=rng.normal(0, 0.5, (33, 2 * H)))
        _SEQ["net"], _SEQ["keep"] = _net(D, H, 1, wx=_SEQ["wx"], wh=_SEQ["wh"], b=_SEQ["b"])
    return _SEQ


@pytest.mark.parametrize("n", X.BPTT_N)
def test_seq_forward_equals_step_calls(n):
    L = ppo_capi.lib()
    q = _seq_problem()
    D, H, net = q["D"], q["H"], q["net"]
    for T in (1, 2, 3, 8):
        obs = _in(q["obs"][:T, :n].reshape(T * n, D))
        z0 = _out(T * n, 4 * H)
        ppo_capi.chk(L.ppo_lstm_xproj(C.byref(net), obs.data_ptr(), T * n, D, z0.data_ptr(), None))
        for mk in X.MASK_KINDS:
            m = X.mask_pattern(mk, T, n)
            mbuf = None if m is None else _in(m.reshape(T * n, 1))
            for stride in (256, 259):
                out = {}
                for mode in ("seq", "step"):
                    sb, cptr, hptr = _state(q["S0"][:n, :H], q["S0"][:n, H:], H, stride)
                    rec = [_out(T * n, 4 * H), _out(T * n, H), _out(T * n, H), _out(T * n, H), _out(T * n, H)]
                    if mode == "seq":
                        ppo_capi.chk(L.ppo_lstm_seq_forward(C.byref(net), z0.data_ptr(), T, n, ppo_capi.ptr(mbuf), cptr, hptr, stride,
                                                            *[r.data_ptr() for r in rec], None))
                    else:
                        for t in range(T):
                            o4, o1 = 4 * t * n * 4 * H, 4 * t * n * H
                            ppo_capi.chk(L.ppo_lstm_step_save_z(C.byref(net), z0.data_ptr() + o4, n, None if m is None else mbuf.data_ptr() + 4 * t * n,
                                                                cptr, hptr, stride, rec[0].data_ptr() + o4, rec[1].data_ptr() + o1,
                                                                rec[2].data_ptr() + o1, rec[3].data_ptr() + o1, rec[4].data_ptr() + o1, None))
                    torch.cuda.synchronize()
                    out[mode] = _read_state(sb, n, H) + tuple(_take(r, T * n) for r in rec)
                names = ("c", "h", "gates", "cprev", "hprev", "tanhc", "latent")
                for k, a, b in zip(names, out["seq"], out["step"]):
                    assert np.array_equal(a, b), (n, T, mk, stride, k, int((a != b).sum()))
                cprev, hprev = (out["seq"][i].reshape(T, n, H) for i in (3, 4))
                lat = out["seq"][6].reshape(T, n, H)
                assert np.array_equal(out["seq"][1], lat[T - 1])
                assert lat.any(axis=2).all()
                if mk == "one":                  # every step starts from a zeroed state, step 0 included (its flag applies to the incoming state)
                    assert not cprev.any() and not hprev.any()
                elif mk in ("none", "zero"):
                    assert np.array_equal(hprev[0], q["S0"][:n, H:].astype(np.float32)) and np.array_equal(hprev[1:], lat[:-1])
                elif mk in ("first", "last"):
                    k = 0 if mk == "first" else T - 1
                    assert not hprev[k].any() and not cprev[k].any()
                    for t in range(T):
                        if t != k:
                            assert hprev[t].any(axis=1).all() and cprev[t].any(axis=1).all(), (mk, T, t)
                    if k > 0:
                        assert np.array_equal(hprev[k - 1], lat[k - 2] if k > 1 else q["S0"][:n, H:].astype(np.float32))
                else:
                    keep = (1.0 - m).astype(np.float32)[:, :, None]
                    prev = np.concatenate([q["S0"][None, :n, H:].astype(np.float32), lat[:-1]])
                    assert np.array_equal(hprev, prev * keep)


# ---------------------------------------------------------------------------------------------------------------------------------
# BPTT on the dyadic problem: exact
# ---------------------------------------------------------------------------------------------------------------------------------
def _bptt_inputs(p, T, n, H):
    net, keep = _net(1, H, 1, wh=p["wh"])
    bufs = dict(dl=_in(p["dlatent"].reshape(T * n, H)), g=_in(p["gates"].reshape(T * n, 4 * H)), cp=_in(p["cprev"].reshape(T * n, H)),
                tc=_in(p["tanhc"].reshape(T * n, H)), m=None if p["mask"] is None else _in(p["mask"].reshape(T * n, 1)))
    return net, keep, bufs


@pytest.mark.parametrize("H", (64, 128))
@pytest.mark.parametrize("n", X.BPTT_N)
def test_bwd_step_dyadic_exact(n, H):
    """T calls from t = T-1 down: dz of every step and the dh / dc carries left after t = 0 equal the float64 sweep bit for bit (the four
    per-wave partial tiles, summed through the LDS tile they overwrite, are exact partial sums)"""
    L = ppo_capi.lib()
    for T in X.BPTT_T:
        for mk in X.MASK_KINDS:
            p = X.bptt_problem(T, n, H, mk)
            ref = p["ref"]
            assert ref["elementwise_exact"] and ref["product"] < X.EXACT_LIMIT and X.dz_tiles_nonzero(ref["dz"][0], H)
            net, keep, b = _bptt_inputs(p, T, n, H)
            dh, dc = _in(np.zeros((n, H))), _in(np.zeros((n, H)))
            dz = _out(T * n, 4 * H)
            for t in range(T - 1, -1, -1):
                o4, o1 = 4 * t * n * 4 * H, 4 * t * n * H
                ppo_capi.chk(L.ppo_lstm_bwd_step(C.byref(net), n, b["dl"].data_ptr() + o1, None if b["m"] is None else b["m"].data_ptr() + 4 * t * n,
                                                 b["g"].data_ptr() + o4, b["cp"].data_ptr() + o1, b["tc"].data_ptr() + o1, dh.data_ptr(),
                                                 dc.data_ptr(), dz.data_ptr() + o4, None))
            torch.cuda.synchronize()
            got = _take(dz, T * n).reshape(T, n, 4 * H)
            for t in range(T - 1, -1, -1):
                assert np.array_equal(got[t], ref["dz"][t].astype(np.float32)), (n, H, T, mk, t, int((got[t] != ref["dz"][t]).sum()))
            assert np.array_equal(_take(dh, n), ref["dh"].astype(np.float32)), (n, H, T, mk, "dh carry")
            assert np.array_equal(_take(dc, n), ref["dc"].astype(np.float32)), (n, H, T, mk, "dc carry")


@pytest.mark.parametrize("n", X.BPTT_N)
def test_seq_backward_dyadic_exact(n):
    """the one-launch sweep (one chain per output tile, double-buffered delta tile, prefetched next step) equals the float64 sweep -- and
    with it the step kernel -- bit for bit"""
    L = ppo_capi.lib()
    H = 128
    for T in X.BPTT_T:
        for mk in X.MASK_KINDS:
            p = X.bptt_problem(T, n, H, mk)
            ref = p["ref"]
            assert ref["elementwise_exact"] and ref["product"] < X.EXACT_LIMIT and X.dz_tiles_nonzero(ref["dz"][0], H)
            net, keep, b = _bptt_inputs(p, T, n, H)
            dz = _out(T * n, 4 * H)
            ppo_capi.chk(L.ppo_lstm_seq_backward(C.byref(net), T, n, b["dl"].data_ptr(), ppo_capi.ptr(b["m"]), b["g"].data_ptr(), b["cp"].data_ptr(),
                                                 b["tc"].data_ptr(), dz.data_ptr(), None))
            torch.cuda.synchronize()
            got = _take(dz, T * n).reshape(T, n, 4 * H)
            for t in range(T - 1, -1, -1):
                assert np.array_equal(got[t], ref["dz"][t].astype(np.float32)), (n, T, mk, t, int((got[t] != ref["dz"][t]).sum()))


# ---------------------------------------------------------------------------------------------------------------------------------
# ppo_lstm_wgrad: integer GEMM, exact
# ---------------------------------------------------------------------------------------------------------------------------------
_WS = {}


def _workspace():
    """ONE workspace for the module, sized for the widest case and filled with NaN once: the kernel must write every slab entry the
    reduction reads, whatever an earlier (larger or smaller) launch left there"""
    if "buf" not in _WS:
        nbytes = max(ppo_capi.lib().ppo_lstm_wgrad_workspace_bytes(D, H, A) for (_, D, H, A, _) in X.WGRAD_CASES)
        _WS["buf"] = torch.full((nbytes // 4,), NAN, dtype=torch.float32, device=DEV)
    return _WS["buf"]


def _run_wgrad(case):
    rows, D, H, A, shift = case
    L = ppo_capi.lib()
    p, ref, bound = X.wgrad_case(*case)
    assert bound < X.EXACT_LIMIT
    ws = _workspace()
    assert L.ppo_lstm_wgrad_workspace_bytes(D, H, A) <= ws.numel() * 4
    net, keep = _net(D, H, A)
    ins = [_in(p[k]) for k in ("x", "hprev", "dz", "latent", "dmean")] + [_in(p["dvalue"][:, None]), _in(p["dlogstd_rows"])]
    g = torch.full((ref.size + 8,), NAN, dtype=torch.float32, device=DEV)
    ppo_capi.chk(L.ppo_lstm_wgrad(C.byref(net), rows, *[t.data_ptr() for t in ins], float(shift), g.data_ptr(), ws.data_ptr(), None))
    torch.cuda.synchronize()
    got = g.cpu().numpy()
    assert np.isnan(got[ref.size:]).all(), "the guard behind the last gradient entry was written"
    assert np.isfinite(got[:ref.size]).all()
    return got[:ref.size], ref.astype(np.float32)


def _assert_wgrad(case, got, ref):
    rows, D, H, A, _ = case
    o, names = 0, ("wx", "wh", "b", "pi/w", "pi/b", "logstd", "vf/w", "vf/b")
    for name, size in zip(names, (D * 4 * H, H * 4 * H, 4 * H, H * A, A, A, H, 1)):
        assert np.array_equal(got[o:o + size], ref[o:o + size]), (case, name, int((got[o:o + size] != ref[o:o + size]).sum()))
        o += size
    assert o == ref.size


@pytest.mark.parametrize("case", X.WGRAD_CASES, ids=["r%d-D%d-H%d-A%d" % c[:4] for c in X.WGRAD_CASES])
def test_wgrad_integer_exact(case):
    """all eight gradient tensors in checkpoint order.  rows: one trip, the guarded second trip, the 8-row rounding of a chunk, 2 chunks,
    the 64-chunk cap (16384 rows = 64 x 256; 16385 and 16400 = 64 chunks of 264 with a short last one resp. 63 chunks).  Widths: the ones
    column on either side of a 64 / 256 column boundary (D + H = 127, 128, 255, 256: the first column of a new blockIdx.y), three y blocks
    (D = 512), head problems padded to 32 and 64 columns (A = 1, 8, 16)."""
    got, ref = _run_wgrad(case)
    _assert_wgrad(case, got, ref)


def test_wgrad_workspace_reuse_and_repeat():
    """one NaN-prefilled workspace through a large, a small and again a large launch; then one case twice: identical bits"""
    for case in X.WGRAD_REUSE:
        got, ref = _run_wgrad(case)
        _assert_wgrad(case, got, ref)
    a, _ = _run_wgrad(X.WGRAD_CASES[9])
    b, _ = _run_wgrad(X.WGRAD_CASES[9])
    assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------------------
# ppo_lstm_head_grad
# ---------------------------------------------------------------------------------------------------------------------------------
SENT = (-7.0, 11.0, 13.0)          # sentinels in the stats slots 2, 5, 7 the kernel must not touch


def _run_head(d, rows, H, A, inv_count, cliprange, vf_coef, calls=1):
    L = ppo_capi.lib()
    net, keep = _net(1, H, A, pw=d["pw"], pb=d["pb"], logstd=d["logstd"], vw=d["vw"], vb=d["vb"])
    ins = [_in(d["latent"])] + [_in(d[k].reshape(rows, -1)) for k in ("act", "adv", "ret", "old", "w")]
    outs = [_out(rows, H), _out(rows, A), _out(rows, 1), _out(rows, A)]
    st = torch.zeros(8, dtype=torch.float64, device=DEV)
    st[2], st[5], st[7] = SENT
    for _ in range(calls):
        ppo_capi.chk(L.ppo_lstm_head_grad(C.byref(net), ins[0].data_ptr(), rows, *[t.data_ptr() for t in ins[1:]], float(inv_count),
                                          float(cliprange), float(vf_coef), *[t.data_ptr() for t in outs], st.data_ptr(), None))
    torch.cuda.synchronize()
    a = [t.cpu().numpy() for t in outs]
    for t in a:
        assert np.isnan(t[rows:]).all() and np.isfinite(t[:rows]).all()
    s = st.cpu().numpy()
    assert tuple(s[[2, 5, 7]]) == SENT
    return a[0][:rows], a[1][:rows], a[2][:rows, 0], a[3][:rows], s


@pytest.mark.parametrize("H", X.HEAD_H)
@pytest.mark.parametrize("A", X.HEAD_A)
def test_head_grad_value_path_exact(A, H):
    """integer latents and head weights, logstd 0, adv 0, inv_count = vf_coef = 1: dmean and dlogstd_rows exactly zero, dvalue,
    dlatent = dvalue x vf_w, stats[1] and stats[6] exact; the block's last rows (rows = 1, 127, 129, 257) add zeros to the reduction"""
    for rows in X.HEAD_ROWS:
        p = X.head_value_problem(rows, H, A)
        assert p["bound"] < X.EXACT_LIMIT
        dlat, dmean, dvalue, dls, s = _run_head(p, rows, H, A, 1.0, 0.2, 1.0)
        assert not dmean.any() and not dls.any(), (rows, H, A)
        assert np.array_equal(dvalue, p["dvalue"].astype(np.float32)) and np.array_equal(dlat, p["dlatent"].astype(np.float32)), (rows, H, A)
        assert s[1] == p["stat1"] and s[6] == rows and s[4] == 0 and s[0] == 0


def _rowwise(got, ref, what):
    ref2 = ref.reshape(ref.shape[0], -1)
    lim = 3e-4 * np.abs(ref2).max(axis=1, keepdims=True) + 1e-7
    err = np.abs(got.reshape(ref2.shape).astype(np.float64) - ref2)
    assert (err <= lim).all(), (what, float((err / lim).max()), int((err > lim).any(axis=1).sum()))


@pytest.mark.parametrize("with_nan", (False, True), ids=("finite", "nan-old"))
@pytest.mark.parametrize("H,A", [(64, 1), (64, 8), (128, 8), (128, 16)])
def test_head_grad_branches_per_row(H, A, with_nan):
    """rows on each side of both clip bounds for either sign of the advantage, adv = 0, w = 0, NaN old neglogp, inv_count = 1 / (3 rows):
    every row within 3e-4 of ITS OWN largest reference entry (+ 1e-7), statistics at the tolerances of test_bptt_gradients_match_oracle"""
    rows = 257
    d = X.head_branch_problem(rows, H, A, with_nan)
    ref = d["ref"]
    dlat, dmean, dvalue, dls, s = _run_head(d, rows, H, A, d["inv_count"], d["cliprange"], d["vf_coef"])
    _rowwise(dlat, ref["dlatent"], "dlatent")
    _rowwise(dmean, ref["dmean"], "dmean")
    _rowwise(dls, ref["dlogstd_rows"], "dlogstd_rows")
    _rowwise(dvalue, ref["dvalue"], "dvalue")
    for kind in ("adv0", "w0") + (("nan",) if with_nan else ()):
        sel = d["kind"] == kind
        assert sel.any() and not dmean[sel].any() and not dls[sel].any(), kind
    rs = ref["stats"]
    assert s[6] == rows and s[4] == rs[4]
    assert np.allclose([s[0] / rows, s[1] / rows], [rs[0] / rows, rs[1] / rows], rtol=2e-4, atol=2e-5)
    assert np.isnan(s[3]) == np.isnan(rs[3]) == with_nan
    if with_nan:
        assert s[4] >= (d["kind"] == "nan").sum()                            # a NaN row has ratio 2: counted as clipped
    else:
        assert np.allclose(s[3] / rows, rs[3] / rows, rtol=2e-4, atol=2e-5)


def test_head_grad_accumulates_into_stats():
    d = X.head_branch_problem(257, 128, 8, False)
    one = _run_head(d, 257, 128, 8, d["inv_count"], d["cliprange"], d["vf_coef"])
    two = _run_head(d, 257, 128, 8, d["inv_count"], d["cliprange"], d["vf_coef"], calls=2)
    for k in (0, 1, 3, 4, 6):
        assert two[4][k] == pytest.approx(2.0 * one[4][k], rel=1e-12), k      # (float64 atomics over three blocks: order may differ)
    assert two[4][6] == 514 and two[4][4] == 2 * one[4][4]
    for a, b in zip(one[:4], two[:4]):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------------------
# argument errors: negative code, text, nothing launched
# ---------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_before_any_launch():
    L = ppo_capi.lib()
    D, H, A, n, T = 8, 128, 4, 4, 2
    net, keep = _net(D, H, A)
    bufs = {k: torch.full((T * n + GUARD, 4 * H + 8), NAN, dtype=torch.float32, device=DEV) for k in "abcdefghij"}
    st = torch.zeros(8, dtype=torch.float64, device=DEV)
    ws = _workspace()
    P = lambda k: bufs[k].data_ptr()

    def variant(**kw):
        v = LstmNet()
        C.memmove(C.byref(v), C.byref(net), C.sizeof(LstmNet))
        for k, val in kw.items():
            setattr(v, k, val)
        return v

    def step(v, n_=n, os_=D, ss=2 * H):
        return L.ppo_lstm_step_save(C.byref(v), P("a"), n_, os_, None, P("b"), P("c"), ss, P("d"), P("e"), P("f"), P("g"), None)

    def stepz(v, n_=n, ss=2 * H):
        return L.ppo_lstm_step_save_z(C.byref(v), P("a"), n_, None, P("b"), P("c"), ss, P("d"), P("e"), P("f"), P("g"), P("h"), None)

    def xproj(v, rows=n, os_=D):
        return L.ppo_lstm_xproj(C.byref(v), P("a"), rows, os_, P("b"), None)

    def bwd(v, n_=n):
        return L.ppo_lstm_bwd_step(C.byref(v), n_, P("a"), None, P("b"), P("c"), P("d"), P("e"), P("f"), P("g"), None)

    def seqf(v, T_=T, n_=n, ss=2 * H):
        return L.ppo_lstm_seq_forward(C.byref(v), P("a"), T_, n_, None, P("b"), P("c"), ss, P("d"), P("e"), P("f"), P("g"), P("h"), None)

    def seqb(v, T_=T, n_=n):
        return L.ppo_lstm_seq_backward(C.byref(v), T_, n_, P("a"), None, P("b"), P("c"), P("d"), P("e"), None)

    def wgrad(v, rows=n):
        return L.ppo_lstm_wgrad(C.byref(v), rows, P("a"), P("b"), P("c"), P("d"), P("e"), P("f"), P("g"), 0.0, P("h"), ws.data_ptr(), None)

    def head(v, rows=n):
        return L.ppo_lstm_head_grad(C.byref(v), P("a"), rows, P("b"), P("c"), P("d"), P("e"), P("f"), 1.0, 0.2, 0.5, P("g"), P("h"), P("i"), P("j"),
                                    st.data_ptr(), None)

    h96, h64, ijfo = variant(hidden=96), variant(hidden=64), variant(gate_order=ppo_capi.LSTM_GATES_IJFO)
    filt = variant(obs_mean=P("i"), obs_invstd=P("j"))
    cases = [("step hidden 96", step(h96), -2), ("step_z hidden 96", stepz(h96), -2), ("xproj hidden 96", xproj(h96), -2),
             ("bwd_step hidden 96", bwd(h96), -3), ("seq_forward hidden 96", seqf(h96), -2), ("seq_backward hidden 96", seqb(h96), -2),
             ("seq_forward hidden 64", seqf(h64), -2), ("seq_backward hidden 64", seqb(h64), -2),
             ("bwd_step IJFO", bwd(ijfo), -2), ("seq_forward IJFO", seqf(ijfo), -2), ("seq_backward IJFO", seqb(ijfo), -2),
             ("step state_stride", step(net, ss=H - 1), -8), ("step_z state_stride", stepz(net, ss=H - 1), -8),
             ("seq_forward state_stride", seqf(net, ss=H - 1), -1),
             ("step obs_stride", step(net, os_=D - 1), -3), ("xproj obs_stride", xproj(net, os_=D - 1), -3),
             ("step_z with filter", stepz(filt), -10),
             ("step n 0", step(net, n_=0), -1), ("step_z n -1", stepz(net, n_=-1), -1), ("xproj rows 0", xproj(net, rows=0), -1),
             ("bwd_step n 0", bwd(net, n_=0), -1), ("seq_forward n 0", seqf(net, n_=0), -1), ("seq_forward T 0", seqf(net, T_=0), -1),
             ("seq_backward n 0", seqb(net, n_=0), -1), ("seq_backward T -1", seqb(net, T_=-1), -1),
             ("wgrad rows 0", wgrad(net, rows=0), -1), ("head_grad rows 0", head(net, rows=0), -1),
             ("wgrad hidden 96", wgrad(h96), -3), ("wgrad hidden 32", wgrad(variant(hidden=32)), -3),
             ("wgrad ob_dim 0", wgrad(variant(ob_dim=0)), -4), ("wgrad ob_dim 513", wgrad(variant(ob_dim=513)), -4),
             ("wgrad ac_dim 0", wgrad(variant(ac_dim=0)), -5), ("wgrad ac_dim 17", wgrad(variant(ac_dim=17)), -5)]
    # (the return codes were collected one by one above; the text belongs to the last failing call: check it per call below)
    for name, rc, want in cases:
        assert rc == want, (name, rc, want)
    for call in (lambda: step(h96), lambda: seqf(h64), lambda: bwd(ijfo), lambda: wgrad(variant(ac_dim=17)), lambda: stepz(filt),
                 lambda: xproj(net, os_=D - 1), lambda: step(net, ss=H - 1), lambda: head(net, rows=0)):
        assert call() < 0 and len(L.ppo_last_error()) > 0
    assert b"17" in (wgrad(variant(ac_dim=17)), L.ppo_last_error())[1] and b"96" in (wgrad(h96), L.ppo_last_error())[1]
    torch.cuda.synchronize()
    for k, t in bufs.items():
        assert bool(torch.isnan(t).all()), "an argument error wrote to buffer " + k
    assert not st.any()
