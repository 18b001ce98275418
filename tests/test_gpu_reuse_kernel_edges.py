"""The three masked recurrent-update entries (ppo_adv_moments_masked_ws, ppo_adv_normalize_masked, ppo_lstm_head_grad_masked) at
their chunk, block and mask edges, through the C ABI, against their unmasked counterparts:

  * every row valid: the bits of the unmasked entries;
  * a random mask: the bits of the unmasked entries run on the valid rows alone wherever the summation order is the same (per-row
    outputs always; the moments while the minibatch is one 4096-row chunk), otherwise float64 numpy sums of the very terms within
    n * 2**-52 * sum |term| -- n additions, each rounded to at most half an ulp of a partial sum that is at most sum |term|;
  * no valid row: zeros, nothing non-finite, no statistic touched.

The per-row terms of the head statistics are the unmasked kernel's own: one launch per row on zeroed statistics leaves 0 + term."""
import ctypes as C

import numpy as np
import pytest

from conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch
    from robosumo_selfplay_amd import ppo_capi
    from robosumo_selfplay_amd.ppo_capi import LstmNet, fill_lstm_net_ifou

    DEV = torch.device("cuda:0")

EPS = 2.0 ** -52


def _up(x, dt=np.float32):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=dt)).to(DEV)


def _st():
    return torch.cuda.current_stream(DEV).cuda_stream


# ---- moments / normalise -------------------------------------------------------------------------------------------------------
def _moments(ret, val, valid=None):
    L = ppo_capi.lib()
    n = ret.numel()
    ws = torch.zeros(L.ppo_adv_moments_workspace_bytes(), dtype=torch.uint8, device=DEV)
    mom = torch.full((3,), float("nan"), dtype=torch.float64, device=DEV)
    adv = torch.full((n + 2,), float("nan"), dtype=torch.float32, device=DEV)
    for _ in range(2):      # twice on one workspace: the arrival counter and the count are left at zero by every call
        if valid is None:
            ppo_capi.chk(L.ppo_adv_moments_ws(ret.data_ptr(), val.data_ptr(), None, n, mom.data_ptr(), ws.data_ptr(), _st()))
            ppo_capi.chk(L.ppo_adv_normalize(ret.data_ptr(), val.data_ptr(), None, n, mom.data_ptr(), adv.data_ptr(), _st()))
        else:
            ppo_capi.chk(L.ppo_adv_moments_masked_ws(ret.data_ptr(), val.data_ptr(), valid.data_ptr(), n, mom.data_ptr(), ws.data_ptr(), _st()))
            ppo_capi.chk(L.ppo_adv_normalize_masked(ret.data_ptr(), val.data_ptr(), valid.data_ptr(), n, mom.data_ptr(), adv.data_ptr(), _st()))
    torch.cuda.synchronize()
    a = adv.cpu().numpy()
    assert np.isnan(a[n:]).all(), "rows behind the last one were written"
    return mom.cpu().numpy(), a[:n]


@pytest.mark.parametrize("n", [1, 4095, 4096, 4097, 2 * 4096 + 1])
def test_masked_moments_and_normalise(n):
    rng = np.random.default_rng(n)
    r, v = rng.normal(0.3, 1.0, n).astype(np.float32), rng.normal(0, 1.0, n).astype(np.float32)
    ret, val = _up(r), _up(v)
    # every row valid: the unmasked entries, bit for bit
    m0, a0 = _moments(ret, val)
    m1, a1 = _moments(ret, val, _up(np.ones(n)))
    assert m1.tobytes() == m0.tobytes() and a1.tobytes() == a0.tobytes() and m1[2] == n
    # a random mask (row 0 kept valid so that n = 1 has a row): invalid rows carry NaN, which must reach nothing
    valid = rng.random(n) < 0.6
    valid[0] = True
    rm, vm = np.where(valid, r, np.float32("nan")), np.where(valid, v, np.float32("nan"))
    m2, a2 = _moments(_up(rm), _up(vm), _up(valid))
    nv = int(valid.sum())
    assert m2[2] == nv and np.isfinite(m2).all() and (a2[~valid] == 0).all() and np.isfinite(a2).all()
    mc, ac = _moments(_up(r[valid]), _up(v[valid]))                      # the unmasked entries on the compacted rows
    d = (r[valid] - v[valid]).astype(np.float64)                          # float32 subtraction first, as the kernels take it
    for k, term in enumerate((d, d * d)):
        print("n %d moment %d: masked %r compacted %r float64 %r" % (n, k, m2[k], mc[k], term.sum()))
    if n <= 4096:                                                         # one block, the same order
        assert m2.tobytes() == mc.tobytes() and a2[valid].tobytes() == ac.tobytes()
    else:
        for k, term in enumerate((d, d * d)):
            assert abs(m2[k] - term.sum()) <= n * EPS * np.abs(term).sum(), (k, m2[k], term.sum())
        # the normalisation is per row: the unmasked entry on the compacted rows, handed the masked moments, gives the same bits
        L = ppo_capi.lib()
        rc, vc, md = _up(r[valid]), _up(v[valid]), _up(m2, np.float64)
        want = torch.empty(nv, dtype=torch.float32, device=DEV)
        ppo_capi.chk(L.ppo_adv_normalize(rc.data_ptr(), vc.data_ptr(), None, nv, md.data_ptr(), want.data_ptr(), _st()))
        torch.cuda.synchronize()
        assert a2[valid].tobytes() == want.cpu().numpy().tobytes()
    # no valid row: zeros, no division
    m3, a3 = _moments(_up(rm), _up(vm), _up(np.zeros(n)))
    assert m3.tobytes() == np.zeros(3).tobytes() and a3.tobytes() == np.zeros(n, np.float32).tobytes()


def test_masked_moments_refuse_missing_arguments():
    L = ppo_capi.lib()
    z = torch.zeros(64, dtype=torch.float64, device=DEV)
    assert L.ppo_adv_moments_masked_ws(z.data_ptr(), z.data_ptr(), None, 4, z.data_ptr(), z.data_ptr(), _st()) != 0
    assert L.ppo_adv_normalize_masked(z.data_ptr(), z.data_ptr(), None, 4, z.data_ptr(), z.data_ptr(), _st()) != 0
    assert L.ppo_adv_moments_masked_ws(z.data_ptr(), z.data_ptr(), z.data_ptr(), 0, z.data_ptr(), z.data_ptr(), _st()) != 0


# ---- head gradient -------------------------------------------------------------------------------------------------------------
class _Head(object):
    """One head-gradient problem on the device: a net with random heads, ``rows`` latent rows and their per-row inputs."""

    def __init__(self, rows, H, A, seed):
        rng = np.random.default_rng(seed)
        self.rows, self.H, self.A = rows, H, A
        D = 5
        shapes = [(D, 4 * H), (H, 4 * H), (4 * H,), (H, A), (A,), (1, A), (H, 1), (1,)]
        host = [np.zeros(s, np.float32) for s in shapes]
        host[3] = rng.normal(0, 0.3, (H, A)).astype(np.float32); host[4] = rng.normal(0, 0.1, A).astype(np.float32)
        host[5] = rng.normal(-0.3, 0.1, (1, A)).astype(np.float32)
        host[6] = rng.normal(0, 0.3, (H, 1)).astype(np.float32); host[7] = rng.normal(0, 0.1, 1).astype(np.float32)
        self.ts = [_up(x) for x in host]
        self.net = fill_lstm_net_ifou(LstmNet(), D, A, H, [t.data_ptr() for t in self.ts])
        self.lat = rng.uniform(-1, 1, (rows, H)).astype(np.float32)
        mean = self.lat @ host[3] + host[4]
        self.act = (mean + rng.normal(0, 0.7, (rows, A))).astype(np.float32)
        z = (self.act - mean) / np.exp(host[5])
        nlp = 0.5 * (z * z).sum(1) + 0.5 * np.log(2 * np.pi) * A + host[5].sum()
        self.old = (nlp + rng.normal(0, 0.25, rows)).astype(np.float32)      # ratios on both sides of the clip range
        self.adv = rng.normal(0, 1, rows).astype(np.float32)
        self.ret = rng.normal(0, 1, rows).astype(np.float32)
        self.w = rng.uniform(0.5, 1.5, rows).astype(np.float32)

    def run(self, sel=None, inv_count=None, valid=None, count=None, old=None, stats0=None):
        """The unmasked entry on the rows ``sel`` (default all) with ``inv_count``, or the masked one with ``valid`` / ``count``.
        -> (dlatent, dmean, dvalue, dlogstd_rows, stats); two guard rows behind every output must stay NaN."""
        L = ppo_capi.lib()
        sel = np.arange(self.rows) if sel is None else np.asarray(sel)
        rows, H, A = len(sel), self.H, self.A
        old = self.old if old is None else old
        ins = [_up(x[sel]) for x in (self.lat, self.act, self.adv, self.ret, old, self.w)]
        outs = [torch.full((rows + 2, c), float("nan"), dtype=torch.float32, device=DEV) for c in (H, A, 1, A)]
        stats = torch.zeros(ppo_capi.NSTATS, dtype=torch.float64, device=DEV) if stats0 is None else _up(stats0, np.float64)
        lat, act, adv, ret, oldd, w = ins
        if valid is None:
            ppo_capi.chk(L.ppo_lstm_head_grad(C.byref(self.net), lat.data_ptr(), rows, act.data_ptr(), adv.data_ptr(), ret.data_ptr(), oldd.data_ptr(),
                                              w.data_ptr(), float(inv_count), 0.2, 0.5, *[o.data_ptr() for o in outs], stats.data_ptr(), _st()))
        else:
            vd, cd = _up(valid[sel]), _up([count], np.float64)
            ppo_capi.chk(L.ppo_lstm_head_grad_masked(C.byref(self.net), lat.data_ptr(), rows, act.data_ptr(), adv.data_ptr(), ret.data_ptr(),
                                                     oldd.data_ptr(), w.data_ptr(), vd.data_ptr(), cd.data_ptr(), 0.2, 0.5,
                                                     *[o.data_ptr() for o in outs], stats.data_ptr(), _st()))
        torch.cuda.synchronize()
        res = []
        for o in outs:
            a = o.cpu().numpy()
            assert np.isnan(a[rows:]).all(), "guard rows were written"
            res.append(a[:rows])
        return res + [stats.cpu().numpy()]

    def row_terms(self):
        """[rows][NSTATS] float64: what each row adds to the statistics (the unmasked kernel, one row per launch)."""
        L = ppo_capi.lib()
        ins = [_up(x) for x in (self.lat, self.act, self.adv, self.ret, self.old, self.w)]
        outs = [torch.empty((1, c), dtype=torch.float32, device=DEV) for c in (self.H, self.A, 1, self.A)]
        terms = torch.zeros((self.rows, ppo_capi.NSTATS), dtype=torch.float64, device=DEV)
        for r in range(self.rows):
            ptrs = [x[r:].data_ptr() for x in ins]
            ppo_capi.chk(L.ppo_lstm_head_grad(C.byref(self.net), ptrs[0], 1, ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5], 1.0, 0.2, 0.5,
                                              *[o.data_ptr() for o in outs], terms[r].data_ptr(), _st()))
        torch.cuda.synchronize()
        return terms.cpu().numpy()


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("A", [8, 16])
@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("rows", [127, 128, 129])
def test_masked_head_gradient(rows, H, A):
    """The masked head gradient against the unmasked entry.  The float64 reference of the statistics is the sum over the valid rows of
    the per-row terms that ``ppo_lstm_head_grad`` itself produces, one row per launch (``_Head.row_terms``), not an independent
    restatement of the loss: a float32 restatement in numpy does not reproduce the kernel's terms to the last bit, and the bound
    n 2^-52 sum|term| is about the SUMMATION.  So this checks the masked reduction (which rows enter, that nothing else does, the
    count) and not the term arithmetic; that is pinned by the existing tests of the unmasked kernel and, above, by the bitwise
    comparison of every valid row's outputs with it."""
    P = _Head(rows, H, A, seed=rows * 1000 + H + A)
    # every row valid, *count_dev = rows: every output and the statistics equal the unmasked entry's, bit for bit
    plain = P.run(inv_count=1.0 / rows)
    full = P.run(valid=np.ones(rows, np.float32), count=rows)
    assert _same(full, plain) and plain[4][6] == rows and 0 < plain[4][4] < rows          # clipped and unclipped rows present
    # a random mask; one invalid row carries a NaN old neglogp (an unmasked row like it poisons stats[3])
    rng = np.random.default_rng(rows + H + A)
    valid = (rng.random(rows) < 0.6).astype(np.float32)
    valid[0], valid[rows - 1], valid[1] = 1.0, 1.0, 0.0        # both ends of the launch valid, row 1 invalid
    old = P.old.copy()
    old[1] = np.nan
    nv = int(valid.sum())
    sel = np.nonzero(valid)[0]
    got = P.run(valid=valid, count=nv, old=old)
    comp = P.run(sel=sel, inv_count=1.0 / nv)                  # the unmasked entry on the compacted rows
    for g, c in zip(got[:4], comp[:4]):
        assert not g[valid == 0].any() and not np.signbit(g[valid == 0]).any()           # exact zeros
        assert g[sel].tobytes() == c.tobytes()
    terms = P.row_terms()
    assert np.isfinite(got[4]).all() and got[4][6] == nv
    for k in (0, 1, 3, 4):
        t = terms[sel, k]
        print("rows %d H %d A %d stats[%d]: masked %r compacted %r float64 %r" % (rows, H, A, k, got[4][k], comp[4][k], t.sum()))
        assert abs(got[4][k] - t.sum()) <= rows * EPS * np.abs(t).sum(), (k, got[4][k], t.sum())
    assert got[4][2] == 0 and got[4][5] == 0 and got[4][7] == 0                             # slots the kernel never touches
    # no valid row (count 0 -> inv_count 1): zeros everywhere, the statistics untouched
    s0 = np.arange(1, ppo_capi.NSTATS + 1, dtype=np.float64) * 1.5
    none = P.run(valid=np.zeros(rows, np.float32), count=0, old=old, stats0=s0)
    assert all(not x.any() for x in none[:4]) and none[4].tobytes() == s0.tobytes()


def test_masked_head_gradient_refuses_missing_arguments():
    L = ppo_capi.lib()
    P = _Head(4, 64, 8, seed=1)
    z = torch.zeros(4096, dtype=torch.float32, device=DEV)
    p = z.data_ptr()
    assert L.ppo_lstm_head_grad_masked(C.byref(P.net), p, 4, p, p, p, p, p, None, p, 0.2, 0.5, p, p, p, p, p, _st()) != 0
    assert L.ppo_lstm_head_grad_masked(C.byref(P.net), p, 4, p, p, p, p, p, p, None, 0.2, 0.5, p, p, p, p, p, _st()) != 0
    assert L.ppo_lstm_head_grad_masked(C.byref(P.net), p, 0, p, p, p, p, p, p, p, 0.2, 0.5, p, p, p, p, p, _st()) != 0
