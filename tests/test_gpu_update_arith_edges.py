"""Rollout and optimiser arithmetic of include/sumo_ppo.h at edge shapes: ppo_adv_moments (multi-block arrival counter, grid-stride
chunks, the workspace pool wrapping round), ppo_adv_normalize, ppo_vtrace (block edges, done patterns, ratios on the bars, NaN / inf
propagation), ppo_clip_adam (block edges, every clipping branch), ppo_reward_mix / ppo_post_step / ppo_loss_stats / ppo_a2c_loss_stats.
References: int64 / float64 numpy and oracle/ppo_oracle.py; every tolerance is the one tests/test_gpu_ppo.py already uses for the
same quantity, everything else is compared exactly."""
import numpy as np
import pytest

from conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch
    from oracle import ppo_oracle as po
    from robosumo_selfplay_amd import ppo_capi

    DEV = torch.device("cuda:0")


def _up(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


# ------------------------------------------------------------------------------------------------------------------------------------
# advantage moments: integer-valued returns / values, |x| <= 64, so sum d and sum d^2 are exact in float64 in any order
# ------------------------------------------------------------------------------------------------------------------------------------
ADV_PART_BYTES = 2 * 256 * 8      # the per-block partial sums at the head of the workspace; the arrival counter follows them


def _adv_problem(n, use_idx, seed):
    rng = np.random.RandomState(seed)
    NB = n + n // 2 + 3 if use_idx else n
    ret = rng.randint(-64, 65, NB).astype(np.float32)
    val = rng.randint(-64, 65, NB).astype(np.float32)
    idx = None
    if use_idx:                                   # gather from a larger array, duplicates allowed, unused entries NaN
        idx = rng.randint(0, NB, n).astype(np.int32)
        unused = np.ones(NB, bool)
        unused[idx] = False
        ret[unused] = np.nan
        val[unused] = np.nan
    r, v = (ret, val) if idx is None else (ret[idx], val[idx])
    d = r.astype(np.int64) - v.astype(np.int64)
    return ret, val, idx, (int(d.sum()), int((d * d).sum()), n), (r, v)


def _moments_ws(ret, val, idx, n, ws):
    L = ppo_capi.lib()
    mom = torch.full((3,), -1.0, dtype=torch.float64, device=DEV)
    ppo_capi.chk(L.ppo_adv_moments_ws(ret.data_ptr(), val.data_ptr(), ppo_capi.ptr(idx), n, mom.data_ptr(), ws.data_ptr(), None))
    torch.cuda.synchronize()
    assert not bool(ws[ADV_PART_BYTES:].any()), "the arrival counter must be left at zero"
    return mom.cpu().numpy()


@pytest.mark.parametrize("use_idx", [False, True])
@pytest.mark.parametrize("n", [1, 63, 1024, 4095, 4096, 4097, 3 * 4096 + 5, 257 * 4096 + 7])
def test_adv_moments_exact_and_normalize(n, use_idx):
    """1 block / 1 chunk up to 256 blocks with block 0 taking two chunks (n = 257 * 4096 + 7): the three moments equal int64 numpy;
    the normalised advantages equal po.normalize_advantages at the tolerance of test_gradients_match_oracle (1e-5)."""
    L = ppo_capi.lib()
    ret, val, idx, want, (r, v) = _adv_problem(n, use_idx, 100 + n % 1000)
    d_ret, d_val, d_idx = _up(ret), _up(val), _up(idx)
    ws = torch.zeros(L.ppo_adv_moments_workspace_bytes(), dtype=torch.uint8, device=DEV)
    mom = _moments_ws(d_ret, d_val, d_idx, n, ws)
    assert (mom[0], mom[1], mom[2]) == want
    pooled = torch.zeros(3, dtype=torch.float64, device=DEV)
    ppo_capi.chk(L.ppo_adv_moments(d_ret.data_ptr(), d_val.data_ptr(), ppo_capi.ptr(d_idx), n, pooled.data_ptr(), None))
    adv = torch.full((n + 8,), 777.0, dtype=torch.float32, device=DEV)
    ppo_capi.chk(L.ppo_adv_normalize(d_ret.data_ptr(), d_val.data_ptr(), ppo_capi.ptr(d_idx), n, pooled.data_ptr(), adv.data_ptr(), None))
    torch.cuda.synchronize()
    assert tuple(pooled.cpu().numpy()) == want
    a = adv.cpu().numpy()
    assert np.all(a[n:] == 777.0)
    assert np.allclose(a[:n], po.normalize_advantages(r, v), rtol=1e-5, atol=1e-5)
    if n == 1:
        assert a[0] == 0.0


def test_adv_moments_workspace_across_grid_sizes_and_pool_wrap():
    """One caller workspace through a 4-block, a 1-block and a 4-block call (stale partials of the wide call must not count, the
    counter ends at zero each time); then 20 calls of the pool form (16 library workspaces, handed out round robin: four of them
    serve a second call) with alternating grid sizes, queued without a synchronisation in between."""
    L = ppo_capi.lib()
    ws = torch.zeros(L.ppo_adv_moments_workspace_bytes(), dtype=torch.uint8, device=DEV)
    probs = [_adv_problem(n, True, 7 + k) for k, n in enumerate([3 * 4096 + 5, 63, 3 * 4096 + 6, 1, 4097])]
    dev = [(_up(p[0]), _up(p[1]), _up(p[2])) for p in probs]
    for k in (0, 1, 2, 0):
        mom = _moments_ws(dev[k][0], dev[k][1], dev[k][2], probs[k][3][2], ws)
        assert tuple(mom) == probs[k][3], k
    out = torch.full((20, 3), -1.0, dtype=torch.float64, device=DEV)
    for c in range(20):
        k = c % len(probs)
        ppo_capi.chk(L.ppo_adv_moments(dev[k][0].data_ptr(), dev[k][1].data_ptr(), dev[k][2].data_ptr(), probs[k][3][2],
                                       out[c].data_ptr(), None))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    for c in range(20):
        assert tuple(o[c]) == probs[c % len(probs)][3], c


@pytest.mark.parametrize("n", [1, 4097])
def test_adv_normalize_constant_advantage_is_exact_zero(n):
    """ret - val = 0.375 in every row: sum d, sum d^2, the mean and the variance are exact in float64 (dyadic), so the variance is
    exactly 0 and every normalised advantage (d - mean) / (0 + 1e-8) exactly 0."""
    L = ppo_capi.lib()
    rng = np.random.RandomState(n)
    val = rng.randint(-64, 65, n).astype(np.float32)
    ret = val + np.float32(0.375)
    d_ret, d_val = _up(ret), _up(val)
    mom = torch.zeros(3, dtype=torch.float64, device=DEV)
    adv = torch.full((n,), 777.0, dtype=torch.float32, device=DEV)
    ppo_capi.chk(L.ppo_adv_moments(d_ret.data_ptr(), d_val.data_ptr(), None, n, mom.data_ptr(), None))
    ppo_capi.chk(L.ppo_adv_normalize(d_ret.data_ptr(), d_val.data_ptr(), None, n, mom.data_ptr(), adv.data_ptr(), None))
    torch.cuda.synchronize()
    assert tuple(mom.cpu().numpy()) == (0.375 * n, 0.140625 * n, n)
    assert not adv.cpu().numpy().any()
    assert not po.normalize_advantages(ret, val).any()


# ------------------------------------------------------------------------------------------------------------------------------------
# V-trace
# ------------------------------------------------------------------------------------------------------------------------------------
GAMMA, LAM = 0.995, 0.95


def _vtrace_kernel(rew, val, nlp, onlp, dones, last_d, last_v, rho_bar, c_bar):
    T, N = rew.shape[1:]
    keep = [_up(x) for x in (rew, val, nlp, onlp, dones.astype(np.uint8), last_d.astype(np.uint8), last_v)]
    ret = torch.full((2, T, N), 777.0, dtype=torch.float32, device=DEV)
    r1, r2, r3 = (torch.full((T, N), 777.0, dtype=torch.float32, device=DEV) for _ in range(3))
    ppo_capi.chk(ppo_capi.lib().ppo_vtrace(*[k.data_ptr() for k in keep], T, N, GAMMA, LAM, rho_bar, c_bar, ret.data_ptr(), r1.data_ptr(),
                                           r2.data_ptr(), r3.data_ptr(), None))
    torch.cuda.synchronize()
    return ret.cpu().numpy(), r1.cpu().numpy(), r2.cpu().numpy(), r3.cpu().numpy()


def _vtrace_oracle(rew, val, nlp, onlp, dones, last_d, last_v, rho_bar, c_bar):
    """runner.py:166-196 in numpy float32 / float64 as test_vtrace_kernel_vs_oracle_large restates it"""
    with np.errstate(all="ignore"):
        opr, oer = np.exp(onlp[1] - nlp[1]), np.exp(nlp[0] - onlp[0])
        ratio = opr * oer
        ones = np.ones_like(ratio)
        e0 = po.vtrace_returns(rew[0], val[0], dones[0], last_d[:, 0], last_v[0], ones, ones * np.float32(LAM), GAMMA)
        e1 = po.vtrace_returns(rew[1], val[1], dones[1], last_d[:, 1], last_v[1], np.clip(ratio, None, np.float32(rho_bar)),
                               np.clip(ratio, None, np.float32(c_bar)) * np.float32(LAM), GAMMA)
    return e0, e1, opr, oer, ratio


def _dones(pattern, T, N, rng):
    d, last = np.zeros((2, T, N), bool), np.zeros((N, 2), bool)
    if pattern == "all":
        d[:], last[:] = True, True
    elif pattern == "every_step":          # every recorded step starts an episode, the step after the rollout does not
        d[:] = True
    elif pattern == "only_last":
        last[:] = True
    elif pattern == "agents_differ":       # the two agents' flags differ, inside the rollout and after it
        d[0] = rng.uniform(size=(T, N)) < 0.4
        d[1] = rng.uniform(size=(T, N)) < 0.4
        last[:, 0] = np.arange(N) % 2 == 0
        last[:, 1] = ~last[:, 0]
    else:
        assert pattern == "none"
    return d, last


@pytest.mark.parametrize("pattern", ["none", "all", "every_step", "only_last", "agents_differ"])
@pytest.mark.parametrize("T,N", [(1, 1), (1, 129), (3, 128), (2, 257), (5, 130)])
def test_vtrace_edge_shapes_done_patterns_and_ratios(T, N, pattern):
    """One env / one step, one env past a 128-thread block, exactly a block, two blocks + 1.  Four ratio regimes per shape:
      equal   opponent neglogp == neglogp: both ratios exactly 1 = rho_bar = c_bar, so agent 1's returns are bitwise the oracle's too;
      spread  neglogp differences in {0, +2, -2}: ratios from e^-4 to e^4, far from both bars or exactly on them;
      nan     NaN neglogps: the NaN masks of agent 1's returns and of the three ratio outputs equal numpy's, agent 0 is not touched;
      inf     +200 in one array against -200 in the other: inf * 0 -> NaN exactly where numpy float32 has it.
    Agent 0 always bitwise; finite values of agent 1 at rtol 1e-5 / atol 1e-4 and ratios at rtol 2e-6 as the existing test."""
    rng = np.random.RandomState(1000 * T + N)
    rew = rng.normal(0, 3, (2, T, N)).astype(np.float32)
    val = rng.normal(0, 5, (2, T, N)).astype(np.float32)
    nlp = rng.normal(10, 1, (2, T, N)).astype(np.float32)
    last_v = rng.normal(0, 5, (2, N)).astype(np.float32)
    dones, last_d = _dones(pattern, T, N, rng)
    diff = (rng.randint(-1, 2, (2, T, N)) * 2).astype(np.float32)
    cell = rng.permutation(T * N)[:3] if T * N >= 3 else np.zeros(3, int)       # three distinct cells (one env, one step: the only one)
    for regime in ("equal", "spread", "nan", "inf"):
        onlp = nlp.copy() if regime == "equal" else (nlp + diff).astype(np.float32)
        nl = nlp.copy()
        if regime == "nan":
            onlp[1].ravel()[cell[0]] = np.nan
            nl[0].ravel()[cell[1]] = np.nan
            nl[1].ravel()[cell[2]] = np.nan
        if regime == "inf":
            onlp[1].ravel()[cell[0]] = nl[1].ravel()[cell[0]] + np.float32(200)      # off-policy ratio inf ...
            onlp[0].ravel()[cell[0]] = nl[0].ravel()[cell[0]] + np.float32(200)      # ... times off-env ratio 0
            onlp[1].ravel()[cell[1]] = nl[1].ravel()[cell[1]] - np.float32(200)      # and 0 * inf
            onlp[0].ravel()[cell[1]] = nl[0].ravel()[cell[1]] - np.float32(200)
        for rho_bar, c_bar in ((1.0, 1.0), (10.0, 1.0)):
            g, opr, oer, ratio = _vtrace_kernel(rew, val, nl, onlp, dones, last_d, last_v, rho_bar, c_bar)
            e0, e1, eopr, eoer, eratio = _vtrace_oracle(rew, val, nl, onlp, dones, last_d, last_v, rho_bar, c_bar)
            assert np.array_equal(g[0], e0), (regime, "agent 0 returns must be bit-exact")
            for got, want in ((opr, eopr), (oer, eoer), (ratio, eratio)):
                assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want)), regime
                fin = np.isfinite(want)
                assert np.allclose(got[fin], want[fin], rtol=2e-6, atol=0), regime
            assert np.array_equal(np.isnan(g[1]), np.isnan(e1)), regime
            fin = np.isfinite(e1)
            assert np.array_equal(np.isfinite(g[1]), fin) and np.allclose(g[1][fin], e1[fin], rtol=1e-5, atol=1e-4), regime
            if regime == "equal":
                assert np.all(ratio == 1.0) and np.array_equal(g[1], e1), "ratio exactly 1: agent 1 bit-exact too"
            if regime == "nan":
                assert np.isnan(eratio).sum() >= 1 and np.isnan(e1).sum() >= 1
            if regime == "inf":
                assert np.isnan(eratio.ravel()[cell[:2]]).all() and (np.isinf(eopr) | np.isinf(eoer)).any() and ((eopr == 0) | (eoer == 0)).any()


# ------------------------------------------------------------------------------------------------------------------------------------
# clip_by_global_norm + Adam
# ------------------------------------------------------------------------------------------------------------------------------------
def _clip_adam(p0, m0, v0, g, t, max_norm, with_stats=True):
    p, m, v, dg = (_up(x.copy()) for x in (p0, m0, v0, g))
    st = torch.full((8,), -1.0, dtype=torch.float64, device=DEV) if with_stats else None
    ppo_capi.chk(ppo_capi.lib().ppo_clip_adam(p.data_ptr(), dg.data_ptr(), m.data_ptr(), v.data_ptr(), len(p0), t, 1e-3, 0.9, 0.999, 1e-5,
                                              max_norm, ppo_capi.ptr(st), None))
    torch.cuda.synchronize()
    return p.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), (st.cpu().numpy() if with_stats else None)


def _adam_oracle(p0, m0, v0, g, t, max_norm, clip=True):
    g64 = g.astype(np.float64)
    with np.errstate(all="ignore"):
        if clip and max_norm > 0:
            gc, norm = po.clip_by_global_norm([g64], max_norm)
        else:
            gc, norm = [g64], np.sqrt(np.sum(np.square(g64)))
        ep, em, ev = po.adam_step([p0.astype(np.float64)], gc, [m0.astype(np.float64)], [v0.astype(np.float64)], t, 1e-3)
    return ep[0], em[0], ev[0], norm


def _close(got, want):
    """test_clip_adam_matches_tf1_formulation's tolerances; NaN masks must agree, finite entries are compared"""
    for (a, b, atol) in zip(got[:3], want[:3], (1e-6, 1e-7, 1e-9)):
        if not np.array_equal(np.isnan(a), np.isnan(b)):
            return False
        fin = ~np.isnan(b)
        if not np.allclose(a[fin], b[fin], rtol=1e-5, atol=atol):
            return False
    return True


@pytest.mark.parametrize("t", [1, 7, 10 ** 6])
@pytest.mark.parametrize("P", [1, 1023, 1024, 1025, 8192, 8193, 24529])
def test_clip_adam_block_edges_and_every_branch(P, t):
    """P around the 1024-parameter block and the 8192-entry stride of the norm loop; first step, a middle step, bias correction gone.
    The second-moment history is of order 1 (in [0.5, 1.5]): the kernel forms 1 - beta2 in float32 as TF does, 4.7e-5 relative from
    the float64 value, so the existing 1e-5 bound on v is a bound on a v that its history dominates -- as in the existing test."""
    rng = np.random.RandomState(P + t % 1000)
    p0 = rng.normal(0, 1, P).astype(np.float32)
    m0 = rng.normal(0, 0.1, P).astype(np.float32)
    v0 = rng.uniform(0.5, 1.5, P).astype(np.float32)
    g = rng.normal(0, 0.05, P).astype(np.float32)
    norm = float(np.sqrt(np.sum(np.square(g.astype(np.float64)))))
    # norm < max_norm: moves as if unclipped
    got = _clip_adam(p0, m0, v0, g, t, 2.0 * norm)
    assert _close(got, _adam_oracle(p0, m0, v0, g, t, 0.0, clip=False)) and got[3][7] == pytest.approx(norm, rel=1e-5)
    # norm > max_norm
    got = _clip_adam(p0, m0, v0, g, t, 0.5 * norm)
    assert _close(got, _adam_oracle(p0, m0, v0, g, t, 0.5 * norm)) and got[3][7] == pytest.approx(norm, rel=1e-5)
    # stats = NULL: same update
    again = _clip_adam(p0, m0, v0, g, t, 0.5 * norm, with_stats=False)
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], again[:3]))
    # max_norm = 0: no clipping
    got = _clip_adam(p0, m0, v0, g, t, 0.0)
    assert _close(got, _adam_oracle(p0, m0, v0, g, t, 0.0)) and got[3][7] == pytest.approx(norm, rel=1e-5)
    # norm exactly max_norm: (3, 4, 0, ...) against 5 (P = 1: (5))
    ge = np.zeros(P, np.float32)
    ge[:2] = (3, 4) if P > 1 else (5,)
    got = _clip_adam(p0, m0, v0, ge, t, 5.0)
    assert got[3][7] == 5.0 and _close(got, _adam_oracle(p0, m0, v0, ge, t, 0.0, clip=False)) and _close(got, _adam_oracle(p0, m0, v0, ge, t, 5.0))
    # all-zero gradient: 0 / max(0, max_norm), no NaN
    gz = np.zeros(P, np.float32)
    got = _clip_adam(p0, m0, v0, gz, t, 0.5)
    assert got[3][7] == 0.0 and all(np.isfinite(x).all() for x in got[:3]) and _close(got, _adam_oracle(p0, m0, v0, gz, t, 0.5))
    # one inf entry: norm inf, scale 0, inf * 0 = NaN in that entry alone
    gi = g.copy()
    gi[P // 2] = np.inf
    got, want = _clip_adam(p0, m0, v0, gi, t, 0.5), _adam_oracle(p0, m0, v0, gi, t, 0.5)
    assert np.isinf(got[3][7]) and np.isinf(want[3])
    assert _close(got, want) and np.isnan(got[0]).sum() == 1 and np.isnan(got[0][P // 2]) and np.isnan(got[1][P // 2]) and np.isnan(got[2][P // 2])


# ------------------------------------------------------------------------------------------------------------------------------------
# reward mix, post-step records, loss statistics
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [0.0, 1.0, float(np.linspace(1, 0, 500)[249])])
@pytest.mark.parametrize("n", [1, 127, 128, 129])
def test_reward_mix_and_post_step(n, alpha):
    """2 n threads around the 256-thread block; agent_stride = n + 5 with the gap sentinel-filled.  The reward is bitwise
    float32(alpha * shaping + (1 - alpha) * main) evaluated in float64; the episode records are agent 0's."""
    L = ppo_capi.lib()
    rng = np.random.RandomState(n)
    info = rng.normal(0, 3, (n, 2, 8))
    want = (alpha * info[:, :, 6] + (1 - alpha) * info[:, :, 3]).astype(np.float32).T          # [2][n]
    stride = n + 5
    d_info = _up(info)
    done = (rng.uniform(size=(n, 2)) < 0.5).astype(np.uint8)
    done[:, 1] = 1 - done[:, 0]                                  # agent 1's flag is the opposite: copying the wrong column shows
    ep_r, ep_l = rng.normal(0, 100, n), rng.randint(1, 500, n).astype(np.int32)
    d_done, d_epr, d_epl = _up(done), _up(ep_r), _up(ep_l)
    for post in (False, True):
        out = torch.full((2, stride), 777.0, dtype=torch.float32, device=DEV)
        o_done = torch.full((n + 3,), 9, dtype=torch.uint8, device=DEV)
        o_epr = torch.full((n + 3,), 777.0, dtype=torch.float64, device=DEV)
        o_epl = torch.full((n + 3,), 777, dtype=torch.int32, device=DEV)
        if post:
            ppo_capi.chk(L.ppo_post_step(d_info.data_ptr(), n, alpha, out.data_ptr(), stride, d_done.data_ptr(), d_epr.data_ptr(),
                                         d_epl.data_ptr(), o_done.data_ptr(), o_epr.data_ptr(), o_epl.data_ptr(), None))
        else:
            ppo_capi.chk(L.ppo_reward_mix(d_info.data_ptr(), n, alpha, out.data_ptr(), stride, None))
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert np.array_equal(o[:, :n], want) and np.all(o[:, n:] == 777.0)
        if post:
            assert np.array_equal(o_done.cpu().numpy()[:n], done[:, 0]) and np.all(o_done.cpu().numpy()[n:] == 9)
            assert np.array_equal(o_epr.cpu().numpy()[:n], ep_r) and np.all(o_epr.cpu().numpy()[n:] == 777.0)
            assert np.array_equal(o_epl.cpu().numpy()[:n], ep_l) and np.all(o_epl.cpu().numpy()[n:] == 777)


@pytest.mark.parametrize("ac", [1, 8, 16])
def test_loss_stats_from_sums(ac):
    """out = sums / count and the entropy of the diagonal Gaussian (po.entropy), to 1e-12."""
    L = ppo_capi.lib()
    rng = np.random.RandomState(ac)
    sums = rng.normal(0, 50, 8)
    sums[6] = 117.0
    logstd = rng.normal(0, 0.5, ac).astype(np.float32)
    d_s, d_l = _up(sums), _up(logstd)
    out5 = torch.full((6,), 777.0, dtype=torch.float64, device=DEV)
    out3 = torch.full((4,), 777.0, dtype=torch.float64, device=DEV)
    ppo_capi.chk(L.ppo_loss_stats(d_s.data_ptr(), d_l.data_ptr(), ac, out5.data_ptr(), None))
    ppo_capi.chk(L.ppo_a2c_loss_stats(d_s.data_ptr(), d_l.data_ptr(), ac, out3.data_ptr(), None))
    torch.cuda.synchronize()
    ent = po.entropy(logstd.astype(np.float64), 1)[0]
    o5, o3 = out5.cpu().numpy(), out3.cpu().numpy()
    assert o5[5] == 777.0 and o3[3] == 777.0
    assert np.abs(o5[:5] - np.array([sums[0] / 117, sums[1] / 117, ent, sums[3] / 117, sums[4] / 117])).max() <= 1e-12
    assert np.abs(o3[:3] - np.array([sums[0] / 117, sums[1] / 117, ent])).max() <= 1e-12
