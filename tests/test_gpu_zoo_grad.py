"""ppo_grad_act (the PPO gradient of a policy-zoo MLP net: tanh trunks, value affine) and ppo_obs_filter.

* against the float64 reference tests/zoo_grad_ref.py (checked by central differences in tests/test_zoo_learner_cpu.py) at the three zoo
  widths -- the KT = 8 / 11 / 14 variants of the kernel -- on tail tiles, one and several workgroups per net, a shuffled gather, with the
  bounds of tests/test_gpu_ppo.py::test_gradients_match_oracle (2e-4 per tensor; 1e-4, 1e-4, 1e-3 on the statistics; 1e-4 on log-ratios);
* with flags = 0, v_scale = 1, v_shift = 0 against ppo_grad, bit for bit, on the integer problems of tests/exact_mlp_ref.py;
* ppo_obs_filter against the float32 numpy expression, bit for bit, in place and out of place, guard columns untouched;
* every argument refusal of the two entries."""
import numpy as np
import pytest

import exact_mlp_ref as E
import zoo_grad_ref as Z
from conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch
    from oracle import ppo_oracle as po
    from robosumo_selfplay_amd import policies, ppo_capi

    DEV = torch.device("cuda:0")

WIDTHS = [(120, 8), (164, 12), (208, 16)]
ROWS = [1, 15, 16, 17, 37, 1000]          # 1000: through a shuffled idx out of 2000 data rows
V_SCALE, V_SHIFT, CLIP = 2.5, 0.7, 5.0
_WS, _PROBLEM = {}, {}


def _up(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def _workspace(ob, ac):
    """One workspace per net (its layout depends on the parameter count), zeroed once."""
    if (ob, ac) not in _WS:
        _WS[(ob, ac)] = torch.zeros(ppo_capi.lib().ppo_grad_workspace_bytes(ob, ac), dtype=torch.uint8, device=DEV)
    return _WS[(ob, ac)]


def _problem(ob, ac, n):
    """Inputs and the float64 reference of one (width, rows) case, computed once and left unchanged."""
    key = (ob, ac, n)
    if key in _PROBLEM:
        return _PROBLEM[key]
    rng = np.random.RandomState(100 * ob + n)
    NB = 2000 if n == 1000 else n
    p = Z.random_net(rng, ob, ac)
    raw = rng.normal(0.5, 2.0, (NB, ob)).astype(np.float32)
    fmean = rng.normal(0.5, 0.5, ob).astype(np.float32)
    finv = rng.uniform(0.3, 1.5, ob).astype(np.float32)              # some entries reach the clip
    filt = (fmean, finv, CLIP)
    act = rng.normal(0, 1, (NB, ac)).astype(np.float32)
    ret = rng.normal(V_SHIFT, 2, NB).astype(np.float32)
    val = rng.normal(V_SHIFT, 2, NB).astype(np.float32)
    mean, _, _ = Z.forward(p, raw, filt)
    old = (po.neglogp(mean, p[10].astype(np.float64), act) + rng.normal(0, 0.3, NB)).astype(np.float32)
    w = rng.uniform(0.5, 2.0, NB).astype(np.float32)
    idx = rng.permutation(NB)[:n].astype(np.int32) if n == 1000 else None
    sel = idx if idx is not None else np.arange(n)
    advs = po.normalize_advantages(ret[sel], val[sel]).astype(np.float32)
    ref = Z.loss_and_grads(p, raw[sel], act[sel], advs, ret[sel], old[sel], w[sel], 0.2, 0.01, 0.5, filt=filt, v_scale=V_SCALE, v_shift=V_SHIFT)
    _PROBLEM[key] = dict(p=p, raw=raw, filt=filt, act=act, ret=ret, old=old, w=w, idx=idx, advs=advs, ref=ref, NB=NB)
    return _PROBLEM[key]


def _filtered(pr, ob):
    """The rows through ppo_obs_filter into a buffer of stride ob + 1 whose guard column is NaN."""
    L = ppo_capi.lib()
    raw, mean, inv = _up(pr["raw"]), _up(pr["filt"][0]), _up(pr["filt"][1])
    out = torch.full((pr["NB"], ob + 1), float("nan"), dtype=torch.float32, device=DEV)
    ppo_capi.chk(L.ppo_obs_filter(raw.data_ptr(), pr["NB"], ob, ob, mean.data_ptr(), inv.data_ptr(), CLIP, out.data_ptr(), ob + 1, None))
    return out


def _errors(g, st, lrat, ref, ob, ac, n):
    """(worst per-tensor relative error, [pg, vf, kl] relative errors, clipfrac and log-ratio absolute errors)."""
    _, stats, lr, grads = ref
    worst = 0.0
    for a, b in zip(policies.unflatten_params(g, ob, ac), grads):
        b = np.asarray(b).reshape(a.shape)
        worst = max(worst, float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12)))
    rel = [abs(st[k] / n - stats[k]) / max(abs(stats[k]), 1e-30) for k in (0, 1, 3)]
    return worst, rel, abs(st[4] / n - stats[4]), float(np.abs(lrat - lr).max())


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("ob,ac", WIDTHS)
def test_gradients_match_the_float64_reference(ob, ac, n, monkeypatch):
    pr = _problem(ob, ac, n)
    L, ws = ppo_capi.lib(), _workspace(ob, ac)
    obs = _filtered(pr, ob)
    assert torch.isnan(obs[:, ob]).all()
    params = _up(policies.flatten_params(pr["p"]))
    act, ret, old, w, idx, adv = (_up(pr[k]) for k in ("act", "ret", "old", "w", "idx", "advs"))
    _, stats, lr, _ = pr["ref"]
    for cap in (None, 1, 3):                                            # the default grid, one workgroup per net, three
        if cap is None:
            monkeypatch.delenv("PPO_GRAD_BLOCKS", raising=False)
        else:
            monkeypatch.setenv("PPO_GRAD_BLOCKS", str(cap))
        g = torch.full((params.numel(),), 777.0, dtype=torch.float32, device=DEV)
        st = torch.zeros(8, dtype=torch.float64, device=DEV)
        lrat = torch.full((n + 16,), float("nan"), dtype=torch.float32, device=DEV)
        ppo_capi.chk(L.ppo_grad_act(params.data_ptr(), obs.data_ptr(), ob + 1, ob, ac, act.data_ptr(), adv.data_ptr(), ret.data_ptr(),
                                    old.data_ptr(), w.data_ptr(), ppo_capi.ptr(idx), n, 1.0 / n, 0.2, 0.01, 0.5, ppo_capi.GRAD_TANH,
                                    V_SCALE, V_SHIFT, g.data_ptr(), st.data_ptr(), lrat.data_ptr(), ws.data_ptr(), None))
        torch.cuda.synchronize()
        s, lg = st.cpu().numpy(), lrat.cpu().numpy()
        worst, rel, dclip, dlr = _errors(g.cpu().numpy(), s, lg[:n], pr["ref"], ob, ac, n)
        print("ppo_grad_act (%d, %d) n %d cap %s: tensor %.3g  pg %.3g vf %.3g kl %.3g  clipfrac %.3g  log-ratio %.3g"
              % (ob, ac, n, cap, worst, rel[0], rel[1], rel[2], dclip, dlr))
        assert worst < 2e-4
        assert s[6] == n and np.isnan(lg[n:]).all()
        assert s[0] / n == pytest.approx(stats[0], rel=1e-4, abs=1e-6) and s[1] / n == pytest.approx(stats[1], rel=1e-4)
        assert s[3] / n == pytest.approx(stats[3], rel=1e-3, abs=1e-6) and s[4] / n == pytest.approx(stats[4], abs=2.0 / n)
        assert np.allclose(lg[:n], lr, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("name", ["width-121-8", "width-209-16"])
def test_flags_zero_is_ppo_grad_bit_for_bit(name, monkeypatch):
    case = [c for c in E.CASES if c[0] == name][0]
    d = E.build_case(case)
    ob, ac, n = d["ob"], d["ac"], d["n"]
    monkeypatch.setenv("PPO_GRAD_BLOCKS", str(d["cap"]))
    L, ws = ppo_capi.lib(), _workspace(ob, ac)
    params = _up(policies.flatten_params(E.problem(ob, ac)["params"]))
    obs, act, ret, w, old, idx, adv = (_up(d[k]) for k in ("obs", "act", "ret", "w", "old", "idx", "adv_mb"))
    outs = []
    for entry in ("ppo_grad", "ppo_grad_act"):
        g = torch.full((params.numel(),), 777.0, dtype=torch.float32, device=DEV)
        st = torch.zeros(8, dtype=torch.float64, device=DEV)
        lrat = torch.full((n,), 777.0, dtype=torch.float32, device=DEV)
        head = (params.data_ptr(), obs.data_ptr(), d["obs_stride"], ob, ac, act.data_ptr(), adv.data_ptr(), ret.data_ptr(), old.data_ptr(),
                w.data_ptr(), ppo_capi.ptr(idx), n, 1.0, 0.2, 1.0, 1.0)
        tail = (g.data_ptr(), st.data_ptr(), lrat.data_ptr(), ws.data_ptr(), None)
        ppo_capi.chk(getattr(L, entry)(*head, *(() if entry == "ppo_grad" else (0, 1.0, 0.0)), *tail))
        torch.cuda.synchronize()
        outs.append((g.cpu().numpy(), st.cpu().numpy(), lrat.cpu().numpy()))
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()
    assert np.isfinite(outs[0][0]).all() and outs[0][0].any() and outs[0][1][6] == n


@pytest.mark.parametrize("n", [1, 17])
@pytest.mark.parametrize("in_place", [False, True])
def test_obs_filter_is_the_numpy_expression(n, in_place):
    rng = np.random.RandomState(n)
    ob, stride, ostride = 120, 123, 123 if in_place else 125
    x = rng.normal(0.5, 3.0, (n, stride)).astype(np.float32)
    mean, inv = rng.normal(0.5, 0.5, ob).astype(np.float32), rng.uniform(0.3, 3.0, ob).astype(np.float32)
    want = np.clip((x[:, :ob] - mean) * inv, np.float32(-CLIP), np.float32(CLIP))
    assert want.dtype == np.float32 and (np.abs(want) == CLIP).any() and (np.abs(want) < CLIP).any()
    src, dm, di = _up(x), _up(mean), _up(inv)
    dst = src if in_place else torch.full((n, ostride), 7.0, dtype=torch.float32, device=DEV)
    ppo_capi.chk(ppo_capi.lib().ppo_obs_filter(src.data_ptr(), n, stride, ob, dm.data_ptr(), di.data_ptr(), CLIP, dst.data_ptr(), ostride, None))
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert got[:, :ob].tobytes() == want.tobytes()
    guard = x[:, ob:] if in_place else np.full((n, ostride - ob), 7.0, np.float32)
    assert np.array_equal(got[:, ob:], guard)
    if not in_place:
        assert np.array_equal(src.cpu().numpy(), x)


def test_argument_refusals():
    L = ppo_capi.lib()
    ob, ac, n = 120, 8, 16
    ws = _workspace(ob, ac)
    P = L.ppo_param_count(ob, ac)
    buf = torch.zeros(P + n * (ob + ac + 8), dtype=torch.float32, device=DEV)
    st = torch.zeros(8, dtype=torch.float64, device=DEV)
    p = buf.data_ptr()

    def grad(**kw):
        a = dict(params=p, obs=p, stride=ob, ob=ob, ac=ac, act=p, adv=p, ret=p, old=p, w=p, idx=None, n=n, inv=1.0 / n, clip=0.2, ent=0.0, vf=0.5,
                 flags=ppo_capi.GRAD_TANH, scale=1.0, shift=0.0, grads=p, stats=st.data_ptr(), lr=None, ws=ws.data_ptr())
        a.update(kw)
        return L.ppo_grad_act(a["params"], a["obs"], a["stride"], a["ob"], a["ac"], a["act"], a["adv"], a["ret"], a["old"], a["w"], a["idx"], a["n"],
                              a["inv"], a["clip"], a["ent"], a["vf"], a["flags"], a["scale"], a["shift"], a["grads"], a["stats"], a["lr"], a["ws"], None)

    before = buf.clone()
    for kw, msg in ([(dict(flags=2), "flags"), (dict(flags=3), "flags"), (dict(flags=-1), "flags")]
                    + [(dict(scale=s), "v_scale") for s in (0.0, -1.0, float("nan"), float("inf"))]
                    + [(dict(shift=s), "v_shift") for s in (float("nan"), float("inf"), float("-inf"))]
                    + [(dict([(k, None)]), "bad arguments") for k in ("params", "obs", "act", "adv", "ret", "old", "w", "grads", "stats", "ws")]
                    + [(dict(n=0), "bad arguments"), (dict(ac=17), "ac_dim"), (dict(ac=0), "ac_dim"), (dict(ob=225), "ob_dim")]):
        for flags in ((kw["flags"],) if "flags" in kw else (0, ppo_capi.GRAD_TANH)):
            assert grad(**dict(kw, flags=flags)) < 0, kw
            assert msg in L.ppo_last_error().decode(), (kw, L.ppo_last_error())
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and not bool(st.any())              # nothing was launched

    def filt(**kw):
        a = dict(obs=p, n=n, stride=ob, ob=ob, mean=p, inv=p, clip=5.0, out=p + 4 * n * ob, ostride=ob)
        a.update(kw)
        return L.ppo_obs_filter(a["obs"], a["n"], a["stride"], a["ob"], a["mean"], a["inv"], a["clip"], a["out"], a["ostride"], None)

    for kw in (dict(n=0), dict(n=-3), dict(obs=None), dict(mean=None), dict(inv=None), dict(out=None), dict(clip=0.0), dict(clip=-5.0),
               dict(clip=float("nan")), dict(ostride=ob - 1), dict(stride=ob - 1), dict(ob=0), dict(out=p, ostride=ob + 1, stride=ob)):
        assert filt(**kw) < 0, kw
        assert "ppo_obs_filter" in L.ppo_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
