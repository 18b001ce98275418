"""``ppo_mixed_pair_step`` (include/sumo_ppo.h) -- a learner seat on both sides of one step of a mixed match-up in one launch -- against
its definition, ``co_train.pair_step(fused=False)``: ``ppo_forward`` per run of tiles sharing a row and torch copies, per side.  Plain
buffers without an engine; obs / act rows wider than the widths, sentinels everywhere the kernel may not write, agent 1's done flags
the complement of agent 0's.  Every comparison is ``torch.equal`` over whole tensors."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import has_gpu

pytestmark = pytest.mark.gpu
if has_gpu():
    import torch
    from robosumo_selfplay_amd import co_train, matches, mixed, ppo_capi, zoo_pairs

HERE = os.path.dirname(os.path.abspath(__file__))
DIMS = {"ant": (121, 8), "bug": (165, 12), "spider": (209, 16)}            # what a learner of the species reads / writes
PAIRS = [("ant", "bug"), ("bug", "spider"), ("spider", "ant")]              # agent 0 / agent 1
ACT_SENTINEL, REC_SENTINEL, DONE_SENTINEL = 777.0, 333.0, 99
NROWS = 3
_CACHE = {}


def _seat(species, side):
    """Three distinct parameter rows of the species' MLP(64,64) policy (logstd away from zero, so the noise scale shows)."""
    key = (species, side)
    if key not in _CACHE:
        D, A = DIMS[species]
        rng = np.random.default_rng(7 + side)
        rows = [(0.1 * rng.standard_normal(matches.param_count(D, A))).astype(np.float32) for _ in range(NROWS)]
        _CACHE[key] = mixed.LearnerSeat(D, A, rows, device=0)
        assert len(_CACHE[key]) == NROWS and _CACHE[key].table.stride(0) == ppo_capi.lib().ppo_param_count(D, A)
    return _CACHE[key]


class _Bufs:
    """What ``pair_step`` reads of an env, without an engine."""

    def __init__(self, seats, n, seed=0):
        g = torch.Generator(device="cuda").manual_seed(seed)
        D, A = [s.ob_dim for s in seats], [s.ac_dim for s in seats]
        self.num_envs, self.device = n, torch.device("cuda", 0)
        self.model = type("Model", (), {"obs_dims": tuple(D), "act_dims": tuple(A)})()
        self.spec = type("Spec", (), {"id": "buffers"})()
        self.obs_dev = 3.0 * torch.randn((n, 2, max(D) + 6), generator=g, device="cuda")
        self.act_dev = torch.full((n, 2, max(A) + 3), ACT_SENTINEL, device="cuda")
        self.noise = tuple(torch.randn((n, a), generator=g, device="cuda") for a in A)
        self.done_dev = torch.zeros((n, 2), dtype=torch.uint8, device="cuda")
        self.done_dev[:, 0] = (torch.rand(n, generator=g, device="cuda") < 0.4).to(torch.uint8)
        self.done_dev[:, 1] = 1 - self.done_dev[:, 0]          # agent 1's flags are the complement: a record of the wrong agent shows
        self.records = tuple(dict(obs=torch.full((n, d), REC_SENTINEL, device="cuda"), act=torch.full((n, a), REC_SENTINEL, device="cuda"),
                                  nlp=torch.full((n,), REC_SENTINEL, device="cuda"), val=torch.full((n,), REC_SENTINEL, device="cuda"),
                                  done=torch.full((n,), DONE_SENTINEL, dtype=torch.uint8, device="cuda")) for d, a in zip(D, A))

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream


def _untouched(rec, rows=slice(None)):
    return all(bool((v[rows] == (DONE_SENTINEL if k == "done" else REC_SENTINEL)).all()) for k, v in rec.items())


def _written(rec, rows=slice(None)):
    return all(bool((v[rows] != (DONE_SENTINEL if k == "done" else REC_SENTINEL)).all()) for k, v in rec.items())


def _record_arg(rec, mode):
    if mode == "none":
        return None
    return {k: v for k, v in rec.items() if not (mode == "no-value" and k == "val")}


def _both(seats, rows, ntiles, noise, rec_modes, seed=0):
    """(fused, definition) runs on equal buffers: [(bufs, status)].  ``rows``: (rows of side 0, rows of side 1) or None."""
    n = 16 * ntiles
    tr = None if rows is None else tuple(None if r is None else torch.tensor(r, dtype=torch.int32, device="cuda") for r in rows)
    out = []
    for fused in (True, False):
        b = _Bufs(seats, n, seed)
        obs0 = b.obs_dev.clone()
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        co_train.pair_step(b, seats, tr, b.noise if noise else None, tuple(_record_arg(r, m) for r, m in zip(b.records, rec_modes)),
                           fused=fused, status=status)
        torch.cuda.synchronize()
        assert torch.equal(b.obs_dev, obs0)                    # the observations are read only
        out.append((b, int(status.item())))
    return out


def _assert_equal_runs(f, d):
    (bf, _), (bd, _) = f, d
    assert torch.equal(bf.act_dev, bd.act_dev)
    for s in range(2):
        for k in bf.records[s]:
            assert torch.equal(bf.records[s][k], bd.records[s][k]), (s, k)


def _forward(b, seat, side, rows, noise):
    """The definition spelled out: one ppo_forward per tile with that tile's row."""
    n, D, A = b.num_envs, seat.ob_dim, seat.ac_dim
    act = torch.empty((n, A), device="cuda"); nlp = torch.empty(n, device="cuda"); val = torch.empty(n, device="cuda")
    for t in range(n // 16):
        r = 0 if rows is None else rows[t]
        sl = slice(16 * t, 16 * t + 16)
        ppo_capi.chk(ppo_capi.lib().ppo_forward(seat.table[r].data_ptr(), b.obs_dev[sl, side].data_ptr(), 16, b.obs_dev.stride(0), D, A,
                                                ppo_capi.FWD_PI | ppo_capi.FWD_VF, b.noise[side][sl].data_ptr() if noise else None, None,
                                                act[sl].data_ptr(), nlp[sl].data_ptr(), val[sl].data_ptr(), None, b._stream()))
    torch.cuda.synchronize()
    return act, nlp, val


SHAPES = [("16-row-null", None, 1), ("16-row0", ([0], [0]), 1), ("48-rows", ([0, 2, 1], [1, 0, 2]), 3), ("48-null-one-side", (None, [1, 0, 2]), 3)]


@pytest.mark.parametrize("name,rows,ntiles", SHAPES, ids=[s[0] for s in SHAPES])
@pytest.mark.parametrize("sp0,sp1", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_pair_step_equals_its_definition(sp0, sp1, name, rows, ntiles):
    seats = (_seat(sp0, 0), _seat(sp1, 1))
    for noise in (True, False):
        for rec_mode in ("full", "no-value", "none"):
            f, d = _both(seats, rows, ntiles, noise, (rec_mode, rec_mode))
            _assert_equal_runs(f, d)
            b, status = f
            assert status == 0 and d[1] == 0
            for s, seat in enumerate(seats):
                D, A = seat.ob_dim, seat.ac_dim
                act, nlp, val = _forward(b, seat, s, None if rows is None else rows[s], noise)
                assert torch.equal(b.act_dev[:, s, :A], act)
                assert bool((b.act_dev[:, s, A:] == ACT_SENTINEL).all())          # action columns past the side's width
                rec = b.records[s]
                if rec_mode == "none":
                    assert _untouched(rec)
                    continue
                assert torch.equal(rec["obs"], b.obs_dev[:, s, :D]) and torch.equal(rec["done"], b.done_dev[:, s])      # the side's OWN flag
                assert torch.equal(rec["act"], act) and torch.equal(rec["nlp"], nlp)
                if rec_mode == "full":
                    assert torch.equal(rec["val"], val)
                else:
                    assert bool((rec["val"] == REC_SENTINEL).all())
                if not noise:
                    assert torch.isfinite(rec["nlp"]).all()


@pytest.mark.parametrize("rec_modes", [("full", "none"), ("none", "full"), ("no-value", "full")], ids=["side0", "side1", "mixed"])
def test_a_record_on_one_side_only(rec_modes):
    seats = (_seat("ant", 0), _seat("bug", 1))
    rows = ([0, 2, 1], [1, 0, 2])
    f, d = _both(seats, rows, 3, True, rec_modes)
    _assert_equal_runs(f, d)
    b, status = f
    assert status == 0
    for s, seat in enumerate(seats):
        act, nlp, val = _forward(b, seat, s, rows[s], True)
        assert torch.equal(b.act_dev[:, s, :seat.ac_dim], act)
        rec = b.records[s]
        if rec_modes[s] == "none":
            assert _untouched(rec)
        else:
            assert torch.equal(rec["act"], act) and torch.equal(rec["nlp"], nlp) and torch.equal(rec["done"], b.done_dev[:, s])
            assert torch.equal(rec["val"], val) if rec_modes[s] == "full" else bool((rec["val"] == REC_SENTINEL).all())


@pytest.mark.parametrize("bad_side", [0, 1])
@pytest.mark.parametrize("sp0,sp1", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_tile_without_a_table_row(sp0, sp1, bad_side):
    seats = (_seat(sp0, 0), _seat(sp1, 1))
    rows = [[0, 2, 1], [1, 0, 2]]
    rows[bad_side][1] = NROWS if bad_side == 0 else -1          # tile 1: one past the table / below it
    bad = slice(16, 32)
    f, d = _both(seats, rows, 3, True, ("full", "full"))
    _assert_equal_runs(f, d)                                   # the definition skips that run: everything else equals it
    b, status = f
    assert status == ppo_capi.mixed_status(1, bad_side) and ppo_capi.mixed_status_decode(status) == (1, bad_side) and d[1] == 0
    assert bool((b.act_dev[bad, bad_side] == ACT_SENTINEL).all()) and _untouched(b.records[bad_side], bad)
    for rng in (slice(0, 16), slice(32, 48)):
        assert bool((b.act_dev[rng, bad_side, :seats[bad_side].ac_dim] != ACT_SENTINEL).all()) and _written(b.records[bad_side], rng)
    other = 1 - bad_side                                        # the other side is complete
    act, nlp, val = _forward(b, seats[other], other, rows[other], True)
    assert torch.equal(b.act_dev[:, other, :seats[other].ac_dim], act) and torch.equal(b.records[other]["val"], val)
    assert torch.equal(b.records[other]["obs"], b.obs_dev[:, other, :seats[other].ob_dim])


@pytest.mark.parametrize("sp0,sp1", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_side_0_keeps_the_bits_of_ppo_mixed_step(sp0, sp1):
    """The launch that existed before, on the same buffers: its side 0 runs the same device function."""
    seats = (_seat(sp0, 0), _seat(sp1, 1))
    rows = ([2, 0, 1], [1, 0, 2])
    (b, status), _ = _both(seats, rows, 3, True, ("full", "full"))
    key = "zoo-" + sp1
    if key not in _CACHE:
        with np.load(os.path.join(HERE, "golden", "zoo_v3_params.npz"), allow_pickle=False) as z:
            _CACHE[key] = zoo_pairs.ZooSeat([z[sp1 + "-mlp-v3"].copy()], DIMS[sp1][0] - 1, DIMS[sp1][1], device=0)
    zseat = _CACHE[key]
    m = _Bufs(seats, 48, 0)                                    # the same seed: the same observations, noise and flags
    assert torch.equal(m.obs_dev, b.obs_dev) and torch.equal(m.noise[0], b.noise[0])
    mixed.mixed_step(m, seats[0], zseat, torch.zeros(3, dtype=torch.int32, device="cuda"), None, m.noise[0], None,
                     torch.tensor(rows[0], dtype=torch.int32, device="cuda"), m.records[0], fused=True)
    torch.cuda.synchronize()
    assert status == 0 and torch.equal(m.act_dev[:, 0], b.act_dev[:, 0])
    for k in m.records[0]:
        assert torch.equal(m.records[0][k], b.records[0][k]), k


def test_argument_errors_return_before_a_launch():
    seats = (_seat("ant", 0), _seat("bug", 1))
    n = 32
    b = _Bufs(seats, n, 3)
    L = ppo_capi.lib()
    obs, act, done = b.obs_dev, b.act_dev, b.done_dev
    status = torch.zeros(1, dtype=torch.int32, device="cuda")

    def sides(change_side=None, seat_kw=None, **kw):
        arr = (ppo_capi.PairSide * 2)()
        for s in range(2):
            p = arr[s]
            p.seat = seats[s].struct(None)
            p.obs, p.noise, p.done, p.action = obs[:, s].data_ptr(), b.noise[s].data_ptr(), done[:, s].data_ptr(), act[:, s].data_ptr()
            r = p.record
            r.obs, r.action, r.neglogp, r.value, r.done = (b.records[s][k].data_ptr() for k in mixed.RECORD_KEYS)
            if s == change_side:
                for k, v in (seat_kw or {}).items():
                    setattr(p.seat, k, v)
                for k, v in kw.items():
                    setattr(p, k, v)
        return arr

    def call(arr, n_=n, obs_stride=obs.stride(0), done_stride=2, act_stride=act.stride(0)):
        rc = L.ppo_mixed_pair_step(arr, n_, obs_stride, done_stride, act_stride, status.data_ptr(), b._stream())
        return rc, L.ppo_last_error().decode()

    messages, codes = set(), set()
    rc, msg = call(None)
    assert rc < 0 and msg
    messages.add(msg); codes.add(rc)
    for kw in (dict(n_=8), dict(n_=24), dict(n_=0)):
        rc, msg = call(sides(), **kw)
        assert rc < 0 and msg, kw
        messages.add(msg); codes.add(rc)
    for s in range(2):
        D, A, P = seats[s].ob_dim, seats[s].ac_dim, seats[s].P
        per_side = [(dict(seat_kw=dict(table=None)), {}), (dict(obs=None), {}), (dict(action=None), {}), (dict(seat_kw=dict(nrows=0)), {}),
                    (dict(seat_kw=dict(ob_dim=0)), {}), (dict(seat_kw=dict(ob_dim=513)), {}), (dict(seat_kw=dict(ac_dim=0)), {}),
                    (dict(seat_kw=dict(ac_dim=17)), {}), (dict(seat_kw=dict(row_stride=P - 1)), {}), ({}, dict(done_stride=0))]
        if s == 1:      # agent 1 is the wider side here: a stride below its widths (above agent 0's)
            per_side += [({}, dict(obs_stride=D - 1)), ({}, dict(act_stride=A - 1))]
        else:           # agent 0's widths made wider than the strides
            per_side += [(dict(seat_kw=dict(ob_dim=obs.stride(0) + 1)), {}), (dict(seat_kw=dict(ac_dim=16)), dict(act_stride=15))]
        for skw, ckw in per_side:
            arr = sides(s, **skw) if skw else sides()
            if "done_stride" in ckw and s == 1:                 # only this side gives flags: the refusal must name it
                arr[0].done = None
            rc, msg = call(arr, **ckw)
            assert rc < 0 and ("side %d" % s) in msg, (s, skw, ckw, msg)
            messages.add(msg); codes.add(rc)
    assert len(codes) == 11 and len(messages) >= 2 + 2 * 9      # every kind of refusal has its own code, every side its own message
    torch.cuda.synchronize()
    assert bool((b.act_dev == ACT_SENTINEL).all()) and int(status.item()) == 0 and all(_untouched(r) for r in b.records)
    rc, _ = call(sides())                                       # the same call without a fault goes through
    torch.cuda.synchronize()
    assert rc == 0 and int(status.item()) == 0 and all(_written(r) for r in b.records)
    assert bool((b.act_dev[:, 0, :8] != ACT_SENTINEL).all()) and bool((b.act_dev[:, 1, :12] != ACT_SENTINEL).all())
