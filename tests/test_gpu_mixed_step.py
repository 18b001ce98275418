"""``ppo_mixed_step`` (include/sumo_ppo.h) -- both seats of one step of a mixed match-up in one launch -- against its definition,
``mixed.mixed_step(fused=False)``: ``ppo_forward`` per run of tiles sharing a learner row, ``zoo_pairs.seat_act(fused=False)`` and
torch copies.  Plain buffers without an engine; obs / act rows wider than the widths, sentinels everywhere the kernel may not write.
Every comparison is ``torch.equal`` over whole tensors."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import has_gpu

pytestmark = pytest.mark.gpu
if has_gpu():
    import torch
    from robosumo_selfplay_amd import matches, mixed, ppo_capi, zoo_pairs

HERE = os.path.dirname(os.path.abspath(__file__))
ZOO_DIMS = {"ant": (120, 8), "bug": (164, 12), "spider": (208, 16)}        # what a zoo net reads / writes; a learner reads one column more
PAIRS = [("ant", "bug"), ("bug", "spider"), ("spider", "ant")]              # learner / seat
ACT_SENTINEL, STATE_SENTINEL, REC_SENTINEL, DONE_SENTINEL = 777.0, 555.0, 333.0, 99
NROWS = 3
_CACHE = {}


def _nets():
    if "nets" not in _CACHE:
        with np.load(os.path.join(HERE, "golden", "zoo_v3_params.npz"), allow_pickle=False) as z:
            _CACHE["nets"] = {k: z[k].copy() for k in z.files}
    return _CACHE["nets"]


def _zoo_seat(species):
    """[mlp 0, mlp 1, lstm 0]: table entries 0, 1, 2."""
    key = "zoo-" + species
    if key not in _CACHE:
        m, l = _nets()[species + "-mlp-v3"], _nets()[species + "-lstm-v3"]
        m1 = (m * (1.0 + 0.05 * np.random.default_rng(1).standard_normal(m.shape))).astype(np.float32)
        D, A = ZOO_DIMS[species]
        _CACHE[key] = zoo_pairs.ZooSeat([m, m1, l], D, A, device=0)
        assert _CACHE[key].entries.tolist() == [0, 1, 2]
    return _CACHE[key]


def _learner_seat(species):
    """Three distinct parameter rows of the species' MLP(64,64) policy (logstd away from zero, so the noise scale shows)."""
    key = "learner-" + species
    if key not in _CACHE:
        D, A = ZOO_DIMS[species][0] + 1, ZOO_DIMS[species][1]
        rng = np.random.default_rng(7)
        rows = [(0.1 * rng.standard_normal(matches.param_count(D, A))).astype(np.float32) for _ in range(NROWS)]
        _CACHE[key] = mixed.LearnerSeat(D, A, rows, device=0)
        assert len(_CACHE[key]) == NROWS and _CACHE[key].table.stride(0) == ppo_capi.lib().ppo_param_count(D, A)
    return _CACHE[key]


class _Bufs:
    """What ``mixed_step`` reads of an env, without an engine."""

    def __init__(self, lseat, zseat, n, seed, done_mode):
        g = torch.Generator(device="cuda").manual_seed(seed)
        D0, A0, D1, A1 = lseat.ob_dim, lseat.ac_dim, zseat.ob_dim, zseat.ac_dim
        self.num_envs, self.device = n, torch.device("cuda", 0)
        self.model = type("Model", (), {"obs_dims": (D0, D1 + 1), "act_dims": (A0, A1)})()
        self.spec = type("Spec", (), {"id": "buffers"})()
        self.obs_dev = 3.0 * torch.randn((n, 2, max(D0, D1) + 6), generator=g, device="cuda")
        self.act_dev = torch.full((n, 2, max(A0, A1) + 3), ACT_SENTINEL, device="cuda")
        self.noise0 = torch.randn((n, A0), generator=g, device="cuda")
        self.noise1 = torch.randn((n, A1), generator=g, device="cuda")
        self.state0 = 0.5 * torch.randn((n, 128), generator=g, device="cuda")
        self.done_dev = torch.zeros((n, 2), dtype=torch.uint8, device="cuda")
        if done_mode == "set":
            self.done_dev[:, 0] = 1
        elif done_mode == "mixed":
            self.done_dev[:, 0] = (torch.rand(n, generator=g, device="cuda") < 0.4).to(torch.uint8)
        self.done_dev[:, 1] = 1 - self.done_dev[:, 0]          # agent 1's flags are the complement: a wrong mask or record shows
        self.record = dict(obs=torch.full((n, D0), REC_SENTINEL, device="cuda"), act=torch.full((n, A0), REC_SENTINEL, device="cuda"),
                           nlp=torch.full((n,), REC_SENTINEL, device="cuda"), val=torch.full((n,), REC_SENTINEL, device="cuda"),
                           done=torch.full((n,), DONE_SENTINEL, dtype=torch.uint8, device="cuda"))

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def state(self, zseat, entries):
        s = self.state0.clone()
        for t, e in enumerate(entries):
            if not zseat.n_mlp <= e < zseat.n_mlp + zseat.n_lstm:
                s[16 * t:16 * t + 16] = STATE_SENTINEL
        return s


def _record_arg(b, mode):
    if mode == "none":
        return None
    return {k: v for k, v in b.record.items() if not (mode == "no-value" and k == "val")}


def _both(lseat, zseat, rows, entries, noise, rec_mode, done_mode, seed=0):
    """(fused, definition) runs on equal buffers: [(bufs, state, status)]."""
    n = 16 * len(entries)
    te = torch.tensor(entries, dtype=torch.int32, device="cuda")
    tr = None if rows is None else torch.tensor(rows, dtype=torch.int32, device="cuda")
    out = []
    for fused in (True, False):
        b = _Bufs(lseat, zseat, n, seed, done_mode)
        obs0 = b.obs_dev.clone()
        st = b.state(zseat, entries)
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        mixed.mixed_step(b, lseat, zseat, te, st, b.noise0 if noise else None, b.noise1 if noise else None, tr, _record_arg(b, rec_mode),
                         fused=fused, status=status)
        torch.cuda.synchronize()
        assert torch.equal(b.obs_dev, obs0)                    # the observations are read only
        out.append((b, st, int(status.item())))
    return out


def _assert_equal_runs(f, d):
    (bf, sf, _), (bd, sd, _) = f, d
    assert torch.equal(bf.act_dev, bd.act_dev) and torch.equal(sf, sd)
    for k in bf.record:
        assert torch.equal(bf.record[k], bd.record[k]), k


SHAPES = [("16-row-null-mlp", None, [0]), ("16-row0-lstm", [0], [2]), ("16-row-null-lstm", None, [2]), ("16-row0-mlp", [0], [0]),
          ("48-row-null", None, [0, 2, 1]), ("48-rows", [2, 0, 1], [0, 2, 1])]


@pytest.mark.parametrize("name,rows,entries", SHAPES, ids=[s[0] for s in SHAPES])
@pytest.mark.parametrize("learner,seat", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_mixed_step_equals_its_definition(learner, seat, name, rows, entries):
    lseat, zseat = _learner_seat(learner), _zoo_seat(seat)
    D0, A0, A1 = lseat.ob_dim, lseat.ac_dim, zseat.ac_dim
    n = 16 * len(entries)
    for noise in (True, False):
        for rec_mode in ("full", "none", "no-value"):
            for done_mode in ("clear", "set", "mixed"):
                f, d = _both(lseat, zseat, rows, entries, noise, rec_mode, done_mode)
                _assert_equal_runs(f, d)
                b, st, status = f
                assert status == 0
                # the definition once more, spelled out: one ppo_forward per tile with that tile's row
                act = torch.empty((n, A0), device="cuda"); nlp = torch.empty(n, device="cuda"); val = torch.empty(n, device="cuda")
                for t in range(len(entries)):
                    r = 0 if rows is None else rows[t]
                    sl = slice(16 * t, 16 * t + 16)
                    ppo_capi.chk(ppo_capi.lib().ppo_forward(lseat.table[r].data_ptr(), b.obs_dev[sl, 0].data_ptr(), 16, b.obs_dev.stride(0), D0, A0,
                                                            ppo_capi.FWD_PI | ppo_capi.FWD_VF, b.noise0[sl].data_ptr() if noise else None, None,
                                                            act[sl].data_ptr(), nlp[sl].data_ptr(), val[sl].data_ptr(), None, b._stream()))
                torch.cuda.synchronize()
                assert torch.equal(b.act_dev[:, 0, :A0], act)
                # sentinels: action columns past either side's width, state rows of MLP tiles
                assert bool((b.act_dev[:, 0, A0:] == ACT_SENTINEL).all()) and bool((b.act_dev[:, 1, A1:] == ACT_SENTINEL).all())
                assert bool((b.act_dev[:, 1, :A1] != ACT_SENTINEL).all())
                for t, e in enumerate(entries):
                    if e < zseat.n_mlp:
                        assert bool((st[16 * t:16 * t + 16] == STATE_SENTINEL).all())
                if rec_mode == "none":
                    assert all(bool((v == (DONE_SENTINEL if k == "done" else REC_SENTINEL)).all()) for k, v in b.record.items())
                else:
                    assert torch.equal(b.record["obs"], b.obs_dev[:, 0, :D0]) and torch.equal(b.record["done"], b.done_dev[:, 0])
                    assert torch.equal(b.record["act"], act) and torch.equal(b.record["nlp"], nlp)
                    if rec_mode == "full":
                        assert torch.equal(b.record["val"], val)
                    else:
                        assert bool((b.record["val"] == REC_SENTINEL).all())
                if not noise and rec_mode == "full":           # the mean: the action a noise-free ppo_forward gives has neglogp of z = 0
                    assert torch.isfinite(b.record["nlp"]).all()


@pytest.mark.parametrize("learner,seat", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_tile_without_a_table_row(learner, seat):
    lseat, zseat = _learner_seat(learner), _zoo_seat(seat)
    A0, A1 = lseat.ac_dim, zseat.ac_dim
    bad_tile = slice(16, 32)
    # a learner row equal to nrows on tile 1
    f, d = _both(lseat, zseat, [2, NROWS, 1], [0, 2, 1], True, "full", "mixed")
    _assert_equal_runs(f, d)                                   # the definition skips that run: every other tile equals it
    b, st, status = f
    assert status == ppo_capi.mixed_status(1, 0) and ppo_capi.mixed_status_decode(status) == (1, 0) and d[2] == 0
    assert bool((b.act_dev[bad_tile, 0] == ACT_SENTINEL).all()) and bool((b.act_dev[bad_tile, 1, :A1] != ACT_SENTINEL).all())
    for k, v in b.record.items():
        assert bool((v[bad_tile] == (DONE_SENTINEL if k == "done" else REC_SENTINEL)).all()), k
        assert bool((v[:16] != (DONE_SENTINEL if k == "done" else REC_SENTINEL)).all()), k
    assert bool((b.act_dev[:16, 0, :A0] != ACT_SENTINEL).all()) and bool((b.act_dev[32:, 0, :A0] != ACT_SENTINEL).all())
    # a zoo entry equal to n_mlp + n_lstm on tile 1
    f, d = _both(lseat, zseat, [2, 0, 1], [0, zseat.n_mlp + zseat.n_lstm, 2], True, "full", "mixed")
    _assert_equal_runs(f, d)
    b, st, status = f
    assert status == ppo_capi.mixed_status(1, 1) and ppo_capi.mixed_status_decode(status) == (1, 1)
    assert bool((b.act_dev[bad_tile, 1] == ACT_SENTINEL).all()) and bool((st[bad_tile] == STATE_SENTINEL).all())
    assert bool((b.act_dev[:, 0, :A0] != ACT_SENTINEL).all()) and not bool((st[32:] == STATE_SENTINEL).any())
    assert torch.equal(b.record["obs"], b.obs_dev[:, 0, :lseat.ob_dim])


def test_argument_errors_return_before_a_launch():
    lseat, zseat = _learner_seat("ant"), _zoo_seat("bug")
    n = 32
    b = _Bufs(lseat, zseat, n, 3, "mixed")
    te = torch.zeros(n // 16, dtype=torch.int32, device="cuda")
    st = torch.full((n, 128), STATE_SENTINEL, device="cuda")
    L = ppo_capi.lib()
    obs, act, done = b.obs_dev, b.act_dev, b.done_dev
    rec = ppo_capi.MixedRecord()
    rec.obs, rec.action, rec.neglogp, rec.value, rec.done = (b.record[k].data_ptr() for k in mixed.RECORD_KEYS)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")

    def call(ls=None, zs=None, null_learner=False, null_seat=False, **kw):
        a = dict(obs0=obs[:, 0].data_ptr(), obs1=obs[:, 1].data_ptr(), n=n, obs_stride=obs.stride(0), done=done.data_ptr(), done_stride=2,
                 act0=act[:, 0].data_ptr(), act1=act[:, 1].data_ptr(), act_stride=act.stride(0))
        a.update(kw)
        ls = lseat.struct(None) if ls is None else ls
        zs = zseat.struct(te, st) if zs is None else zs
        rc = L.ppo_mixed_step(None if null_learner else C.byref(ls), None if null_seat else C.byref(zs), a["obs0"], a["obs1"], a["n"],
                              a["obs_stride"], a["done"], a["done_stride"], b.noise0.data_ptr(), b.noise1.data_ptr(), a["act0"], a["act1"],
                              a["act_stride"], C.byref(rec), status.data_ptr(), b._stream())
        return rc, L.ppo_last_error().decode()

    def learner(**kw):
        s = lseat.struct(None)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def seat(**kw):
        s = zseat.struct(te, st)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    cases = [dict(null_learner=True), dict(ls=learner(table=None)), dict(obs0=None), dict(act0=None), dict(ls=learner(nrows=0)),
             dict(ls=learner(ob_dim=0)), dict(ls=learner(ob_dim=513)), dict(ls=learner(ac_dim=0)), dict(ls=learner(ac_dim=17)),
             dict(obs_stride=lseat.ob_dim - 1, zs=seat(ob_dim=8)), dict(act_stride=lseat.ac_dim - 1, zs=seat(ac_dim=2)),
             dict(ls=learner(row_stride=lseat.P - 1)), dict(null_seat=True), dict(obs1=None), dict(act1=None), dict(n=8), dict(n=24),
             dict(zs=seat(ob_dim=0)), dict(zs=seat(ob_dim=513)), dict(obs_stride=zseat.ob_dim - 1), dict(zs=seat(ac_dim=0)),
             dict(zs=seat(ac_dim=17)), dict(act_stride=zseat.ac_dim - 1), dict(zs=seat(n_mlp=0, n_lstm=0)), dict(zs=seat(mlp_params=None)),
             dict(zs=seat(lstm_filt=None)), dict(zs=seat(state=None)), dict(zs=seat(tile_entry=None)), dict(done_stride=0)]
    messages = set()
    for kw in cases:
        rc, msg = call(**kw)
        assert rc < 0 and msg, kw
        messages.add((rc, msg))
    assert len({rc for rc, _ in messages}) == 18 and len({m for _, m in messages}) >= 18      # every kind of refusal has its own code and message
    torch.cuda.synchronize()
    assert bool((b.act_dev == ACT_SENTINEL).all()) and bool((st == STATE_SENTINEL).all()) and int(status.item()) == 0
    assert all(bool((v == (DONE_SENTINEL if k == "done" else REC_SENTINEL)).all()) for k, v in b.record.items())
    rc, _ = call()                                             # the same call without a fault goes through
    torch.cuda.synchronize()
    assert rc == 0 and int(status.item()) == 0 and bool((b.act_dev[:, 0, :lseat.ac_dim] != ACT_SENTINEL).all())
