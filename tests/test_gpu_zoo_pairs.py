"""Zoo-vs-zoo play on the GPU (robosumo_selfplay_amd/zoo_pairs.py, ``ppo_zoo_seat_act``): the one-launch seat
kernel against its definition -- the ``ppo_forward_filtered`` / ``ppo_lstm_step`` launches of ``seat_act(fused=False)``, which
tests/test_gpu_zoo*.py pin to the oracle -- bit for bit (``torch.equal``: both sides run one copy of the arithmetic, so there is no
tolerance), what the kernel leaves alone, its out-of-range entries, and the drivers built on it on a mixed scene."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT, has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch
    from robosumo_selfplay_amd import mjcf, render, zoo_pairs
    from robosumo_selfplay_amd.vec_env import SumoVecEnv
    import zoo_tournament

HERE = os.path.dirname(os.path.abspath(__file__))
DIMS = {"ant": (120, 8), "bug": (164, 12), "spider": (208, 16)}
ACT_SENTINEL, STATE_SENTINEL = 777.0, 555.0
_CACHE = {}


def _nets():
    if "nets" not in _CACHE:
        with np.load(os.path.join(HERE, "golden", "zoo_v3_params.npz"), allow_pickle=False) as z:
            _CACHE["nets"] = {k: z[k].copy() for k in z.files}
    return _CACHE["nets"]


def _variant(v, seed):
    """A second net of the same shape: every entry of the fixture vector scaled by 1 + 5 % noise."""
    return (v * (1.0 + 0.05 * np.random.default_rng(seed).standard_normal(v.shape))).astype(np.float32)


def _seat(species):
    """[mlp 0, mlp 1, lstm 0, lstm 1] of one species: table entries 0 .. 3."""
    if species not in _CACHE:
        m, l = _nets()[species + "-mlp-v3"], _nets()[species + "-lstm-v3"]
        D, A = DIMS[species]
        _CACHE[species] = zoo_pairs.ZooSeat([m, _variant(m, 1), l, _variant(l, 2)], D, A, device=0)
        assert _CACHE[species].entries.tolist() == [0, 1, 2, 3]
    return _CACHE[species]


class _Model:
    pass


class _Bufs:
    """The buffers ``seat_act`` reads of an env, without an engine: obs / act rows wider than the nets' widths, two agents per env, the
    seat under test on ``side``; everything it may not write holds a sentinel."""

    def __init__(self, seat, n, side, seed, done_mode):
        g = torch.Generator(device="cuda").manual_seed(seed)
        D, A = seat.ob_dim, seat.ac_dim
        self.num_envs, self.device, self.side = n, torch.device("cuda", 0), side
        self.model = _Model()
        self.model.obs_dims = (D + 1, D + 1)
        self.model.act_dims = (A, A)
        self.spec = type("Spec", (), {"id": "buffers"})()
        self.obs_dev = 3.0 * torch.randn((n, 2, D + 6), generator=g, device="cuda")        # some columns beyond the +-5 clip of the filter
        self.act_dev = torch.full((n, 2, A + 3), ACT_SENTINEL, device="cuda")
        self.noise = torch.randn((n, A), generator=g, device="cuda")
        self.state0 = 0.5 * torch.randn((n, 128), generator=g, device="cuda")
        self.done_dev = torch.zeros((n, 2), dtype=torch.uint8, device="cuda")              # (drawn last: one seed, one obs / noise / state)
        if done_mode == "ones":
            self.done_dev[:, 0] = 1
        elif done_mode == "mixed":
            self.done_dev[:, 0] = (torch.rand(n, generator=g, device="cuda") < 0.4).to(torch.uint8)
        self.done_dev[:, 1] = 1 - self.done_dev[:, 0]                                      # the other agent's flags are not the mask

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def state(self, seat, tile_entry):
        s = self.state0.clone()
        for t, e in enumerate(tile_entry):
            if not seat.n_mlp <= e < seat.n_mlp + seat.n_lstm:
                s[16 * t:16 * t + 16] = STATE_SENTINEL
        return s


def _both(seat, entries, side, noise, done_mode, seed=0, null_state=False):
    """(fused, definition) runs on equal buffers: ((act, state, obs, status), (act, state, obs))."""
    n = 16 * len(entries)
    te = torch.tensor(entries, dtype=torch.int32, device="cuda")
    out = []
    for fused in (True, False):
        b = _Bufs(seat, n, side, seed, done_mode)
        obs0 = b.obs_dev.clone()
        st = None if null_state else b.state(seat, entries)
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        zoo_pairs.seat_act(seat, b, side, te, st, b.noise if noise else None, fused=fused, status=status)
        torch.cuda.synchronize()
        assert torch.equal(b.obs_dev, obs0)                                               # the observations are read only
        out.append((b.act_dev, st, b, int(status.item())))
    return out


SHAPES = [("16-mlp", [0]), ("16-lstm", [2]), ("48-mixed", [0, 2, 1]), ("48-lstm", [3, 2, 3])]


@pytest.mark.parametrize("noise", [True, False], ids=["noise", "mean"])
@pytest.mark.parametrize("name,entries", SHAPES, ids=[s for s, _ in SHAPES])
@pytest.mark.parametrize("species", sorted(DIMS))
def test_seat_kernel_equals_its_definition(species, name, entries, noise):
    seat = _seat(species)
    A = seat.ac_dim
    for side, done_mode in ((0, "zeros"), (1, "ones"), (1, "mixed")):
        (af, sf, bf, status), (ad, sd, _, _) = _both(seat, entries, side, noise, done_mode, seed=len(entries) + side)
        assert status == 0
        assert torch.equal(af, ad) and torch.equal(sf, sd), (species, name, noise, done_mode)
        # the definition really acted: every action column of the seat is written, finite, and the LSTM rows moved
        assert torch.isfinite(af).all() and not (af[:, side, :A] == ACT_SENTINEL).any()
        # nothing else is written: the columns from ac_dim on, the other seat's rows, the state rows of MLP tiles
        assert (af[:, side, A:] == ACT_SENTINEL).all() and (af[:, 1 - side] == ACT_SENTINEL).all()
        for t, e in enumerate(entries):
            rows = slice(16 * t, 16 * t + 16)
            if e < seat.n_mlp:
                assert (sf[rows] == STATE_SENTINEL).all()
            else:
                assert torch.isfinite(sf[rows]).all() and not torch.equal(sf[rows], bf.state0[rows])


def test_lstm_rows_restart_where_the_previous_step_ended():
    """A row whose done flag is set gives what a zero state gives; the others what their own state gives."""
    seat = _seat("ant")
    entries = [2, 3]
    n = 32
    te = torch.tensor(entries, dtype=torch.int32, device="cuda")
    b = _Bufs(seat, n, 0, 3, "mixed")
    st = b.state0.clone()
    zoo_pairs.seat_act(seat, b, 0, te, st, b.noise)
    fin = b.done_dev[:, 0] != 0
    b2 = _Bufs(seat, n, 0, 3, "zeros")
    st2 = b2.state0.clone()
    st2[fin] = 0.0
    zoo_pairs.seat_act(seat, b2, 0, te, st2, b2.noise)
    torch.cuda.synchronize()
    assert 0 < int(fin.sum()) < n
    assert torch.equal(b.act_dev, b2.act_dev) and torch.equal(st, st2)


def test_mlp_only_seat_takes_no_state():
    m = _nets()["spider-mlp-v3"]
    seat = zoo_pairs.ZooSeat([m, _variant(m, 4)], 208, 16, device=0)
    (af, _, _, status), (ad, _, _, _) = _both(seat, [1, 0, 1], 1, True, "mixed", null_state=True)
    assert status == 0 and torch.equal(af, ad) and not (af[:, 1, :16] == ACT_SENTINEL).any()


@pytest.mark.parametrize("entries,bad", [([0, 4, 2], [1]), ([2, -1, 1], [1]), ([4, 0, -1], [0, 2]), ([2 ** 31 - 1], [0]), ([-2 ** 31], [0])])
def test_out_of_range_entries_write_nothing(entries, bad):
    seat = _seat("bug")
    A = seat.ac_dim
    (af, sf, bf, status), (ad, sd, _, _) = _both(seat, entries, 0, True, "mixed", seed=9)
    assert status in [1 + t for t in bad]
    assert torch.equal(af, ad) and torch.equal(sf, sd)                  # the definition skips such a tile
    for t in range(len(entries)):
        rows = slice(16 * t, 16 * t + 16)
        if t in bad:
            assert (af[rows] == ACT_SENTINEL).all() and (sf[rows] == STATE_SENTINEL).all()
        else:
            assert not (af[rows, 0, :A] == ACT_SENTINEL).any()


# ---- drivers ----------------------------------------------------------------------------------------------------------------
def _scene_seats(env, kinds0, kinds1):
    sp = zoo_tournament.species_of(env.spec.id)
    return tuple(zoo_pairs.seat_for(env, side, [_nets()["%s-%s-v3" % (sp[side], k)] for k in kinds])
                 for side, kinds in enumerate((kinds0, kinds1)))


def _near_time_limit(envs, K):
    """Episodes end (and auto-reset) at different steps inside the K steps played."""
    for g in range(envs[0].groups):
        qpos, qvel, warm, cnt = envs[0].engines[g].get_state()
        cnt[:, 0] = envs[0].model.timestep_limit - (K - 2) + (np.arange(len(cnt)) % (K - 3))
        for e in envs:
            e.engines[g].set_state(qpos, qvel, warm, cnt)


@pytest.mark.parametrize("env_id,N", [("RoboSumo-Ant-vs-Bug-v0", 32), ("RoboSumo-Spider-vs-Spider-v0", 16)])
def test_pair_steps_fused_equals_stepwise(env_id, N):
    K = 8
    ef, es = [SumoVecEnv(env_id, num_envs=N, seed=7, adjust_z=-0.5) for _ in range(2)]
    try:
        seats = _scene_seats(ef, ("mlp", "lstm"), ("lstm", "mlp"))
        assert [s.kinds for s in seats] == [["mlp", "lstm"], ["lstm", "mlp"]]
        env_net = np.repeat(np.arange(N // 16) % 2, 16) if N > 16 else np.ones(N, np.int64)
        tiles = tuple(torch.from_numpy(s.tile_entries(env_net)).cuda() for s in seats)
        g = torch.Generator(device="cuda").manual_seed(1)
        noise = tuple(torch.randn((K, N, s.ac_dim), generator=g, device="cuda") for s in seats)
        assert noise[0].shape[2] == ef.model.act_dims[0] and noise[1].shape[2] == ef.model.act_dims[1]
        res = []
        for e in (ef, es):
            e.reset_device()
        _near_time_limit([ef, es], K)
        for e, fused in ((ef, True), (es, False)):
            states = tuple(s.new_state(N) for s in seats)
            score = torch.zeros((N, 3), dtype=torch.int32, device="cuda")
            zoo_pairs.pair_steps(e, seats, tiles, states, score, 2, K, noise, fused=fused)
            torch.cuda.synchronize()
            res.append((e.obs_dev, e.done_dev, e.act_dev, states[0], states[1], score))
        for a, b in zip(*res):
            assert torch.equal(a, b)
        assert int(res[0][5].sum()) >= N                                 # every env finished an episode inside the K steps
        for s, te, st in zip(seats, tiles, res[0][3:5]):                 # the state rows of LSTM tiles moved, those of MLP tiles did not
            lstm_rows = (te >= s.n_mlp).repeat_interleave(16)
            assert bool((st[lstm_rows] != 0).any(1).all()) and not bool((st[~lstm_rows] != 0).any())
    finally:
        ef.close()
        es.close()


def test_pair_steps_reports_an_entry_without_a_net():
    env = SumoVecEnv("RoboSumo-Ant-vs-Bug-v0", num_envs=16, seed=0)
    try:
        seats = _scene_seats(env, ("mlp",), ("mlp", "lstm"))
        env.reset_device()
        tiles = (torch.zeros(1, dtype=torch.int32, device="cuda"), torch.full((1,), 2, dtype=torch.int32, device="cuda"))
        for fused in (True, False):
            score = torch.zeros((16, 3), dtype=torch.int32, device="cuda")
            with pytest.raises(ValueError, match="names no net"):
                zoo_pairs.pair_steps(env, seats, tiles, (None, seats[1].new_state(16)), score, 1, 1, None, fused=fused)
    finally:
        env.close()


def test_play_zoo_pairs_on_a_mixed_scene(tmp_path):
    env = SumoVecEnv("RoboSumo-Ant-vs-Bug-v0", num_envs=64, seed=0, adjust_z=0.25)
    try:
        seats = _scene_seats(env, ("mlp", "lstm"), ("lstm", "mlp"))
        pairs = [(0, 0), (0, 1), (1, 0), (1, 1)]
        play = lambda **kw: zoo_pairs.play_zoo_pairs(env, seats[0], seats[1], pairs, 1, 16, seed=5, **kw)
        first = play()
        assert len(first) == 4
        for r in first:
            assert r["rounds"] == 16 and r["wins"] + r["losses"] + r["draws"] == 16
            assert 0 < r["env_steps"] <= 16 * 64 * 8                     # at most 501 steps, in chunks of 64
        assert env.adjust_z == 0.25
        rec = str(tmp_path / "rec")
        assert play(record=rec, every=8) == first                        # the same seed, the same games; recording changes nothing
        assert play(fused=False) == first
        assert env.adjust_z == 0.25
        traj = render.load_trajectory(os.path.join(rec, "traj.npz"))
        nq = mjcf.load_model("RoboSumo-Ant-vs-Bug-v0").nq
        assert traj["qpos"].shape[1:] == (64, nq) and traj["qpos"].shape[0] == first[0]["env_steps"] // 16 // 8
        assert traj["env_id"] == "RoboSumo-Ant-vs-Bug-v0" and traj["every"] == 8 and traj["score"].shape == (64, 3)
        assert np.isfinite(traj["qpos"]).all()
        with pytest.raises(ValueError, match="non-existent zoo net"):
            zoo_pairs.play_zoo_pairs(env, seats[0], seats[1], [(0, 2)], 1, 16)
    finally:
        env.close()


def test_tournament_script_plays_the_demos_pair(tmp_path):
    zoo = tmp_path / "assets"
    for sp, fam in (("bug", "lstm"), ("ant", "mlp")):
        os.makedirs(str(zoo / sp / fam))
        np.save(str(zoo / sp / fam / "agent-params-v3.npy"), _nets()["%s-%s-v3" % (sp, fam)])
    out = str(tmp_path / "result.json")
    r = zoo_tournament.main(["--zoo", str(zoo), "--env", "RoboSumo-Bug-vs-Ant-v0", "--policy-names", "lstm", "mlp", "--param-versions", "3", "3",
                             "--max_episodes", "16", "--num_env", "16", "--out", out])
    with open(out) as f:
        js = json.load(f)
    assert js["env_id"] == "RoboSumo-Bug-vs-Ant-v0" and js["trials"] == 16 and js["kinds0"] == ["lstm"] and js["kinds1"] == ["mlp"]
    assert np.asarray(js["counts"]).shape == (1, 1, 3) and int(np.sum(js["counts"])) == 16
    assert js["counts"] == r["counts"] and js["labels0"] == [str(zoo / "bug" / "lstm" / "agent-params-v3.npy")]
    assert js["results"][0]["rounds"] == 16
