"""CPU checks of the cross-family matches (robosumo_selfplay_amd/matches.py; sumo_match_steps_cross / sumo_match_steps_lstm_zoo):
the C declaration of sumo_match_cross against its ctypes mirror, the exports, what the drivers refuse and let through before an env
exists, and play_cross_matches' seating and env-block assignment on a stand-in env."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import compare_versions  # noqa: E402
from robosumo_selfplay_amd import build, capi, matches, policies  # noqa: E402
from robosumo_selfplay_amd.lstm_model import LstmSpec  # noqa: E402

D, A = 120, 8      # Ant-vs-Ant


def _lstm_list(rng, H=128):
    return [rng.standard_normal(s).astype(np.float32) for s in policies.lstm_param_shapes(D, A, H)]


def _mlp_list(rng):
    return [rng.standard_normal(s).astype(np.float32) for s in policies.param_shapes(D, A)]


def _run_dir(tmp_path, name, plists):
    import joblib
    for v, pl in enumerate(plists):
        path = str(tmp_path / name / "checkpoints" / ("%.5i" % v))
        os.makedirs(os.path.dirname(path), exist_ok=True)
        joblib.dump(pl, path)
    return str(tmp_path / name)


# ---- the struct and the exports ------------------------------------------------------------------------------------------------
_CTYPES = {"int": C.c_int, "pointer": C.c_void_p}


def _declared_fields(struct):
    """[(name, 'int' | 'pointer')] of ``typedef struct <struct> { ... }`` in include/sumo_hip.h, in declaration order."""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sumo_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (struct, struct), txt, flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        first, *more = [d.strip() for d in decl.split(",")]
        m = re.match(r"^(?:const\s+)?([A-Za-z_]\w*)\s*(\**)\s*(\w+)$", first)
        assert m, decl
        base, stars, name = m.groups()
        assert stars or base == "int", decl                       # the struct holds ints and pointers only
        out.append((name, "pointer" if stars else base))
        for d in more:                                           # `type a, *b`: every further declarator carries its own stars
            mm = re.match(r"^(\**)\s*(\w+)$", d)
            assert mm, decl
            assert mm.group(1) or base == "int", decl
            out.append((mm.group(2), "pointer" if mm.group(1) else base))
    return out


def test_match_cross_mirror_follows_the_declaration():
    decl = _declared_fields("sumo_match_cross")
    assert [n for n, _ in decl] == ["params", "nsnap_mlp", "ob_dim", "ac_dim", "proto", "nets_dev", "nsnap_lstm", "state", "lstm_side",
                                    "idx0", "idx1", "T", "s0", "K", "quota", "noise0", "noise1", "score"]
    assert [(n, _CTYPES[t]) for n, t in decl] == list(capi.MatchCross._fields_)
    # the parser reads the struct the existing mirror was written for the same way
    assert [(n, _CTYPES[t]) for n, t in _declared_fields("sumo_match_lstm")] == list(capi.MatchLstm._fields_)


def test_cross_entry_points_are_declared_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sumo_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+sumo_match_steps_cross\s*\(\s*sumo_handle_t\s+\w+\s*,\s*const\s+sumo_match_cross\s*\*", txt)
    assert re.search(r"\bint\s+sumo_match_steps_lstm_zoo\s*\(\s*sumo_handle_t\s+\w+\s*,\s*const\s+sumo_match_lstm\s*\*\s*\w+\s*,\s*const\s+sumo_zoo_mlp\s*\*", txt)
    for name in ("sumo_match_steps_cross", "sumo_match_steps_lstm_zoo"):
        assert name in capi.EXPORTS
    assert callable(capi.Engine.match_steps_cross) and callable(capi.Engine.match_steps_lstm_zoo)
    lib = build.lib_path("libsumo_hip.so")
    assert os.path.exists(lib), "the library is built before the tests run"
    L = C.CDLL(lib)
    for name in ("sumo_match_steps_cross", "sumo_match_steps_lstm_zoo"):
        assert hasattr(L, name)


# ---- what the drivers refuse, and what reaches the env -------------------------------------------------------------------------
def test_cross_family_flag_opens_the_version_drivers(tmp_path, monkeypatch):
    rng = np.random.default_rng(2)
    mlp = _run_dir(tmp_path, "mlp", [_mlp_list(rng) for _ in range(3)])
    lstm = _run_dir(tmp_path, "lstm", [_lstm_list(rng) for _ in range(3)])
    lstm64 = _run_dir(tmp_path, "lstm64", [_lstm_list(rng, 64) for _ in range(3)])

    def no_env(*a, **k):
        raise AssertionError("an env was built")
    monkeypatch.setattr(matches, "_make_env", no_env)
    # with the flag both seatings pass the checks and reach the env
    for p1, p2 in ((mlp, lstm), (lstm, mlp)):
        with pytest.raises(AssertionError, match="env was built"):
            matches.compare_history_versions(p1, p2, 4, cross_family=True)
        with pytest.raises(AssertionError, match="env was built"):
            compare_versions.main(["--p1", p1, "--p2", p2, "--trials", "4", "--cross_family"])
    # mixed LSTM widths stay refused, before the env; so does LSTM(64) against MLP on the fused launch (it plays step by step)
    with pytest.raises(ValueError, match=r"LSTM\(128\).*LSTM\(64\)"):
        matches.compare_history_versions(lstm, lstm64, 4, cross_family=True)
    with pytest.raises(ValueError, match=r"LSTM\(128\) policies only.*fused=False"):
        matches.compare_history_versions(mlp, lstm64, 4, cross_family=True)
    with pytest.raises(AssertionError, match="env was built"):
        matches.compare_history_versions(mlp, lstm64, 4, cross_family=True, fused=False)
    # without the flag everything is refused as before
    for kw in ({}, {"cross_family": False}):
        with pytest.raises(ValueError, match=r"MLP\(64,64\).*LSTM\(128\).*same network"):
            matches.compare_history_versions(mlp, lstm, 4, **kw)
        with pytest.raises(ValueError, match=r"LSTM\(128\).*MLP\(64,64\).*same network"):
            matches.compare_history_versions(lstm, mlp, 4, **kw)
        with pytest.raises(ValueError, match=r"LSTM\(128\).*LSTM\(64\)"):
            matches.compare_history_versions(lstm, lstm64, 4, **kw)
    with pytest.raises(ValueError, match=r"MLP\(64,64\).*LSTM\(128\)"):
        compare_versions.main(["--p1", mlp, "--p2", lstm, "--trials", "4"])
    # the zoo evaluation builds its env before it looks at the opponent files, with and without the flag
    for kw in ({"cross_family": True}, {}):
        with pytest.raises(AssertionError, match="env was built"):
            matches.evaluate_history_against_zoo(lstm, [str(tmp_path / "agent-params-v3.npy")], 4, **kw)


class _FakeModel:
    obs_dims, act_dims, timestep_limit = (D, D), (A, A), 500


class _FakeEnv:
    """What _play_batches touches of a SumoVecEnv, on the CPU."""
    def __init__(self, N):
        import torch
        self.num_envs, self.device, self.model = N, torch.device("cpu"), _FakeModel()
        self.seeds, self.adjust_z, self.resets = np.zeros(N, np.uint64), -0.5, 0

    def reset_device(self):
        self.resets += 1


class _FakeZoo:
    recurrent, ac_dim, ob_dim, capacity = False, A, D - 1, 2


def _tables(rng, n_mlp=3, n_lstm=2, H=128):
    mt = matches.SnapshotTable(policies.PolicySpec(D, A, value_network="copy", activation="relu"), n_mlp, "cpu")
    for k in range(n_mlp):
        mt.set(k, _mlp_list(rng))
    lt = matches.LstmSnapshotTable(LstmSpec(D, A, H), n_lstm, "cpu")
    for k in range(n_lstm):
        lt.set(k, _lstm_list(rng, H))
    return mt, lt


def test_play_cross_matches_refusals():
    mt, lt = _tables(np.random.default_rng(3))
    env = _FakeEnv(8)
    with pytest.raises(ValueError, match="one SnapshotTable.*one LstmSnapshotTable"):
        matches.play_cross_matches(env, mt, mt, [(0, 1)], 1, 4)
    with pytest.raises(ValueError, match="one SnapshotTable.*one LstmSnapshotTable"):
        matches.play_cross_matches(env, lt, lt, [(0, 1)], 1, 4)
    # rows are checked against the table of their own seat: row 2 exists in the MLP table only
    with pytest.raises(ValueError, match=r"pair \(0, 2\)"):
        matches.play_cross_matches(env, mt, lt, [(0, 2)], 1, 4)
    with pytest.raises(ValueError, match=r"pair \(2, 0\)"):
        matches.play_cross_matches(env, lt, mt, [(2, 0)], 1, 4)
    _, lt64 = _tables(np.random.default_rng(4), H=64)
    with pytest.raises(ValueError, match=r"LSTM\(128\) policies only.*fused=False"):
        matches.play_cross_matches(env, mt, lt64, [(0, 1)], 1, 4)
    # the step functions refuse swapped tables and a seat outside {0, 1}
    import torch
    st, sc = torch.zeros((8, 256)), torch.zeros((8, 3), dtype=torch.int32)
    i = np.zeros(8, np.int32)
    with pytest.raises(ValueError, match="in this order"):
        matches.cross_match_steps_stepwise(env, lt, mt, 0, i, i, st, sc, 1, 1)
    with pytest.raises(ValueError, match="lstm_side"):
        matches.cross_match_steps_fused(env, mt, lt, 2, i, i, st, sc, 1, 1)
    with pytest.raises(ValueError, match="recurrent state"):
        matches.cross_match_steps_fused(env, mt, lt, 1, i, i, st[:, :128].contiguous(), sc, 1, 1)
    # play_against_zoo: the default keeps refusing an LSTM table against zoo MLP nets
    with pytest.raises(ValueError, match="zoo MLP nets"):
        matches.play_against_zoo(env, lt, _FakeZoo(), [(0, 0)], 1, 4)
    with pytest.raises(ValueError, match="zoo MLP nets"):
        matches.play_against_zoo(env, lt, _FakeZoo(), [(0, 0)], 1, 4, cross_family=False)
    with pytest.raises(ValueError, match=r"LSTM\(128\) policies only.*fused=False"):
        matches.play_against_zoo(env, lt64, _FakeZoo(), [(0, 0)], 1, 4, cross_family=True)


@pytest.mark.parametrize("lstm_first", [False, True])
def test_play_cross_matches_assigns_env_blocks_as_env_assignment(monkeypatch, lstm_first):
    """Pure planning: with the step driver replaced by a recorder, every batch hands over env_assignment's (idx0, idx1) for its
    pairs, the seat of the recurrent table, and a fresh zero state."""
    mt, lt = _tables(np.random.default_rng(5))
    N, epp = 10, 4                                               # two blocks per batch, two envs left over
    env = _FakeEnv(N)
    t0, t1 = (lt, mt) if lstm_first else (mt, lt)
    pairs = [(1, 2), (0, 1), (1, 0)] if lstm_first else [(2, 1), (1, 0), (0, 1)]
    calls = []

    def record(env_, pairing, states, idx0, idx1, score, quota, K, noise, fused):
        lstm_side = pairing.lstm_side
        assert pairing.seats[1 - lstm_side].table is mt and pairing.seats[lstm_side].table is lt
        assert quota == 2 and K == 16 and noise is None and fused is False
        state = states[lstm_side]
        assert states[1 - lstm_side] is None and tuple(state.shape) == (N, 256) and float(state.abs().sum()) == 0.0
        calls.append((lstm_side, np.array(idx0), np.array(idx1)))
        state.fill_(1.0)                                         # the next batch must not see it
        score[:, 0] = quota
    monkeypatch.setattr(matches, "pairing_steps", record)         # the one seam between the play drivers and the step paths
    res = matches.play_cross_matches(env, t0, t1, pairs, 2, epp, deterministic=True, chunk=16, fused=False)
    batches = matches.plan_batches(len(pairs), epp, N)
    assert [len(b) for b in batches] == [2, 1] and len(calls) == 2 and env.resets == 2
    for (side, i0, i1), batch in zip(calls, batches):
        e0, e1, _ = matches.env_assignment(pairs, batch, epp, N)
        assert side == (0 if lstm_first else 1)
        assert np.array_equal(i0, e0) and np.array_equal(i1, e1)
    assert [r["wins"] for r in res] == [2 * epp] * 3 and all(r["rounds"] == 2 * epp for r in res)
