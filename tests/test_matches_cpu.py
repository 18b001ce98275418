"""CPU checks of the checkpoint-vs-checkpoint match feature (robosumo_selfplay_amd/matches.py, compare_versions.py, sumo_match_steps):
checkpoint listing and pairing against the reference's compare_history_version.py, env -> pair assignment, refusals, CLI arguments,
the C declaration, the export list and the ctypes mirror of sumo_match."""
import ctypes as C
import os
import re
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import compare_versions  # noqa: E402
from robosumo_selfplay_amd import build, capi, matches, policies  # noqa: E402

D, A = 120, 8      # Ant-vs-Ant


def _spec():
    return policies.PolicySpec(D, A, value_network="copy", activation="relu")


def _run(tmp_path, name, ids):
    ck = tmp_path / name / "checkpoints"
    ck.mkdir(parents=True)
    for i in ids:
        (ck / i).write_bytes(b"x")
    return str(tmp_path / name)


def test_listing_sorts_and_drops_the_initial_version(tmp_path):
    run = _run(tmp_path, "r", ["00003", "00000", "00010", "00001", "00002"])
    (tmp_path / "r" / "checkpoints" / "notes.txt").write_text("not a checkpoint")
    assert matches.list_checkpoints(run) == ["00001", "00002", "00003", "00010"]
    # the checkpoint directory itself is accepted as well
    assert matches.list_checkpoints(os.path.join(run, "checkpoints")) == ["00001", "00002", "00003", "00010"]
    # the reference: [f for f in listdir if f != '00000'].sort() -- the same order for zero-padded names
    ref = sorted(f for f in os.listdir(os.path.join(run, "checkpoints")) if f != "00000" and f.isdigit())
    assert matches.list_checkpoints(run) == ref


def test_pairing_is_index_wise_up_to_the_shorter_list(tmp_path):
    a = ["00001", "00002", "00003"]
    b = ["00005", "00006"]
    with pytest.warns(UserWarning, match="comparing the first 2"):
        assert matches.pair_versions(a, b) == [("00001", "00005"), ("00002", "00006")]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert matches.pair_versions(a, a) == list(zip(a, a))


def test_trials_split_and_env_blocks():
    assert matches.split_trials(50, 256) == (50, 1)
    assert matches.split_trials(500, 256) == (250, 2)
    assert matches.split_trials(7, 4) == (1, 7)
    for trials, n in [(50, 256), (500, 256), (12, 5), (1, 1)]:
        epp, rpe = matches.split_trials(trials, n)
        assert epp * rpe == trials and epp <= n
    pairs = [(0, 5), (1, 6), (2, 7), (3, 8), (4, 9)]
    batches = matches.plan_batches(len(pairs), 3, 10)
    assert batches == [[0, 1, 2], [3, 4]]
    assert sorted(p for b in batches for p in b) == list(range(len(pairs)))
    idx0, idx1, active = matches.env_assignment(pairs, batches[1], 3, 10)
    assert idx0.tolist() == [3, 3, 3, 4, 4, 4, 0, 0, 0, 0] and idx1.tolist() == [8, 8, 8, 9, 9, 9, 0, 0, 0, 0]
    assert active.tolist() == [True] * 6 + [False] * 4
    # blocks are contiguous: every pair's envs form one run
    idx0, idx1, _ = matches.env_assignment(pairs, batches[0], 3, 10)
    assert matches._runs(idx0) == [(0, 3, 0), (3, 6, 1), (6, 9, 2), (9, 10, 0)]
    with pytest.raises(ValueError):
        matches.plan_batches(2, 11, 10)


def test_snapshot_vectors_and_refusals(tmp_path):
    import joblib
    rng = np.random.default_rng(0)
    plist = [rng.standard_normal(s).astype(np.float32) for s in policies.param_shapes(D, A)]
    p = str(tmp_path / "00001")
    joblib.dump(plist, p)
    v = matches.snapshot_vector(_spec(), p)
    assert v.dtype == np.float32 and np.array_equal(v, policies.flatten_params(plist))
    assert np.array_equal(matches.snapshot_vector(_spec(), v), v)
    # LSTM checkpoints (LstmPPOModel.save) are refused with a clear error
    lp = str(tmp_path / "00002")
    joblib.dump([np.zeros(s, np.float32) for s in policies.lstm_param_shapes(D, A)], lp)
    with pytest.raises(ValueError, match="LSTM checkpoint"):
        matches.snapshot_vector(_spec(), lp)

    class FakeLstm:
        recurrent = True
    with pytest.raises(ValueError, match="recurrent"):
        matches.snapshot_vector(_spec(), FakeLstm())
    # a checkpoint of a policy with another observation width does not fit the table
    other = [np.zeros(s, np.float32) for s in policies.param_shapes(D + 16, A)]
    with pytest.raises(ValueError, match="does not match"):
        matches.snapshot_vector(_spec(), other)
    with pytest.raises(ValueError):
        matches.snapshot_vector(_spec(), np.zeros(10, np.float32))


def test_mixed_matchups_are_refused():
    class M:
        obs_dims, act_dims, timestep_limit = (120, 136), (8, 8), 500

    class Env:
        model, cfrc_mode = M(), "zero"

    class T:
        spec = _spec()
    with pytest.raises(ValueError, match="homogeneous"):
        matches._check_env(Env(), T())
    Env.model.obs_dims, Env.model.act_dims = (120, 120), (8, 8)
    matches._check_env(Env(), T())
    Env.cfrc_mode = "rne_post"
    with pytest.raises(ValueError, match="rne_post"):
        matches._check_env(Env(), T())


def test_cli_arguments():
    a = compare_versions.parse_args(["--p1", "x", "--p2", "y"])
    assert (a.p1, a.p2, a.round_robin, a.trials, a.deterministic, a.adjust_z) == ("x", "y", False, 10, False, -0.5)
    a = compare_versions.parse_args(["--path", "r", "--round_robin", "--interval", "3", "--trials", "20", "--num_env", "64",
                                     "--seed", "4", "--deterministic", "--adjust_z", "0"])
    assert (a.path, a.round_robin, a.interval, a.trials, a.num_env, a.seed, a.deterministic, a.adjust_z) == ("r", True, 3, 20, 64, 4, True, 0.0)
    for bad in (["--p1", "x"], [], ["--path", "r"], ["--round_robin", "--p1", "x", "--p2", "y"], ["--p1", "x", "--p2", "y", "--trials", "0"],
                ["--path", "r", "--round_robin", "--p1", "x"]):
        with pytest.raises(SystemExit):
            compare_versions.parse_args(bad)


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_match_entry_point_is_declared_and_exported():
    txt = _declared("sumo_hip.h")
    assert re.search(r"\bint\s+sumo_match_steps\s*\(\s*sumo_handle_t", txt)
    assert "typedef struct sumo_match" in txt
    assert "sumo_match_steps" in capi.EXPORTS
    lib = build.lib_path("libsumo_hip.so")
    if os.path.exists(lib):
        assert hasattr(C.CDLL(lib), "sumo_match_steps")
