"""CPU checks of recurrent (LSTM) checkpoint matches (robosumo_selfplay_amd/matches.py, sumo_match_steps_lstm): the checkpoint kind
read from the array shapes, LstmSnapshotTable's accepted and refused inputs, the C declaration and the ctypes mirror of
sumo_match_lstm, and the refusal of MLP-vs-LSTM comparisons before anything touches the GPU."""
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


def _lstm_list(rng, H=128, d=D):
    return [rng.standard_normal(s).astype(np.float32) for s in policies.lstm_param_shapes(d, A, H)]


def _mlp_list(rng):
    return [rng.standard_normal(s).astype(np.float32) for s in policies.param_shapes(D, A)]


def _save(path, plist):
    """What LstmPPOModel.save / PPOModel.save write: joblib.dump of the parameter list."""
    import joblib
    os.makedirs(os.path.dirname(path), exist_ok=True)
    joblib.dump(plist, path)
    return path


def test_checkpoint_kind_reads_the_array_shapes(tmp_path):
    rng = np.random.default_rng(0)
    assert matches.checkpoint_kind(_save(str(tmp_path / "m"), _mlp_list(rng))) == ("mlp", None)
    assert matches.checkpoint_kind(_save(str(tmp_path / "l"), _lstm_list(rng))) == ("lstm", 128)
    assert matches.checkpoint_kind(_save(str(tmp_path / "l64"), _lstm_list(rng, 64))) == ("lstm", 64)
    with pytest.raises(ValueError, match="neither"):
        matches.checkpoint_kind(_save(str(tmp_path / "x"), [np.zeros(3, np.float32)]))


def test_lstm_table_accepts_lstm_checkpoints_and_refuses_others(tmp_path):
    rng = np.random.default_rng(1)
    t = matches.LstmSnapshotTable(LstmSpec(D, A, 128), 3, "cpu")
    assert t.recurrent and not t.filled.any()
    plist = _lstm_list(rng)
    flat = np.concatenate([p.ravel() for p in plist])
    p = _save(str(tmp_path / "00001"), plist)
    t.set(0, p)
    assert np.array_equal(t.params[0].numpy(), flat) and t.labels[0] == p
    t.set(1, plist)
    t.set(2, flat)
    assert np.array_equal(t.params[1].numpy(), flat) and np.array_equal(t.params[2].numpy(), flat) and t.filled.all()
    # every net of the device array addresses its own row: wx at the row start, vf_b at its end
    P = t.P
    for k in range(3):
        n = t.nets[k]
        assert (n.hidden, n.ob_dim, n.ac_dim, n.emb_dim, n.emb_w, n.obs_mean) == (128, D, A, 0, None, None)
        assert n.wx == t.params[k].data_ptr() and n.vf_b == t.params[k].data_ptr() + 4 * (P - 1)
    assert bytes(t.nets) == t.nets_dev.numpy().tobytes()
    # an MLP checkpoint, another LSTM width, another observation width
    with pytest.raises(ValueError, match="MLP"):
        t.set(0, _save(str(tmp_path / "mlp"), _mlp_list(rng)))
    with pytest.raises(ValueError, match=r"LSTM\(64\)"):
        t.set(0, _save(str(tmp_path / "l64"), _lstm_list(rng, 64)))
    with pytest.raises(ValueError, match="does not match"):
        t.set(0, _lstm_list(rng, 128, D + 16))
    with pytest.raises(ValueError, match="parameters"):
        t.set(0, np.zeros(10, np.float32))
    with pytest.raises(IndexError):
        t.set(3, flat)

    class FakeMlpModel:
        params, spec = None, None
    with pytest.raises(ValueError, match="MLP"):
        t.set(0, FakeMlpModel())
    # the MLP table keeps refusing LSTM checkpoints with its own message
    with pytest.raises(ValueError, match="LSTM checkpoint"):
        matches.snapshot_vector(policies.PolicySpec(D, A, value_network="copy", activation="relu"), p)


def test_pool_and_table_fill_the_same_nets():
    from robosumo_selfplay_amd import ppo_capi
    from robosumo_selfplay_amd.opponent_pool import fill_lstm_net
    spec = LstmSpec(D, A, 128)
    n = fill_lstm_net(ppo_capi.LstmNet(), 4096, spec)
    sizes = [int(np.prod(s)) for s in policies.lstm_param_shapes(D, A, 128)]
    offs = 4096 + 4 * np.concatenate([[0], np.cumsum(sizes)])
    assert [n.wx, n.wh, n.b, n.head_w, n.head_b, n.logstd, n.vf_w, n.vf_b] == [int(o) for o in offs[:8]]
    assert (n.gate_order, n.forget_bias) == (ppo_capi.LSTM_GATES_IFOU, 0.0)


def _run_dir(tmp_path, name, plists):
    for v, pl in enumerate(plists):
        _save(str(tmp_path / name / "checkpoints" / ("%.5i" % v)), pl)
    return str(tmp_path / name)


def test_mixed_networks_are_refused_before_the_gpu(tmp_path, monkeypatch):
    rng = np.random.default_rng(2)
    mlp = _run_dir(tmp_path, "mlp", [_mlp_list(rng) for _ in range(3)])
    lstm = _run_dir(tmp_path, "lstm", [_lstm_list(rng) for _ in range(3)])
    lstm64 = _run_dir(tmp_path, "lstm64", [_lstm_list(rng, 64) for _ in range(3)])

    def no_env(*a, **k):
        raise AssertionError("an env was built before the refusal")
    monkeypatch.setattr(matches, "_make_env", no_env)
    with pytest.raises(ValueError, match=r"MLP\(64,64\).*LSTM\(128\)"):
        compare_versions.main(["--p1", mlp, "--p2", lstm, "--trials", "4"])
    with pytest.raises(ValueError, match=r"LSTM\(128\).*MLP\(64,64\)"):
        matches.compare_history_versions(lstm, mlp, 4)
    with pytest.raises(ValueError, match=r"LSTM\(128\).*LSTM\(64\)"):
        matches.compare_history_versions(lstm, lstm64, 4)
    # the same kinds pass the check and reach the env
    with pytest.raises(AssertionError, match="env was built"):
        matches.compare_history_versions(lstm, lstm, 4)
    with pytest.raises(AssertionError, match="env was built"):
        matches.round_robin(lstm, 1, 4)


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_lstm_match_entry_point_is_declared_and_exported():
    txt = _declared("sumo_hip.h")
    assert re.search(r"\bint\s+sumo_match_steps_lstm\s*\(\s*sumo_handle_t", txt)
    assert "typedef struct sumo_match_lstm" in txt
    assert "sumo_match_steps_lstm" in capi.EXPORTS
    lib = build.lib_path("libsumo_hip.so")
    if os.path.exists(lib):
        assert hasattr(C.CDLL(lib), "sumo_match_steps_lstm")
