"""CPU-side checks of the fused rollout launches of a recurrent learner against policy-zoo nets (sumo_rollout_steps_lstm_zoo /
sumo_rollout_steps_lstm_zoo_lstm): the library's exports, the header's declarations, the bindings above them, and the launch
structs they take, whose ctypes mirrors keep their fields (the entry points reuse sumo_rollout_lstm, sumo_zoo_mlp and sumo_zoo_lstm
as they are)."""
import ctypes as C
import os
import re

from conftest import ROOT
from robosumo_selfplay_amd import build, capi, lstm_model, runner, vec_env

ENTRIES = ("sumo_rollout_steps_lstm_zoo", "sumo_rollout_steps_lstm_zoo_lstm")


def test_library_exports_the_lstm_zoo_rollout_entry_points():
    build.build_all()
    L = C.CDLL(build.lib_path("libsumo_hip.so"))
    for n in ENTRIES:
        assert n in capi.EXPORTS and hasattr(L, n), n
    for n in ("rollout_steps_lstm_zoo", "rollout_steps_lstm_zoo_lstm"):
        assert callable(getattr(capi.Engine, n, None)), n
        assert callable(getattr(vec_env.SumoVecEnv, n + "_group", None)), n


def test_header_declares_the_lstm_zoo_rollout_entry_points():
    with open(os.path.join(ROOT, "include", "sumo_hip.h")) as f:
        h = f.read()
    for n, zoo in zip(ENTRIES, ("sumo_zoo_mlp", "sumo_zoo_lstm")):
        m = re.search(r"\bint %s\(([^;]*)\);" % n, h)
        assert m, n
        args = " ".join(m.group(1).split())
        assert args.startswith("sumo_handle_t h, const sumo_rollout_lstm* r, const %s* z, float* actions_dev" % zoo), args
        assert args.endswith("void* stream")


def test_launch_struct_mirrors_are_unchanged():
    names = lambda S: [f[0] for f in S._fields_]
    tail = ["T", "Ntot", "env_offset", "s0", "K", "alpha", "noise0", "noise1", "obs", "act", "rew", "val", "nlp", "onlp", "done",
            "ep_done", "ep_r", "ep_l"]
    assert names(capi.RolloutLstm) == ["learner", "opponents_dev", "tile_net_dev", "npool", "state0", "state1"] + tail
    assert names(capi.ZooMlp) == ["params", "filt", "obs_clip", "nzoo", "ob_dim"]
    assert names(capi.ZooLstm) == ["params", "filt", "state", "obs_clip", "forget_bias", "nzoo", "ob_dim", "emb_dim", "hidden"]
    assert (C.sizeof(capi.RolloutLstm), C.sizeof(capi.ZooMlp), C.sizeof(capi.ZooLstm)) == (176, 32, 48)


def test_runner_has_the_lstm_zoo_paths():
    for name in ("lstm_zoo_opponent", "fused_lstm_zoo_ok", "rollout_mode", "fused_steps", "_launch_steps", "_evaluate_step"):
        assert callable(getattr(runner.Runner, name, None)), name
    # the pairs (LSTM learner, zoo net of either family) resolve to the two launches
    for family, entry in zip(("mlp", "lstm"), ENTRIES):
        la = runner.rollout_launch("lstm", "zoo", family)
        assert (la.entry, la.struct, la.selector) == (entry[len("sumo_"):] + "_group", "RolloutLstm", "tile_net_dev")
    assert callable(getattr(lstm_model.LstmPPOModel, "score_and_value", None))
