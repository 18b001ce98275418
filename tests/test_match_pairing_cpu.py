"""CPU checks of the match pairing record (robosumo_selfplay_amd/matches.py ``match_pairing``): the seven
rows of the launch table, both cross seatings, what is refused, and the entry table of capi.py the rows are read from."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from robosumo_selfplay_amd import capi, matches, policies  # noqa: E402
from robosumo_selfplay_amd.lstm_model import LstmSpec  # noqa: E402

D, A = 121, 8


class _Zoo:
    """What a pairing reads of a policy_zoo.ZooTable."""
    recurrent, ac_dim, ob_dim, capacity = False, A, D - 1, 2


class _ZooLstm(_Zoo):
    """... of a policy_zoo.ZooLstmTable."""
    recurrent, hidden = True, 64


def _mlp():
    return matches.SnapshotTable(policies.PolicySpec(D, A, value_network="copy", activation="relu"), 3, "cpu")


def _lstm(H=128):
    return matches.LstmSnapshotTable(LstmSpec(D, A, H), 2, "cpu")


MT, LT, ZOO, ZL = _mlp(), _lstm(), _Zoo(), _ZooLstm()

# agent 0, agent 1 -> Engine entry, launch struct, second struct, lstm_side, families, state widths
ROWS = [
    (MT, MT, "match_steps", capi.Match, None, None, ("ckpt_mlp", "ckpt_mlp"), (None, None)),
    (LT, LT, "match_steps_lstm", capi.MatchLstm, None, None, ("ckpt_lstm", "ckpt_lstm"), (256, 256)),
    (MT, ZOO, "match_steps_zoo", capi.Match, capi.ZooMlp, None, ("ckpt_mlp", "zoo_mlp"), (None, None)),
    (MT, ZL, "match_steps_zoo_lstm", capi.Match, capi.ZooLstm, None, ("ckpt_mlp", "zoo_lstm"), (None, 128)),
    (LT, ZL, "match_steps_lstm_zoo_lstm", capi.MatchLstm, capi.ZooLstm, None, ("ckpt_lstm", "zoo_lstm"), (256, 128)),
    (MT, LT, "match_steps_cross", capi.MatchCross, None, 1, ("ckpt_mlp", "ckpt_lstm"), (None, 256)),
    (LT, MT, "match_steps_cross", capi.MatchCross, None, 0, ("ckpt_lstm", "ckpt_mlp"), (256, None)),
    (LT, ZOO, "match_steps_lstm_zoo", capi.MatchLstm, capi.ZooMlp, None, ("ckpt_lstm", "zoo_mlp"), (256, None)),
]


@pytest.mark.parametrize("t0,t1,entry,struct,second,lstm_side,families,widths", ROWS)
def test_pairing_resolves_to_the_row_of_the_table(t0, t1, entry, struct, second, lstm_side, families, widths):
    p = matches.match_pairing(t0, t1)
    assert (p.entry, p.struct, p.second, p.lstm_side) == (entry, struct, second, lstm_side)
    assert p.seats[0].table is t0 and p.seats[1].table is t1
    assert tuple(s.family for s in p.seats) == families and tuple(s.width for s in p.seats) == widths
    assert p.nlstm == (128 if "ckpt_lstm" in families else None)
    assert callable(getattr(capi.Engine, entry)) and "sumo_" + entry in capi.EXPORTS
    assert struct in matches._FILL and all(f in matches._FORWARD for f in families)


def test_pairing_reads_the_width_of_the_checkpoints():
    l64 = _lstm(64)
    for t0, t1, widths in ((l64, l64, (128, 128)), (l64, MT, (128, None)), (MT, l64, (None, 128)), (l64, ZL, (128, 128)), (l64, ZOO, (128, None))):
        p = matches.match_pairing(t0, t1)
        assert p.nlstm == 64 and tuple(s.width for s in p.seats) == widths
        with pytest.raises(ValueError, match=r"LSTM\(128\) policies only \(got LSTM\(64\)\): use fused=False"):
            matches._refuse_fused_width(p.nlstm)
    matches._refuse_fused_width(128)
    matches._refuse_fused_width(None)


def test_refused_pairs_of_seats():
    for zoo in (ZOO, ZL):
        for other in (MT, LT, ZOO, ZL):
            with pytest.raises(ValueError, match="zoo nets play agent 1 only"):
                matches.match_pairing(zoo, other)
    for t0, t1 in ((MT, _mlp()), (LT, _lstm())):
        with pytest.raises(ValueError, match="two tables of one family"):
            matches.match_pairing(t0, t1)
    with pytest.raises(ValueError, match=r"mixed LSTM widths.*LSTM\(128\) against LSTM\(64\)"):
        matches.match_pairing(LT, _lstm(64))


def test_the_record_is_immutable():
    p = matches.match_pairing(MT, LT)
    for obj, field in ((p, "entry"), (p, "lstm_side"), (p.seats[1], "table"), (p.seats[1], "width")):
        with pytest.raises(AttributeError):
            setattr(obj, field, None)
    assert isinstance(p.seats, tuple) and p == matches.match_pairing(MT, LT)


def test_state_check_names_the_seat():
    import torch
    p = matches.match_pairing(LT, ZL)
    ok0, ok1 = torch.zeros((4, 256)), torch.zeros((4, 128))
    matches._check_state(p.seats[0], ok0, 4)
    matches._check_state(p.seats[1], ok1, 4)
    matches._check_state(matches.match_pairing(MT, MT).seats[0], None, 4)
    with pytest.raises(ValueError, match=r"recurrent states must be two contiguous float32 \[4\]\[256\]"):
        matches._check_state(p.seats[0], ok1, 4)
    with pytest.raises(ValueError, match=r"zoo nets' recurrent state must be a contiguous float32 \[4\]\[128\]"):
        matches._check_state(p.seats[1], torch.zeros((4, 256))[:, ::2], 4)


def test_exports_are_the_parents_tuple():
    assert capi.EXPORTS == (
        "sumo_last_error", "sumo_create", "sumo_destroy", "sumo_dims", "sumo_reset", "sumo_step", "sumo_rollout_steps",
        "sumo_rollout_steps_lstm", "sumo_match_steps", "sumo_match_steps_lstm", "sumo_rollout_steps_zoo", "sumo_match_steps_zoo",
        "sumo_match_steps_zoo_lstm", "sumo_match_steps_lstm_zoo_lstm", "sumo_rollout_steps_zoo_lstm", "sumo_rollout_steps_lstm_zoo",
        "sumo_rollout_steps_lstm_zoo_lstm", "sumo_rollout_steps_zoo_league", "sumo_rollout_steps_lstm_zoo_league", "sumo_match_steps_cross",
        "sumo_match_steps_lstm_zoo", "sumo_rollout_steps_lstm_reuse", "sumo_set_cfrc_mode", "sumo_get_cfrc_ext", "sumo_set_adjust_z",
        "sumo_get_state", "sumo_set_state", "sumo_debug_forward", "sumo_stats", "sumo_profile", "sumo_debug_trace", "sumo_rollout_status",
        "sumo_debug_fault", "sumo_static_layout", "sumo_debug_layout", "sumo_debug_model_ints", "sumo_debug_dump")
    assert isinstance(capi.EXPORTS, tuple)


def test_entry_table_follows_the_header():
    """Every fused entry is declared in include/sumo_hip.h with the structs of the table, in its order."""
    import re
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sumo_hip.h")).read(), flags=re.S)
    c_name = {capi.Rollout: "sumo_rollout", capi.RolloutLstm: "sumo_rollout_lstm", capi.RolloutLstmReuse: "sumo_rollout_lstm_reuse",
              capi.Match: "sumo_match", capi.MatchLstm: "sumo_match_lstm", capi.MatchCross: "sumo_match_cross", capi.ZooMlp: "sumo_zoo_mlp",
              capi.ZooLstm: "sumo_zoo_lstm", capi.ZooLeague: "sumo_zoo_league"}
    for name, (launch, second) in capi.FUSED_ENTRIES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, txt)
        assert m, name
        structs = re.findall(r"const\s+(sumo_\w+)\s*\*", m.group(1))
        assert structs == [c_name[t] for t in (launch, second) if t is not None], name
