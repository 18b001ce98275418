"""CPU-side checks of the fused match launches against policy-zoo LSTM nets (sumo_match_steps_zoo_lstm /
sumo_match_steps_lstm_zoo_lstm): the host rows of the device table (policy_zoo.zoo_lstm_table_rows), the ctypes mirror of
``sumo_zoo_lstm`` against the C compiler's layout, the library's exports and the grouping of opponent files by family behind
matches.evaluate_history_against_zoo."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from zoo_lstm_helpers import golden, synthetic_lstm_flat
from robosumo_selfplay_amd import build, capi, matches, policy_zoo


def test_zoo_lstm_table_rows_hold_the_policy_branch_and_filter():
    A = 8
    flat = golden("ant-lstm-v3")
    D, p = policy_zoo.split_zoo_lstm(flat, A)
    params, filt = policy_zoo.zoo_lstm_table_rows([flat, synthetic_lstm_flat(D, A, 3)], A)
    assert params.dtype == np.float32 and filt.dtype == np.float32
    Pz = 64 * D + 64 + 128 * 256 + 256 + 64 * A + 2 * A                      # include/sumo_hip.h: sumo_zoo_lstm
    assert params.shape == (2, Pz) and filt.shape == (2, 2, D)
    o = 0
    for name, shape in (("p/emb/w", (D, 64)), ("p/emb/b", (64,)), ("lstmp/kernel", (128, 256)), ("lstmp/bias", (256,)),
                        ("p/out/w", (64, A)), ("p/out/b", (A,)), ("logstd", (1, A))):
        assert p[name].shape == shape, name
        n = int(np.prod(shape))
        assert np.array_equal(params[0, o:o + n], p[name].ravel()), name
        o += n
    assert o == Pz
    mean, std = policy_zoo.filter_stats(p, "obsfilter")
    assert np.array_equal(filt[0, 0], mean) and np.array_equal(filt[0, 1], (np.float32(1.0) / std).astype(np.float32))
    # the value branch is not in the row
    assert not np.isin(p["v/out/w"].ravel(), params[0]).all()


def test_zoo_lstm_table_rows_refusals():
    A = 8
    with pytest.raises(ValueError, match="MLP"):
        policy_zoo.zoo_lstm_table_rows([golden("ant-mlp-v3")], A)
    with pytest.raises(ValueError, match="ob_dim"):
        policy_zoo.zoo_lstm_table_rows([synthetic_lstm_flat(120, A, 1), synthetic_lstm_flat(100, A, 2)], A)
    with pytest.raises(ValueError, match="neither"):
        policy_zoo.zoo_lstm_table_rows([np.zeros(17, np.float32)], A)
    with pytest.raises(ValueError):
        policy_zoo.zoo_lstm_table_rows([], A)
    # the MLP table keeps refusing LSTM vectors
    with pytest.raises(ValueError, match="LSTM"):
        policy_zoo.zoo_table_rows([synthetic_lstm_flat(120, A, 1)], A)
    assert policy_zoo.zoo_file_kind(golden("ant-mlp-v3").size, A) == "mlp"
    assert policy_zoo.zoo_file_kind(golden("ant-lstm-v3").size, A) == "lstm"
    with pytest.raises(ValueError, match="neither"):
        policy_zoo.zoo_file_kind(17, A)
    # no length fits both families: the counts share their step per observation column and differ by 8 modulo it
    for A_ in (1, 8, 16):
        step = policy_zoo.zoo_mlp_param_count(1, A_) - policy_zoo.zoo_mlp_param_count(0, A_)
        assert step == policy_zoo.zoo_lstm_param_count(1, A_) - policy_zoo.zoo_lstm_param_count(0, A_) == 130
        assert (policy_zoo.zoo_lstm_param_count(0, A_) - policy_zoo.zoo_mlp_param_count(0, A_)) % step == 8


def test_zoo_lstm_struct_mirror_matches_the_header(tmp_path):
    """Size and field offsets of capi.ZooLstm against ``sumo_zoo_lstm`` as gcc lays it out (the method of
    test_zoo_struct_mirror_matches_the_header)."""
    st, cname = capi.ZooLstm, "sumo_zoo_lstm"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sumo_hip.h"', 'int main(void) {',
             '  printf("size %%zu\\n", sizeof(%s));' % cname]
    for fname, _ in st._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(%s, %s));' % (fname, cname, fname))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    table = dict((a, int(v)) for a, v in (ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True,
                                                                              text=True).stdout.splitlines()))
    assert C.sizeof(st) == table["size"]
    for fname, _ in st._fields_:
        assert getattr(st, fname).offset == table[fname], fname
    last = st._fields_[-1][0]
    assert getattr(st, last).offset + getattr(st, last).size + 8 > table["size"]     # every field of the header is mirrored


def test_library_exports_the_zoo_lstm_entry_points():
    build.build_all()
    L = C.CDLL(build.lib_path("libsumo_hip.so"))
    for n in ("sumo_match_steps_zoo_lstm", "sumo_match_steps_lstm_zoo_lstm"):
        assert n in capi.EXPORTS and hasattr(L, n), n


def test_mixed_zoo_evaluation_groups_plans_and_merges():
    kinds = ["lstm", "mlp", "lstm"]
    assert matches.group_zoo_opponents(kinds) == [("mlp", [1]), ("lstm", [0, 2])]
    assert matches.group_zoo_opponents(["lstm"]) == [("lstm", [0])]
    assert matches.group_zoo_opponents(["mlp", "mlp"]) == [("mlp", [0, 1])]
    with pytest.raises(ValueError):
        matches.group_zoo_opponents(["mlp", "gru"])
    ids = [5, 9]
    groups = matches.plan_mixed_zoo_evaluation(len(ids), kinds, 64, 128)
    assert [(g["kind"], g["opponents"]) for g in groups] == [("mlp", [1]), ("lstm", [0, 2])]
    for g in groups:                                                         # each family is planned on its own
        assert g["plan"] == matches.plan_zoo_evaluation(len(ids), len(g["opponents"]), 64, 128)
    # results of the groups (tagged by group, checkpoint, opponent of the group) come back under the caller's opponent numbers
    res = [[dict(wins=gi, losses=c, draws=64 - gi - c - o, rounds=64 - o, env_steps=100 * o) for c, o in g["plan"]["pairs"]]
           for gi, g in enumerate(groups)]
    out = matches.merge_zoo_results(ids, groups, res)
    assert list(out) == [(5, 0), (5, 1), (5, 2), (9, 0), (9, 1), (9, 2)]
    assert out[(5, 1)] == dict(win=0.0, draw=1.0, lose=0.0, rounds=64, env_steps=0)          # MLP group, checkpoint 0, its opponent 0
    assert out[(9, 2)]["rounds"] == 63 and out[(9, 2)]["env_steps"] == 100                      # LSTM group, its opponent 1
    assert out[(9, 2)]["win"] == 1 / 63.0 and out[(9, 2)]["lose"] == 1 / 63.0
    assert out[(9, 0)]["rounds"] == 64 and out[(9, 0)]["win"] == 1 / 64.0
