"""CPU-side checks of the fused launches against policy-zoo MLP nets (sumo_rollout_steps_zoo / sumo_match_steps_zoo): the host
rows of the device table (policy_zoo.zoo_table_rows), the ctypes mirror of ``sumo_zoo_mlp`` against the C compiler's layout, the
library's exports and the batching of matches.evaluate_history_against_zoo."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from robosumo_selfplay_amd import build, capi, matches, policy_zoo
from robosumo_selfplay_amd.policies import flatten_params

HERE = os.path.dirname(os.path.abspath(__file__))


def _synthetic_flat(D, A, seed):
    """A zoo-shaped vector with a non-trivial observation filter (counts, sums) and O(1) weights (as tests/test_gpu_zoo.py)."""
    rng = np.random.default_rng(seed)
    sh = policy_zoo.zoo_mlp_shapes(D, A)
    cnt = 1000.0
    parts = []
    for k in policy_zoo._ZOO_MLP_ORDER:
        s = sh[k]
        if k.endswith("/count"):
            v = np.array(cnt)
        elif k.endswith("/sum"):
            v = cnt * rng.normal(0, 0.5, s)
        elif k.endswith("/sumsq"):
            v = cnt * (0.25 + rng.uniform(0.0, 2.0, s))          # some variances below the 1e-2 floor after - mean^2
        elif k == "logstd":
            v = rng.normal(-1.0, 0.3, s)
        elif k.endswith("/w"):
            v = rng.normal(0, 1.0 / np.sqrt(s[0]), s)
        else:
            v = rng.normal(0, 0.1, s)
        parts.append(np.asarray(v, np.float32).ravel())
    return np.concatenate(parts)


def _golden_v3():
    with np.load(os.path.join(HERE, "golden", "zoo_v3_params.npz"), allow_pickle=False) as z:
        return z["ant-mlp-v3"].copy()


def _expected_rows(flat, A):
    D, p = policy_zoo.split_zoo_mlp(flat, A)
    row = flatten_params([p["polfc1/w"], p["polfc1/b"], p["polfc2/w"], p["polfc2/b"], p["vffc1/w"], p["vffc1/b"], p["vffc2/w"],
                          p["vffc2/b"], p["polfinal/w"], p["polfinal/b"], p["logstd"], p["vffinal/w"], p["vffinal/b"]])
    mean, std = policy_zoo.filter_stats(p, "obsfilter")
    return D, row, mean, (np.float32(1.0) / std).astype(np.float32)


def test_zoo_table_rows_follow_the_policy_flattening_and_filter():
    A = 8
    for flats in ([_golden_v3()], [_synthetic_flat(120, A, 3), _synthetic_flat(120, A, 4)]):
        params, filt = policy_zoo.zoo_table_rows(flats, A)
        assert params.dtype == np.float32 and filt.dtype == np.float32
        for k, f in enumerate(flats):
            D, row, mean, invstd = _expected_rows(f, A)
            assert params.shape == (len(flats), row.size) and filt.shape == (len(flats), 2, D)
            assert row.size == 2 * (D * 64 + 64 + 64 * 64 + 64) + 64 * A + 2 * A + 64 + 1      # sumo_ppo.h layout for (D, A)
            assert np.array_equal(params[k], row)
            assert np.array_equal(filt[k, 0], mean) and np.array_equal(filt[k, 1], invstd)
    # the synthetic filter exercises the variance floor: 1 / sqrt(1e-2) = 10
    _, filt = policy_zoo.zoo_table_rows([_synthetic_flat(120, A, 3)], A)
    assert np.isclose(filt[0, 1].max(), 10.0)


def test_zoo_table_rows_refuse_lstm_and_mixed_widths():
    A = 8
    sh = policy_zoo.zoo_lstm_shapes(120, A)
    lstm_flat = np.zeros(sum(int(np.prod(s)) for s in sh.values()), np.float32)
    with pytest.raises(ValueError, match="LSTM"):
        policy_zoo.zoo_table_rows([lstm_flat], A)
    with pytest.raises(ValueError, match="ob_dim"):
        policy_zoo.zoo_table_rows([_synthetic_flat(120, A, 1), _synthetic_flat(100, A, 2)], A)
    with pytest.raises(ValueError):
        policy_zoo.zoo_table_rows([np.zeros(17, np.float32)], A)


def test_zoo_struct_mirror_matches_the_header(tmp_path):
    """Size and field offsets of capi.ZooMlp against ``sumo_zoo_mlp`` as gcc lays it out (the method of test_capi_layout.py)."""
    st, cname = capi.ZooMlp, "sumo_zoo_mlp"
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


def test_library_exports_the_zoo_entry_points():
    build.build_all()
    L = C.CDLL(build.lib_path("libsumo_hip.so"))
    for n in ("sumo_rollout_steps_zoo", "sumo_match_steps_zoo"):
        assert n in capi.EXPORTS and hasattr(L, n), n


def test_zoo_evaluation_plan():
    # 3 checkpoints x 2 opponents, 64 games each on 64 envs: one pair per batch, 64 envs x 1 round
    p = matches.plan_zoo_evaluation(3, 2, 64, 64)
    assert p["pairs"] == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)]
    assert (p["envs_per_pair"], p["rounds_per_env"]) == (64, 1)
    assert p["blocks"] == [(b, 0, 64) for b in range(6)]
    # 256 envs: four pairs share the first batch, the other two the second
    p = matches.plan_zoo_evaluation(3, 2, 64, 256)
    assert (p["envs_per_pair"], p["rounds_per_env"]) == (64, 1)
    assert p["blocks"] == [(0, 0, 64), (0, 64, 128), (0, 128, 192), (0, 192, 256), (1, 0, 64), (1, 64, 128)]
    # 100 games on 64 envs: the largest divisor of 100 that fits is 50 envs x 2 rounds; one pair per batch
    p = matches.plan_zoo_evaluation(2, 1, 100, 64)
    assert (p["envs_per_pair"], p["rounds_per_env"]) == (50, 2)
    assert p["envs_per_pair"] * p["rounds_per_env"] == 100
    assert p["blocks"] == [(0, 0, 50), (1, 0, 50)]
    # a prime number of games larger than the env count runs on one env
    assert matches.plan_zoo_evaluation(1, 1, 67, 64)["envs_per_pair"] == 1
    with pytest.raises(ValueError):
        matches.plan_zoo_evaluation(0, 1, 8, 8)
    # the plan is what env_assignment lays out
    p = matches.plan_zoo_evaluation(2, 2, 4, 8)
    idx0, idx1, active = matches.env_assignment(p["pairs"], [0, 1], p["envs_per_pair"], 8)
    assert idx0.tolist() == [0] * 8 and idx1.tolist() == [0, 0, 0, 0, 1, 1, 1, 1] and active.all()


def test_select_checkpoints():
    assert matches.select_checkpoints(["00000", "00002", "00001", "00004"]) == [0, 1, 2, 4]
    assert matches.select_checkpoints(["00000", "00002", "00001", "00004"], start=1) == [1, 2, 4]
    assert matches.select_checkpoints(range(10), start=1, interval=3) == [1, 4, 7]
    with pytest.raises(ValueError):
        matches.select_checkpoints([1], interval=0)
