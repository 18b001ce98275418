"""Leagues of policy-zoo nets (learn(opponent_mode='fix', fix_opponent_path=[files])), the parts that need no GPU: the tile
assignment plan, the entry encoding of include/sumo_hip.h ``sumo_zoo_league``, the per-member tally of episode records, what
``install_fixed_opponent`` builds for a string and for a list, ``run.py``'s repeated flag, and the ctypes mirror of the struct."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from robosumo_selfplay_amd import alg_ppo, capi, policy_zoo  # noqa: E402
from zoo_lstm_helpers import golden, synthetic_lstm_flat  # noqa: E402


# ---- assignment plan ----------------------------------------------------------------------------------------------------------
def test_plan_is_round_robin_over_tiles_and_rotates_per_update():
    p0 = policy_zoo.league_plan(3, 128)                               # 8 tiles
    assert p0.dtype == np.int32 and p0.tolist() == [0, 1, 2, 0, 1, 2, 0, 1]
    assert policy_zoo.league_plan(3, 128, 1).tolist() == [1, 2, 0, 1, 2, 0, 1, 2]
    assert policy_zoo.league_plan(3, 128, 3).tolist() == p0.tolist()  # the rotation is modulo the league's size
    # over nmembers consecutive updates every tile meets every member
    seen = np.stack([policy_zoo.league_plan(3, 128, u) for u in range(3)])
    assert all(sorted(seen[:, t]) == [0, 1, 2] for t in range(8))


@pytest.mark.parametrize("n,nenvs", [(1, 16), (4, 64), (3, 64), (6, 4096), (5, 80)])
def test_plan_has_every_member_when_tiles_suffice(n, nenvs):
    for off in range(n + 1):
        p = policy_zoo.league_plan(n, nenvs, off)
        assert p.shape == (nenvs // 16,) and sorted(set(p.tolist())) == list(range(n))
        counts = np.bincount(p, minlength=n)
        assert counts.max() - counts.min() <= 1


def test_plan_refusals_name_both_numbers():
    with pytest.raises(ValueError, match=r"3 members.*nenvs = 40"):
        policy_zoo.league_plan(3, 40)                                 # not a multiple of 16
    with pytest.raises(ValueError, match=r"5 members.*nenvs = 64 gives 4"):
        policy_zoo.league_plan(5, 64)                                 # fewer tiles than members
    with pytest.raises(ValueError, match="at least one"):
        policy_zoo.league_plan(0, 64)
    with pytest.raises(ValueError, match="at least one"):
        policy_zoo.load_zoo_league([], 8, 64)                         # an empty file list, before anything touches a device


# ---- entry encoding and grouping ----------------------------------------------------------------------------------------------
def test_entries_group_the_families_and_keep_their_order():
    e, nmlp, nlstm = policy_zoo.league_entries(["lstm", "mlp", "lstm", "mlp", "mlp"])
    assert (nmlp, nlstm) == (3, 2) and e.dtype == np.int32
    assert e.tolist() == [3, 0, 4, 1, 2]                              # MLP rows [0, 3) in file order, then the LSTM rows
    assert policy_zoo.league_entries(["mlp", "mlp"])[0].tolist() == [0, 1]
    assert policy_zoo.league_entries(["lstm", "lstm", "lstm"]) [0].tolist() == [0, 1, 2]      # one family: the table's own rows
    with pytest.raises(ValueError):
        policy_zoo.league_entries(["mlp", "gru"])


def test_families_are_read_from_the_vector_length():
    A = 8
    flats = [golden("ant-mlp-v3"), synthetic_lstm_flat(120, A, 1), golden("ant-lstm-v3"), synthetic_lstm_flat(120, A, 2)]
    kinds = [policy_zoo.zoo_file_kind(f.size, A) for f in flats]
    assert kinds == ["mlp", "lstm", "lstm", "lstm"]
    e, nmlp, nlstm = policy_zoo.league_entries(kinds)
    assert e.tolist() == [0, 1, 2, 3] and (nmlp, nlstm) == (1, 3)
    # the rows the two tables would hold, in the members' order within each family
    pm, _ = policy_zoo.zoo_table_rows([f for f, k in zip(flats, kinds) if k == "mlp"], A)
    pl, _ = policy_zoo.zoo_lstm_table_rows([f for f, k in zip(flats, kinds) if k == "lstm"], A)
    assert pm.shape[0] == 1 and pl.shape[0] == 3
    ref, _ = policy_zoo.zoo_lstm_table_rows([flats[2]], A)
    assert np.array_equal(pl[1], ref[0]) and not np.array_equal(pl[0], ref[0])


# ---- league_scores ------------------------------------------------------------------------------------------------------------
def test_league_scores_on_hand_made_records():
    T, N = 3, 48                                                      # 3 tiles
    d = np.zeros((T, N), bool); r = np.zeros((T, N)); l = np.zeros((T, N), np.int32)
    def ep(t, e, ret, length):
        d[t, e], r[t, e], l[t, e] = True, ret, length
    ep(0, 0, 1800.0, 90)        # tile 0: a win
    ep(2, 15, -2300.0, 120)     # tile 0: a loss
    ep(1, 16, -1900.0, 501)     # tile 1: the time limit, a draw
    ep(1, 17, 1500.0, 200)      # tile 1: a win
    ep(2, 17, 1990.0, 3)        # tile 1: the same env again
    ep(0, 47, -2050.0, 40)      # tile 2: a loss
    r[1, 5] = 1e6               # not an episode end: ignored
    sc = policy_zoo.league_scores(d, r, l, tile_member=[1, 0, 1], nmembers=3)
    assert sc.dtype == np.int64 and sc.shape == (3, 4)
    assert sc.tolist() == [[3, 2, 0, 1], [3, 1, 2, 0], [0, 0, 0, 0]]
    assert (sc[:, 0] == sc[:, 1:].sum(axis=1)).all()
    with pytest.raises(ValueError):
        policy_zoo.league_scores(d, r, l, tile_member=[0, 1], nmembers=2)


# ---- what install_fixed_opponent builds ---------------------------------------------------------------------------------------
class _Stub(object):
    initial_state = None

    def __init__(self, what):
        self.what, self.seeded = what, None

    def seed(self, s):
        self.seeded = s

    def step(self, *a, **k):
        return None

    def value(self, *a, **k):
        return None


class _FakeRunner(object):
    def __init__(self, nenv):
        self.nenv, self.models, self.env = nenv, [None, None], object()


def test_a_single_string_still_yields_a_plain_zoo_policy(monkeypatch):
    calls = []
    monkeypatch.setattr(policy_zoo, "load_zoo_policy", lambda path, ac_dim, device=0, kind=None: calls.append(("single", path)) or _Stub(path))
    monkeypatch.setattr(policy_zoo, "load_zoo_league", lambda paths, ac_dim, nenvs, device=0: calls.append(("league", list(paths), nenvs)) or _Stub(paths))
    r = _FakeRunner(64)
    alg_ppo.install_fixed_opponent(r, "a.npy", 8, "dev", 1017)
    assert calls == [("single", "a.npy")]
    m = r.models[1]
    assert isinstance(m, policy_zoo.FixedOpponentModel) and m.act_model.what == "a.npy" and m.act_model.seeded == 1017
    assert alg_ppo.assign_league(r, 2) is None                       # no league: nothing is re-dealt, nothing is tallied
    for paths in (["a.npy", "b.npy"], ("a.npy",)):
        calls.clear()
        alg_ppo.install_fixed_opponent(r, paths, 8, "dev", 1017)
        assert calls == [("league", list(paths), 64)] and r.models[1].act_model.seeded == 1017
    with pytest.raises(ValueError, match="fix_opponent_path"):
        alg_ppo.install_fixed_opponent(r, None, 8, "dev", 1)


def test_opponent_pool_stays_refused_in_fix_mode():
    with pytest.raises(ValueError, match="fixed opponent"):
        alg_ppo.check_opponent_pool("fix", None, fused=True)


def test_run_py_collects_a_repeated_fix_opponent_path():
    sys.path.insert(0, ROOT)
    import run
    assert run.parse_unknown(["--fix_opponent_path=a.npy"]) == {"fix_opponent_path": "a.npy"}
    got = run.parse_unknown(["--fix_opponent_path=a.npy", "--opponent_mode=fix", "--fix_opponent_path=b.npy", "--fix_opponent_path=c.npy"])
    assert got == {"fix_opponent_path": ["a.npy", "b.npy", "c.npy"], "opponent_mode": "fix"}
    assert run.parse_unknown(["--nsteps=8", "--nsteps=16"]) == {"nsteps": 16}     # other keys keep the last value


# ---- header and ctypes --------------------------------------------------------------------------------------------------------
def test_zoo_league_struct_matches_the_header(tmp_path):
    fields = [("mlp", None), ("lstm", None), ("tile_entry_dev", None), ("mlp.params", capi.ZooMlp.params), ("mlp.ob_dim", capi.ZooMlp.ob_dim),
              ("lstm.params", capi.ZooLstm.params), ("lstm.state", capi.ZooLstm.state), ("lstm.hidden", capi.ZooLstm.hidden)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sumo_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(sumo_zoo_league));']
    for name, _ in fields:
        lines.append('  printf("%s %%zu\\n", offsetof(sumo_zoo_league, %s));' % (name, name))
    lines += ['  return 0;', '}']
    src = tmp_path / "league.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "league"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    table = dict((a, int(b)) for a, b in (ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()))
    Z = capi.ZooLeague
    assert C.sizeof(Z) == table["size"]
    assert [n for n, _ in Z._fields_] == ["mlp", "lstm", "tile_entry_dev"]
    for name, inner in fields:
        head = name.split(".")[0]
        off = getattr(Z, head).offset + (inner.offset if inner is not None else 0)
        assert off == table[name], name
    assert Z.tile_entry_dev.offset + Z.tile_entry_dev.size == table["size"]       # ends in a pointer: no field of the header is missed


def test_library_exports_the_league_launches():
    from robosumo_selfplay_amd import build
    build.build_all()
    L = C.CDLL(build.lib_path("libsumo_hip.so"))
    for n in ("sumo_rollout_steps_zoo_league", "sumo_rollout_steps_lstm_zoo_league"):
        assert hasattr(L, n) and n in capi.EXPORTS
