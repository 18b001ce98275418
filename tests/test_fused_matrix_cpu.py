"""The census of tests/fused_matrix.py, without a device: every policy phase the library compiles has a row on every scene variant
where the Python API can launch it, every launch the pure resolvers name (``runner.rollout_launch``, ``matches.match_pairing``,
``co_train``'s pair launch) is a row, the policy numbers are the ones the engine's entry points pass to ``rollout_launch``, and the
variants' nv are the scenes'."""
import os
import re

import pytest

import fused_matrix as FM
from conftest import ROOT
from robosumo_selfplay_amd import capi, co_train, matches, mjcf, runner, vec_env
from test_match_pairing_cpu import ROWS as PAIRING_ROWS
from test_rollout_mode_cpu import TABLE as ROLLOUT_TABLE

CSRC = os.path.join(ROOT, "robosumo_selfplay_amd", "csrc")
ENTRIES = list(capi.FUSED_ENTRIES) + list(capi.PAIR_ENTRIES)       # in the order of the policy numbers (checked against the source below)
N_POLICY = len(ENTRIES)
CASES = FM.cases()
SAME = [v for v in FM.VARIANTS if not FM.is_mixed(v)]
MIXED = [v for v in FM.VARIANTS if FM.is_mixed(v)]


def _rows(variant):
    return {c.policy: c for c in CASES if c.variant is variant}


def test_the_variants_are_the_issue_s_eleven():
    assert [v.key for v in FM.VARIANTS] == ["ant-static", "ant-dynamic", "bug", "spider-static", "spider-dynamic", "ant-bug", "bug-ant",
                                            "ant-spider", "spider-ant", "bug-spider", "spider-bug"]
    assert len(SAME) == 5 and len(MIXED) == 6
    for v in FM.VARIANTS:
        m = mjcf.load_model(v.env_id)
        assert m.nv == v.nv, v.key
        assert (m.obs_dims[0] != m.obs_dims[1]) == FM.is_mixed(v)
        # static layouts exist for Ant-vs-Ant and Spider-vs-Spider; the variable switches them off and is set for nothing else
        assert v.static == (v.key in ("ant-static", "spider-static")) and (v.layout_env == "0") == v.key.endswith("-dynamic")


def test_every_policy_has_a_row_on_every_variant_where_it_is_reachable():
    """``N_POLICY`` is read from the bindings' entry tables: a new entry (policy 17) fails here until the matrix has rows for it."""
    assert sorted(FM.POLICIES) == list(range(N_POLICY))
    pair = set(range(len(capi.FUSED_ENTRIES), N_POLICY))
    assert pair == {FM.PAIR_POLICY}
    for v in SAME:
        assert sorted(_rows(v)) == list(range(N_POLICY)), v.key
    for v in MIXED:                                                   # every other entry refuses a mixed scene (rollout_scene)
        assert set(_rows(v)) == pair, v.key
    assert len(CASES) == len(SAME) * N_POLICY + len(MIXED) * len(pair)


def test_rows_name_the_entry_of_their_policy():
    for c in CASES:
        assert c.entry == ENTRIES[c.policy] == FM.POLICIES[c.policy][0], c.id
        assert c.entry in capi.EXPORTS or c.entry in capi.PAIR_ENTRIES
        assert c.num_envs % 8 == 0 and c.builder.split(":")[0] in ("rollout", "match", "pair")


def test_policy_numbers_are_the_engine_s():
    """Each ``extern "C" int sumo_*`` entry point of csrc/engine_host_fused.h ends in ``rollout_launch(E, r, POLICY, b, stream)``; the
    number of phases is ``SUMO_N_POLICY`` of csrc/sumo_engine.hip."""
    txt = open(os.path.join(CSRC, "engine_host_fused.h")).read()
    found = {}
    for m in re.finditer(r'extern "C" int (sumo_\w+)\(', txt):
        body = txt[m.end():]
        nxt = body.find('extern "C"')
        k = re.search(r"return rollout_launch\(E, r, (\d+), b, stream\);", body if nxt < 0 else body[:nxt])
        assert k, m.group(1)
        found[m.group(1)] = int(k.group(1))
    assert found == {name: k for k, name in enumerate(ENTRIES)}
    n = re.search(r"^#define SUMO_N_POLICY (\d+)", open(os.path.join(CSRC, "sumo_engine.hip")).read(), re.M)
    assert int(n.group(1)) == N_POLICY


def test_every_rollout_launch_of_the_runner_is_a_row():
    seen = set()
    for case, _ in ROLLOUT_TABLE:
        la = runner.rollout_launch(*case)
        name = "sumo_" + la.entry[:-len("_group")]
        seen.add(name)
        for v in SAME:
            assert name in {c.entry for c in _rows(v).values()}, (case, v.key)
    assert len(seen) == 9


def test_every_match_pairing_is_a_row():
    seen = set()
    for t0, t1, *_ in PAIRING_ROWS:
        name = "sumo_" + matches.match_pairing(t0, t1).entry
        seen.add(name)
        for v in SAME:
            assert name in {c.entry for c in _rows(v).values()}, (name, v.key)
    assert len(seen) == 7 and seen == {"sumo_" + e for e in matches._ENTRY.values()}


def test_the_rollout_and_match_launches_are_all_the_homogeneous_entries():
    named = {"sumo_" + runner.rollout_launch(*case).entry[:-len("_group")] for case, _ in ROLLOUT_TABLE}
    named |= {"sumo_" + e for e in matches._ENTRY.values()}
    assert named == set(capi.FUSED_ENTRIES)


def test_co_train_s_pair_launch_is_a_row():
    (name,) = capi.PAIR_ENTRIES
    method = name[len("sumo_"):] + "_group"
    assert callable(getattr(vec_env.SumoVecEnv, method)) and method in co_train.PairRunner._launch_group.__code__.co_names
    for v in FM.VARIANTS:
        assert _rows(v)[FM.PAIR_POLICY].entry == name, v.key


def test_no_case_id_appears_twice():
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids)
    assert len({(c.variant.key, c.policy) for c in CASES}) == len(CASES)


def test_the_census_of_the_docstring():
    """87 reachable instantiations out of 7 x N_POLICY; the unreachable ones are policies 0 .. 15 at nv 32 and 40."""
    kernels = {FM.kernel_of(c) for c in CASES}
    compiled = {(nv, p, 0) for nv in (28, 32, 36, 40, 44) for p in range(N_POLICY)} | {(nv, p, sl) for nv, sl in ((28, 1), (44, 2)) for p in range(N_POLICY)}
    assert kernels <= compiled and len(compiled) == 7 * N_POLICY
    assert compiled - kernels == {(nv, p, 0) for nv in (32, 40) for p in range(len(capi.FUSED_ENTRIES))}
    assert "87 instantiations" in FM.__doc__ and "32 instantiations" in FM.__doc__ and len(kernels) == 87


@pytest.mark.parametrize("policy", sorted(FM.POLICIES))
def test_tile_modes_get_whole_tiles(policy):
    """The modes that select a table row per 16-env tile run on whole tiles, the others on two tiles and a partial one."""
    _, builder, n = FM.POLICIES[policy]
    per_tile = builder in ("rollout:lstm:pool", "rollout:lstm:zoo_mlp", "rollout:lstm:zoo_lstm", "rollout:mlp:league", "rollout:lstm:league")
    assert n == (64 if builder == "pair" else 48 if per_tile else 40)
