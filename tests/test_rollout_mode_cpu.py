"""The pure part of the Runner's mode resolution (runner.rollout_launch): every (learner, opponent) pair maps to the fused launch the
engine spells for it -- ``sumo_rollout_steps[_lstm][_zoo|_zoo_lstm|_zoo_league|_reuse]`` -- with its launch struct and the struct
field that selects agent 1's net; the pairs without a launch are refused.  No GPU, no env, no models."""
import pytest

from robosumo_selfplay_amd import capi, runner, vec_env

# (learner, opponent, zoo family or league composition (nmlp, nlstm), reuse) -> (SumoVecEnv method, capi struct, selector field)
TABLE = [
    (("mlp", "self", None, False), ("rollout_steps_group", "Rollout", "opponent_index")),
    (("mlp", "zoo", "mlp", False), ("rollout_steps_zoo_group", "Rollout", "opponent_index")),
    (("mlp", "zoo", "lstm", False), ("rollout_steps_zoo_lstm_group", "Rollout", "opponent_index")),
    (("mlp", "league", (3, 0), False), ("rollout_steps_zoo_group", "Rollout", "opponent_index")),
    (("mlp", "league", (0, 3), False), ("rollout_steps_zoo_lstm_group", "Rollout", "opponent_index")),
    (("mlp", "league", (2, 2), False), ("rollout_steps_zoo_league_group", "Rollout", None)),
    (("lstm", "self", None, False), ("rollout_steps_lstm_group", "RolloutLstm", "tile_net_dev")),
    (("lstm", "self", None, True), ("rollout_steps_lstm_reuse_group", "RolloutLstmReuse", "tile_net_dev")),
    (("lstm", "zoo", "mlp", False), ("rollout_steps_lstm_zoo_group", "RolloutLstm", "tile_net_dev")),
    (("lstm", "zoo", "lstm", False), ("rollout_steps_lstm_zoo_lstm_group", "RolloutLstm", "tile_net_dev")),
    (("lstm", "league", (3, 0), False), ("rollout_steps_lstm_zoo_group", "RolloutLstm", "tile_net_dev")),
    (("lstm", "league", (0, 3), False), ("rollout_steps_lstm_zoo_lstm_group", "RolloutLstm", "tile_net_dev")),
    (("lstm", "league", (2, 2), False), ("rollout_steps_lstm_zoo_league_group", "RolloutLstm", None)),
]


@pytest.mark.parametrize("case,expected", TABLE, ids=lambda x: "-".join(map(str, x)) if len(x) == 4 else "")
def test_every_pair_resolves_to_its_launch(case, expected):
    la = runner.rollout_launch(*case)
    assert (la.entry, la.struct, la.selector) == expected
    # the entry exists on the env, its symbol in the library's export list, the struct in the bindings with the selector field
    assert callable(getattr(vec_env.SumoVecEnv, la.entry, None))
    assert la.entry.endswith("_group") and "sumo_" + la.entry[:-len("_group")] in capi.EXPORTS
    fields = [f[0] for f in getattr(capi, la.struct)._fields_]
    assert la.selector is None or la.selector in fields
    assert ("state2" in fields) == case[3]
    # a mixed league's own struct carries the per-tile entries instead
    assert (la.selector is None) == (la.family == "league") and (la.family != "league" or "tile_entry_dev" in [f[0] for f in capi.ZooLeague._fields_])


def test_the_table_covers_every_combination():
    opponents = [("self", None), ("zoo", "mlp"), ("zoo", "lstm"), ("league", (3, 0)), ("league", (0, 3)), ("league", (2, 2))]
    want = {(l, o, f, False) for l in ("mlp", "lstm") for o, f in opponents} | {("lstm", "self", None, True)}
    assert {c for c, _ in TABLE} == want and len(TABLE) == 13
    assert len({e[0] for _, e in TABLE}) == 9                         # the nine rollout entry points, each reached


@pytest.mark.parametrize("learner", ["mlp", "lstm"])
@pytest.mark.parametrize("opponent,family", [("zoo", "mlp"), ("zoo", "lstm"), ("league", (3, 0)), ("league", (0, 3)), ("league", (2, 2))])
def test_reuse_against_a_zoo_opponent_is_not_supported(learner, opponent, family):
    with pytest.raises(NotImplementedError, match="recurrent self-play only"):
        runner.rollout_launch(learner, opponent, family, True)


def test_reuse_with_an_mlp_learner_has_no_launch():
    assert runner.rollout_launch("mlp", "self", None, True) is None


def test_runner_resolves_its_mode_and_driver_from_it():
    for name in ("rollout_mode", "fused_steps", "fused_ok", "fused_lstm_ok", "fused_zoo_ok", "fused_lstm_zoo_ok", "fused_league_ok",
                 "zoo_opponent", "lstm_zoo_opponent", "league_opponent", "_steps_fused", "_steps_fused_lstm", "_step_device", "join_groups"):
        assert callable(getattr(runner.Runner, name, None)), name
    for f in ("learner", "opponent", "zoo", "reuse", "noise_rows", "fused", "entry"):
        assert f in runner.RolloutMode._fields, f
