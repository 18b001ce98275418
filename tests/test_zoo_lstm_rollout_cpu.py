"""CPU-side checks of the fused rollout launch against policy-zoo LSTM nets (sumo_rollout_steps_zoo_lstm): the library's export and
its binding, and the model surface ``ZooLSTMPolicy`` offers to ``FixedOpponentModel`` and the ``Runner`` (by inspection: building
the policy needs a GPU, so the ``FixedOpponentModel`` around a real policy is exercised in tests/test_gpu_zoo_lstm_rollout.py)."""
import ctypes as C
import inspect

from robosumo_selfplay_amd import build, capi, policy_zoo, runner, vec_env


def test_library_exports_the_zoo_lstm_rollout_entry_point():
    build.build_all()
    L = C.CDLL(build.lib_path("libsumo_hip.so"))
    n = "sumo_rollout_steps_zoo_lstm"
    assert n in capi.EXPORTS and hasattr(L, n)
    assert callable(getattr(capi.Engine, "rollout_steps_zoo_lstm"))
    assert callable(getattr(vec_env.SumoVecEnv, "rollout_steps_zoo_lstm_group"))


def test_zoo_lstm_policy_has_the_model_surface():
    P = policy_zoo.ZooLSTMPolicy
    for name in ("step", "value", "action_probability", "evaluate", "act", "reset", "seed"):
        assert callable(getattr(P, name, None)), name
    # what FixedOpponentModel.__init__ reads, and the feeds both Runner modes pass
    src = inspect.getsource(policy_zoo.FixedOpponentModel.__init__)
    assert "policy.step" in src and "policy.value" in src
    for name, feeds in (("step", ("observation", "S", "M", "noise")), ("value", ("ob", "S", "M")),
                        ("action_probability", ("observation", "given_action")),
                        ("evaluate", ("obs", "state", "mask", "given_action", "noise", "out"))):
        params = inspect.signature(getattr(P, name)).parameters
        for f in feeds:
            assert f in params, (name, f)
    assert P.recurrent and P.initial_state is None
    # the Runner's side: the pair (MLP learner, zoo LSTM net) resolves to this launch, and the one driver / evaluator play it
    la = runner.rollout_launch("mlp", "zoo", "lstm")
    assert (la.entry, la.struct, la.selector) == ("rollout_steps_zoo_lstm_group", "Rollout", "opponent_index")
    for name in ("rollout_mode", "fused_steps", "_launch_steps", "_evaluate_step", "zoo_opponent", "fused_zoo_ok"):
        assert callable(getattr(runner.Runner, name, None)), name
