"""``mixed.MixedRunner`` on mixed match-ups: 32 envs, T = 6, a seat of one zoo MLP and one zoo LSTM net, episodes that end inside the
window.  The one-launch step against the definition, two env groups against one, consecutive rollouts, agent 0's returns against the
numpy V-trace oracle, the league tally.  Every comparison is ``torch.equal`` over whole tensors unless stated otherwise."""
import os

import numpy as np
import pytest

from conftest import has_gpu

pytestmark = pytest.mark.gpu
if has_gpu():
    import torch
    from oracle import ppo_oracle as po
    from robosumo_selfplay_amd import mixed, policies, zoo_pairs
    from robosumo_selfplay_amd.model import PPOModel
    from robosumo_selfplay_amd.vec_env import SumoVecEnv

HERE = os.path.dirname(os.path.abspath(__file__))
N, T = 32, 6
ENVS = ["RoboSumo-Ant-vs-Bug-v0", "RoboSumo-Spider-vs-Ant-v0"]
_CACHE = {}


def _nets():
    if "nets" not in _CACHE:
        with np.load(os.path.join(HERE, "golden", "zoo_v3_params.npz"), allow_pickle=False) as z:
            _CACHE["nets"] = {k: z[k].copy() for k in z.files}
    return _CACHE["nets"]


def _near_time_limit(env):
    """Episodes end (auto-reset) at different steps inside the six-step window: env e runs out of time in its step 7 - e % 7."""
    for g, E in enumerate(env.engines):
        qpos, qvel, warm, cnt = E.get_state()
        cnt[:, 0] = env.model.timestep_limit - 6 + ((g * env.group_size + np.arange(len(cnt))) % 7)
        E.set_state(qpos, qvel, warm, cnt)


def _runner(env_id, fused, groups=1):
    env = SumoVecEnv(env_id, num_envs=N, seed=3, groups=groups)
    species = env_id.split("-")[3].lower()                    # agent 1's
    spec = policies.PolicySpec(env.model.obs_dims[0], env.model.act_dims[0], value_network="copy", activation="relu")
    np.random.seed(5)
    model = PPOModel(policy=spec, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, trainable=False)
    model.act_model.seed(101)
    seat = zoo_pairs.seat_for(env, 1, [_nets()[species + "-mlp-v3"], _nets()[species + "-lstm-v3"]])
    r = mixed.MixedRunner(env, model, seat, T, 0.995, 0.95, 500, fused=fused, seat_seed=202)
    _near_time_limit(env)
    return r


def _tensors(out):
    """The device tensors of a rollout tuple, flattened (pairs included), with their positions."""
    flat = []
    for k, x in enumerate(out):
        for j, y in enumerate(x if isinstance(x, tuple) else (x,)):
            if torch.is_tensor(y):
                flat.append(((k, j), y))
    return flat


def _assert_same_rollout(a, b, ra, rb):
    ta, tb = _tensors(a), _tensors(b)
    assert [k for k, _ in ta] == [k for k, _ in tb] and len(ta) >= 11
    for (k, x), (_, y) in zip(ta, tb):
        assert x.shape == y.shape and torch.equal(x, y), k
    assert a[11] == b[11]                                        # the episode records
    for k in ra.last_buffers:
        assert torch.equal(ra.last_buffers[k], rb.last_buffers[k]), k
    assert torch.equal(ra.state, rb.state) and torch.equal(ra.env.obs_dev, rb.env.obs_dev) and torch.equal(ra.env.done_dev, rb.env.done_dev)
    assert np.array_equal(ra.league_scores, rb.league_scores)


@pytest.mark.parametrize("env_id", ENVS)
def test_fused_step_equals_the_definition_and_rollouts_continue(env_id):
    rf, rd = _runner(env_id, True), _runner(env_id, False)
    assert rf.fused and not rd.fused
    of, od = rf.run(1), rd.run(1)
    torch.cuda.synchronize()
    _assert_same_rollout(of, od, rf, rd)
    D0, A0 = rf.env.model.obs_dims[0], rf.env.model.act_dims[0]
    assert of[0][0].shape == (N * T, D0) and of[3][0].shape == (N * T, A0) and of[0][1] is None and of[3][1] is None
    assert of[1].shape == (2, N * T) and torch.isfinite(of[1][0]).all() and torch.isfinite(of[4][0]).all() and torch.isfinite(of[5][0]).all()
    assert bool(torch.isinf(of[5][1]).all())                     # agent 1's neglogp placeholder: no opponent sample is usable
    assert all(bool((of[k] == 1.0).all()) for k in (12, 13, 14))    # the three ratios
    assert float(rf.state.abs().max()) > 0                       # the LSTM tile's state moved
    assert int(rf.last_buffers["ep_done"].sum()) > 0             # episodes did end inside the window
    # the league: one row per member, every finished episode counted once
    sc = rf.league_scores
    assert sc.shape == (2, 4) and int(sc[:, 0].sum()) == int(rf.last_buffers["ep_done"].sum()) == len(of[11])
    assert np.array_equal(sc[:, 1:].sum(1), sc[:, 0]) and rf.tile_member.tolist() == [0, 1]
    # the second rollout continues: its first observations are the env's final ones of the first, the state rows persist
    final_obs, state1 = rf.env.obs_dev[:, 0, :D0].clone(), rf.state.clone()
    assert rf.assign(2) is rf and rf.tile_member.tolist() == [1, 0] and float(rf.state.abs().max()) == 0.0     # every tile changed its net
    rf.assign(1)
    rf.state.copy_(state1); rd.assign(1)
    of2, od2 = rf.run(2), rd.run(2)
    torch.cuda.synchronize()
    _assert_same_rollout(of2, od2, rf, rd)
    assert torch.equal(rf.last_buffers["obs"][0], final_obs)
    assert not torch.equal(of2[3][0], of[3][0])
    rf.env.close(); rd.env.close()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "definition"])
def test_two_groups_equal_one(fused):
    r1, r2 = _runner(ENVS[0], fused, groups=1), _runner(ENVS[0], fused, groups=2)
    o1, o2 = r1.run(3), r2.run(3)
    torch.cuda.synchronize()
    _assert_same_rollout(o1, o2, r1, r2)
    r1.env.close(); r2.env.close()


@pytest.mark.parametrize("env_id", ENVS)
def test_returns_against_the_oracle(env_id):
    r = _runner(env_id, True)
    out = r.run(250)
    torch.cuda.synchronize()
    B = r.last_buffers
    last_v = r.model.act_model.evaluate(r.env.obs_dev[:, 0, :], 2)["value"].cpu().numpy()
    ones = np.ones((T, N), np.float32)
    e0 = po.vtrace_returns(B["rew"][0].cpu().numpy(), B["val"].cpu().numpy(), B["done"].cpu().numpy().astype(bool),
                           r.env.done_dev[:, 0].cpu().numpy().astype(bool), last_v, ones, ones * np.float32(0.95), 0.995)
    got = out[1][0].reshape(N, T).cpu().numpy().T
    assert np.array_equal(got, e0)                               # the bound test_vtrace_kernel_vs_oracle_large holds agent 0 to
    r.env.close()


def test_runner_refusals():
    env = SumoVecEnv(ENVS[0], num_envs=N, seed=3)
    spec = policies.PolicySpec(env.model.obs_dims[1], env.model.act_dims[1], value_network="copy", activation="relu")
    bug_model = PPOModel(policy=spec, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, trainable=False)
    seat = zoo_pairs.seat_for(env, 1, [_nets()["bug-mlp-v3"]])
    with pytest.raises(ValueError, match="does not fit agent 0"):
        mixed.MixedRunner(env, bug_model, seat, T, 0.995, 0.95)
    env.close()
    env = SumoVecEnv(ENVS[0], num_envs=48, seed=3, groups=2)    # groups of 24 envs: off the tile grid
    with pytest.raises(ValueError, match="multiples of 16"):
        mixed.check_groups(env)
    env.close()
