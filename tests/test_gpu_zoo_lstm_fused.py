"""The fused match launches against policy-zoo LSTM nets (include/sumo_hip.h sumo_match_steps_zoo_lstm /
sumo_match_steps_lstm_zoo_lstm) on the GPU: against the step-by-step launches they replace (ppo_forward or ppo_lstm_step for agent
0, ppo_lstm_step on the zoo net's policy branch for agent 1, then step_device) bit for bit, against the numpy restatement of the
zoo net on the observations the engine produced, their loud failures, and the drivers built on them.

Tolerance of the numpy comparison: 5e-5 absolute on agent 1's action mean and state, what test_zoo_lstm_rollout_matches_oracle
(tests/test_gpu_zoo.py) uses for the same net on the step kernel."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, has_gpu
from zoo_lstm_helpers import golden, synthetic_lstm_flat

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch
    from robosumo_selfplay_amd import capi, matches, policies, policy_zoo
    from robosumo_selfplay_amd.lstm_model import LstmSpec
    from robosumo_selfplay_amd.model import PPOModel
    from robosumo_selfplay_amd.vec_env import SumoVecEnv
    from oracle import ppo_oracle as po


def _dims(env):
    return env.observation_space[0].shape[0], env.action_space[0].shape[0]


def _mlp_table(env, k, seed=0, scale=0.3):
    D, A = _dims(env)
    spec = policies.PolicySpec(D, A, value_network="copy", activation="relu")
    rng = np.random.default_rng(seed)
    t = matches.SnapshotTable(spec, k, env.device)
    for j in range(k):
        t.set(j, policies.flatten_params([p + scale * rng.standard_normal(p.shape).astype(np.float32) for p in policies.init_param_list(D, A)]))
    return t


def _lstm_table(env, k, seed=0, scale=0.1):
    D, A = _dims(env)
    rng = np.random.default_rng(seed)
    t = matches.LstmSnapshotTable(LstmSpec(D, A, 128), k, env.device)
    for j in range(k):
        pl = policies.init_lstm_param_list(D, A, 128, rng=np.random.RandomState(int(rng.integers(1 << 30))))
        t.set(j, [p + scale * rng.standard_normal(p.shape).astype(np.float32) for p in pl])
    return t


def _zoo_lstm_table(env, k, seed=20):
    D, A = _dims(env)
    return policy_zoo.ZooLstmTable([synthetic_lstm_flat(D - 1, A, seed + j) for j in range(k)], A, env.device)


def _new_states(N, recurrent):
    z = lambda w: torch.zeros((N, w), dtype=torch.float32, device="cuda")
    return (z(256), z(128)) if recurrent else z(128)


def _state(env):
    torch.cuda.synchronize()
    host = [x.cpu().numpy().copy() for x in (env.obs_dev, env.info_dev, env.done_dev, env.act_dev)]
    for E in env.engines:
        host += list(E.get_state())
    return host


def _near_time_limit(envs):
    """Every episode starts near the time limit, so episodes end (and auto-reset, and the recurrent states reset) inside the launches."""
    for g in range(envs[0].groups):
        qpos, qvel, warm, cnt = envs[0].engines[g].get_state()
        cnt[:, 0] = envs[0].model.timestep_limit - 40 + (np.arange(len(cnt)) % 37)
        for e in envs:
            e.engines[g].set_state(qpos, qvel, warm, cnt)


# ---- 5. / 6. fused == step by step ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id,N,groups", [("RoboSumo-Ant-vs-Ant-v0", 64, 1), ("RoboSumo-Ant-vs-Ant-v0", 64, 2),
                                             ("RoboSumo-Spider-vs-Spider-v0", 32, 1)])
@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("recurrent", [False, True])
def test_zoo_lstm_match_launch_equals_stepwise_path(env_id, N, groups, deterministic, recurrent):
    """Mode 6 (MLP checkpoints, recurrent False) and mode 7 (LSTM(128) checkpoints): score counters, observations, the env action
    buffer, done flags, the physics state and every recurrent state tensor are bit-identical after every chunk."""
    ef, es = [SumoVecEnv(env_id, num_envs=N, seed=11, adjust_z=-0.5, groups=groups) for _ in range(2)]
    table = (_lstm_table if recurrent else _mlp_table)(ef, 3)
    zoo = _zoo_lstm_table(ef, 2)
    assert torch.isclose(zoo.filt[:, 1], torch.tensor(10.0, device="cuda")).any()   # variances under the 1e-2 floor: 1 / std = 10
    rng = np.random.default_rng(5)
    idx0, idx1 = rng.integers(0, 3, N).astype(np.int32), rng.integers(0, 2, N).astype(np.int32)
    assert len(set(idx0)) == 3 and len(set(idx1)) == 2
    for e in (ef, es):
        e.reset_device()
    _near_time_limit([ef, es])
    i0, i1 = torch.from_numpy(idx0).cuda(), torch.from_numpy(idx1).cuda()
    sf = torch.zeros((N, 3), dtype=torch.int32, device="cuda")
    ss = torch.zeros_like(sf)
    stf, sts = _new_states(N, recurrent), _new_states(N, recurrent)
    quota, K, A = 3, 48, table.spec.ac_dim
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    for chunk in range(2):
        noise = None if deterministic else tuple(torch.randn((K, N, A), generator=gen, device="cuda") for _ in range(2))
        matches.zoo_lstm_match_steps_fused(ef, table, zoo, i0, i1, stf, sf, quota, K, noise)
        matches.zoo_lstm_match_steps_stepwise(es, table, zoo, idx0, idx1, sts, ss, quota, K, noise)
        torch.cuda.synchronize()
        assert torch.equal(sf, ss), chunk
        for name in ("obs_dev", "act_dev", "done_dev"):
            assert torch.equal(getattr(ef, name), getattr(es, name)), (name, chunk)
        for k, (x, y) in enumerate(zip(stf, sts) if recurrent else [(stf, sts)]):
            assert torch.equal(x, y), ("state", k, chunk)
            assert float(x.abs().max()) > 0.0
        for k, (x, y) in enumerate(zip(_state(ef), _state(es))):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (k, chunk)
    assert int(sf.sum(1).min()) >= 1, "an env saw no episode end (no state reset) inside the launches"
    assert int(sf.sum(1).max()) <= quota
    assert ef.stats()["rollout_aborts"] == 0
    ef.close(); es.close()


# ---- 7. against numpy -------------------------------------------------------------------------------------------------------
def test_zoo_lstm_match_matches_numpy_net():
    N, steps = 16, 16
    env = SumoVecEnv("RoboSumo-Ant-vs-Ant-v0", num_envs=N, seed=5, adjust_z=-0.5)
    D, A = _dims(env)
    flat = golden("ant-lstm-v3")
    Dz, p = policy_zoo.split_zoo_lstm(flat, A)
    assert Dz == D - 1
    table, zoo = _mlp_table(env, 1), policy_zoo.ZooLstmTable([flat], A, env.device)
    env.reset_device()
    i = torch.zeros(N, dtype=torch.int32, device="cuda")
    sc = torch.zeros((N, 3), dtype=torch.int32, device="cuda")
    st1 = _new_states(N, False)
    ostate = np.zeros((4, N, 64), np.float32)
    worst_a = worst_s = 0.0
    for t in range(steps):
        torch.cuda.synchronize()
        obs1 = env.obs_dev[:, 1, :Dz].cpu().numpy()
        fin = env.done_dev[:, 0].cpu().numpy() != 0
        ostate[:, fin, :] = 0
        mean_o, _, ostate = po.zoo_lstm_step(p, obs1, ostate)
        matches.zoo_lstm_match_steps_fused(env, table, zoo, i, i, st1, sc, 1 << 30, 1)
        torch.cuda.synchronize()
        a1 = env.act_dev[:, 1, :A].cpu().numpy()
        s1 = st1.cpu().numpy()
        e_a = np.abs(a1 - mean_o).max()
        e_s = max(np.abs(s1[:, :64] - ostate[2]).max(), np.abs(s1[:, 64:] - ostate[3]).max())
        worst_a, worst_s = max(worst_a, e_a), max(worst_s, e_s)
        print("step %d: action err %.3g, state err %.3g" % (t, e_a, e_s))
        assert e_a < 5e-5 and e_s < 5e-5, t
        ostate = ostate.astype(np.float32)
    print("worst action err %.3g, worst state err %.3g" % (worst_a, worst_s))
    env.close()


# ---- 8. loud failures ---------------------------------------------------------------------------------------------------------
def test_zoo_lstm_launch_refusals():
    N = 16
    env = SumoVecEnv("RoboSumo-Ant-vs-Ant-v0", num_envs=N, seed=2, adjust_z=-0.5)
    D, A = _dims(env)
    table, ltable, zoo = _mlp_table(env, 2), _lstm_table(env, 2), _zoo_lstm_table(env, 2)
    env.reset_device()
    i = torch.zeros(N, dtype=torch.int32, device="cuda")
    sc = torch.zeros((N, 3), dtype=torch.int32, device="cuda")
    st1, (l0, l1) = _new_states(N, False), _new_states(N, True)
    # an index outside its table: the launch is cut short and rollout_status raises
    bad = i.clone(); bad[3] = 2
    for tab, st in ((table, st1), (ltable, (l0, l1))):
        with pytest.raises(capi.SumoHipError, match="cut short"):
            matches.zoo_lstm_match_steps_fused(env, tab, zoo, i, bad, st, sc, 1, 4)       # idx1 against nzoo
        env.reset_device()
        with pytest.raises(capi.SumoHipError, match="cut short"):
            matches.zoo_lstm_match_steps_fused(env, tab, zoo, bad, i, st, sc, 1, 4)       # idx0 against nsnap
        env.reset_device()
    E, bufs = env.engine, env.env_ptrs(0)

    def zs(**kw):
        z = zoo.struct(st1)
        for k, v in kw.items():
            setattr(z, k, v)
        return z

    mo = capi.Match(params=table.params.data_ptr(), idx0=i.data_ptr(), idx1=i.data_ptr(), nsnap=2, ob_dim=D, ac_dim=A, T=4, s0=0, K=4,
                    quota=1, score=sc.data_ptr())
    import ctypes as C
    ml = capi.MatchLstm(proto=C.addressof(ltable.proto), nets_dev=ltable.nets_dev.data_ptr(), idx0=i.data_ptr(), idx1=i.data_ptr(), nsnap=2,
                        state0=l0.data_ptr(), T=4, s0=0, K=4, quota=1, score=sc.data_ptr())
    for call, launch in ((E.match_steps_zoo_lstm, mo), (E.match_steps_lstm_zoo_lstm, ml)):
        for field, kw in (("ob_dim", dict(ob_dim=D + 1)), ("ob_dim", dict(ob_dim=0)), ("nzoo", dict(nzoo=0)), ("obs_clip", dict(obs_clip=0.0)),
                          ("params", dict(params=None)), ("filt", dict(filt=None)), ("state", dict(state=None)),
                          ("hidden", dict(hidden=128)), ("emb_dim", dict(emb_dim=32))):
            with pytest.raises(capi.SumoHipError, match=field):
                call(launch, zs(**kw), *bufs)
        E.set_cfrc_mode("rne_post")
        with pytest.raises(capi.SumoHipError, match="rne_post"):
            call(launch, zs(), *bufs)
        E.set_cfrc_mode("zero")
    ml.state1 = l1.data_ptr()
    with pytest.raises(capi.SumoHipError, match="state1"):
        E.match_steps_lstm_zoo_lstm(ml, zs(), *bufs)
    ml.state1 = None
    ml.state0 = None
    with pytest.raises(capi.SumoHipError, match="state0"):
        E.match_steps_lstm_zoo_lstm(ml, zs(), *bufs)
    ml.state0 = l0.data_ptr()
    # the Python drivers: table kinds, state shapes, the MLP zoo table's refusals stay
    with pytest.raises(ValueError, match="LSTM"):
        policy_zoo.ZooTable([synthetic_lstm_flat(D - 1, A, 1)], A, env.device)
    with pytest.raises(ValueError, match="MLP"):
        policy_zoo.ZooLstmTable([golden("ant-mlp-v3")], A, env.device)
    mzoo = policy_zoo.ZooTable([golden("ant-mlp-v3")], A, env.device)
    with pytest.raises(ValueError, match="zoo MLP nets"):
        matches.zoo_match_steps_fused(env, ltable, mzoo, i, i, sc, 1, 4)                  # LSTM checkpoints against zoo MLP nets
    with pytest.raises(ValueError, match="zoo MLP nets"):
        matches.play_against_zoo(env, ltable, mzoo, [(0, 0)], 1, 1)
    with pytest.raises(ValueError, match="ZooLstmTable"):
        matches.zoo_lstm_match_steps_fused(env, table, mzoo, i, i, st1, sc, 1, 4)
    with pytest.raises(ValueError, match="state"):
        matches.zoo_lstm_match_steps_fused(env, table, zoo, i, i, l0, sc, 1, 4)           # [N][256] is not a zoo state
    wide = policy_zoo.ZooLstmTable([synthetic_lstm_flat(D + 5, A, 1)], A, env.device)
    with pytest.raises(ValueError, match="ob_dim"):
        matches.zoo_lstm_match_steps_fused(env, table, wide, i, i, st1, sc, 1, 4)
    env.cfrc_mode = "rne_post"
    with pytest.raises(ValueError, match="rne_post"):
        matches.zoo_lstm_match_steps_fused(env, table, zoo, i, i, st1, sc, 1, 4)
    env.cfrc_mode = "zero"
    env.close()
    # mixed match-ups stay refused
    mixed = SumoVecEnv("RoboSumo-Ant-vs-Bug-v0", num_envs=4, seed=2)
    with pytest.raises(ValueError, match="homogeneous"):
        matches.zoo_lstm_match_steps_fused(mixed, table, zoo, i[:4], i[:4], st1[:4], sc[:4], 1, 4)
    with pytest.raises(capi.SumoHipError, match="homogeneous"):
        mixed.engine.match_steps_zoo_lstm(mo, zs(), *mixed.env_ptrs(0))
    mixed.close()


# ---- 9. drivers ---------------------------------------------------------------------------------------------------------------
def _learner(D, A, seed):
    np.random.seed(seed)
    spec = policies.PolicySpec(D, A, value_network="copy", activation="relu")
    m = PPOModel(policy=spec, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, trainable=False)
    rng = np.random.RandomState(seed)
    m.set_param_list([p + rng.normal(0, 0.1, p.shape).astype(np.float32) for p in m.get_param_list()])
    return m


def test_evaluate_history_against_mixed_zoo_files_and_cli(tmp_path):
    run = str(tmp_path / "run")
    os.makedirs(os.path.join(run, "checkpoints"))
    for k in range(1, 3):
        _learner(121, 8, 10 + k).save(os.path.join(run, "checkpoints", "%.5i" % k))
    opp = [str(tmp_path / "lstm-v3.npy"), str(tmp_path / "mlp-v3.npy")]
    np.save(opp[0], golden("ant-lstm-v3"))
    np.save(opp[1], golden("ant-mlp-v3"))
    res = [matches.evaluate_history_against_zoo(run, opp, trials=32, num_env=64, fused=f) for f in (True, False)]
    assert res[0] == res[1]
    r = res[0]
    assert r["checkpoints"] == [1, 2] and r["opponents"] == opp and list(r["results"]) == [(1, 0), (1, 1), (2, 0), (2, 1)]
    for key, x in r["results"].items():
        assert x["rounds"] == 32 and abs(x["win"] + x["draw"] + x["lose"] - 1.0) < 1e-12, key
    sys.path.insert(0, ROOT)
    import eval_against_fix
    tab = eval_against_fix.main(["--path", run, "--opponent_path", opp[0], "--opponent_path", opp[1], "--fused", "--trials", "32",
                                 "--num_env", "64"])
    with open(os.path.join(run, "eval_against_fix.json")) as f:
        js = json.load(f)
    assert [row[0] for row in js] == [1, 2] and np.allclose(tab, np.array(js))
    for row in js:
        assert len(row) == 7
        for k in range(2):                                                 # the CLI's table is the driver's, in --opponent_path order
            x = r["results"][(row[0], k)]
            assert row[1 + 3 * k:4 + 3 * k] == [x["win"], x["draw"], x["lose"]]
