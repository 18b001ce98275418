"""Recurrent (LSTM) checkpoint matches on the GPU: the fused launch (include/sumo_hip.h sumo_match_steps_lstm) against the step-by-step
path -- per step one ppo_lstm_step launch per side and run of envs sharing a snapshot (the kernel LstmPPOModel.step runs), masked by
that side's done flags of the previous step, then env.step_device and the score update.  Everything is compared bit for bit:
observations, info rows, done flags, actions, qpos / qvel / warm start / counters, both agents' recurrent states and the score
counters.  The step-by-step path is tied to LstmPPOModel.step; then the quota, play_matches' round bookkeeping, the refusals and
compare_versions.py end to end on LstmPPOModel checkpoints."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def _env(env_id, N, seed=11):
    from robosumo_selfplay_amd.vec_env import SumoVecEnv
    return SumoVecEnv(env_id, num_envs=N, seed=seed, adjust_z=-0.5)


def _plist(D, A, rng, H=128, scale=0.1):
    from robosumo_selfplay_amd import policies
    pl = policies.init_lstm_param_list(D, A, H, rng=np.random.RandomState(int(rng.integers(1 << 30))))
    return [p + scale * rng.standard_normal(p.shape).astype(np.float32) for p in pl]


def _table(env, k, seed=0, H=128):
    from robosumo_selfplay_amd import matches
    from robosumo_selfplay_amd.lstm_model import LstmSpec
    D, A = env.observation_space[0].shape[0], env.action_space[0].shape[0]
    rng = np.random.default_rng(seed)
    t = matches.LstmSnapshotTable(LstmSpec(D, A, H), k, env.device)
    for j in range(k):
        t.set(j, _plist(D, A, rng, H))
    return t


def _states(N, H=128):
    import torch
    return tuple(torch.zeros((N, 2 * H), dtype=torch.float32, device="cuda") for _ in range(2))


def _state(env, states):
    import torch
    torch.cuda.synchronize()
    host = [x.cpu().numpy().copy() for x in (env.obs_dev, env.info_dev, env.done_dev, env.act_dev) + tuple(states)]
    return host + list(env.engine.get_state())


NAMES = ("obs", "info", "done", "actions", "state0", "state1", "qpos", "qvel", "warm", "counters")
CASES = [("RoboSumo-Ant-vs-Ant-v0", 96, True, "random"), ("RoboSumo-Ant-vs-Ant-v0", 96, False, "random"),
         ("RoboSumo-Spider-vs-Spider-v0", 32, False, "random"), ("RoboSumo-Spider-vs-Spider-v0", 32, True, "random"),
         ("RoboSumo-Ant-vs-Ant-v0", 4096, False, "blocks")]


@pytest.mark.parametrize("env_id,N,deterministic,layout", CASES)
def test_lstm_match_launch_equals_stepwise_path(env_id, N, deterministic, layout):
    import torch
    from robosumo_selfplay_amd import matches
    ef, es = _env(env_id, N), _env(env_id, N)
    table = _table(ef, 3)
    rng = np.random.default_rng(5)
    if layout == "random":
        idx0 = rng.integers(0, 3, N).astype(np.int32)
        idx1 = rng.integers(0, 3, N).astype(np.int32)
        idx1[::4] = idx0[::4]                                     # some envs play a snapshot against itself
    else:                                                         # contiguous blocks (play_matches' layout), waves migrate
        blk = np.arange(N) // 256
        idx0, idx1 = (blk % 3).astype(np.int32), ((blk // 3 + blk) % 3).astype(np.int32)
    assert (idx0 == idx1).any() and (idx0 != idx1).any()
    for e in (ef, es):
        e.reset_device()
    # start every episode near the time limit so episodes end (and auto-reset, masking the states) inside the launches
    qpos, qvel, warm, cnt = ef.engine.get_state()
    cnt[:, 0] = ef.model.timestep_limit - 40 + (np.arange(N) % 37)
    for e in (ef, es):
        e.engine.set_state(qpos, qvel, warm, cnt)
    i0, i1 = torch.from_numpy(idx0).cuda(), torch.from_numpy(idx1).cuda()
    sf, ss = _states(N), _states(N)
    cf = torch.zeros((N, 3), dtype=torch.int32, device="cuda")
    cs = torch.zeros_like(cf)
    quota, K = 2, 24
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    A = table.spec.ac_dim
    for chunk in range(3):
        noise = None if deterministic else tuple(torch.randn((K, N, A), generator=gen, device="cuda") for _ in range(2))
        matches.match_steps_fused_lstm(ef, table, i0, i1, sf, cf, quota, K, noise)
        matches.match_steps_stepwise_lstm(es, table, idx0, idx1, ss, cs, quota, K, noise)
        a, b = _state(ef, sf), _state(es, ss)
        for name, x, y in zip(NAMES, a, b):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (name, chunk, np.argwhere(x != y)[:5])
        assert torch.equal(cf, cs), chunk
    sc = cf.cpu().numpy()
    assert sc.sum() > 0, "no episode ended inside the launches"
    assert sc.sum(1).max() <= quota
    assert float(sf[0].abs().sum()) > 0 and float(sf[1].abs().sum()) > 0
    assert ef.stats()["rollout_aborts"] == 0
    ef.close(); es.close()


@pytest.mark.parametrize("deterministic", [True, False])
def test_first_step_equals_lstm_model_step(deterministic):
    """One step of the step-by-step path (and of the fused launch) from random states and done flags: each side's action and new
    state equal LstmPPOModel.step(obs, S, M) of the model the side plays."""
    import torch
    from robosumo_selfplay_amd import matches
    from robosumo_selfplay_amd.lstm_model import LstmPPOModel, LstmSpec
    N = 48
    es, ef = _env("RoboSumo-Ant-vs-Ant-v0", N), _env("RoboSumo-Ant-vs-Ant-v0", N)
    D, A = es.observation_space[0].shape[0], es.action_space[0].shape[0]
    spec = LstmSpec(D, A, 128)
    rng = np.random.default_rng(9)
    models = []
    for _ in range(2):
        m = LstmPPOModel(policy=spec, trainable=False)
        m.set_param_list(_plist(D, A, rng))
        models.append(m)
    table = matches.LstmSnapshotTable(spec, 2, es.device)
    table.set(0, models[0]); table.set(1, models[1])
    for e in (es, ef):
        e.reset_device()
    done = torch.from_numpy(rng.integers(0, 2, (N, 2)).astype(np.uint8)).cuda()
    S = [torch.from_numpy(rng.standard_normal((N, 256)).astype(np.float32)).cuda() for _ in range(2)]
    noise = None if deterministic else tuple(torch.randn((1, N, A), device="cuda") for _ in range(2))
    for e in (es, ef):
        e.done_dev.copy_(done)
    obs = es.obs_dev[:, :, :D].clone()
    ss, sf = [s.clone() for s in S], [s.clone() for s in S]
    idx0, idx1 = np.zeros(N, np.int32), np.ones(N, np.int32)
    sc = torch.zeros((N, 3), dtype=torch.int32, device="cuda")
    matches.match_steps_stepwise_lstm(es, table, idx0, idx1, ss, sc, 1, 1, noise)
    matches.match_steps_fused_lstm(ef, table, torch.from_numpy(idx0).cuda(), torch.from_numpy(idx1).cuda(), sf, sc.clone(), 1, 1, noise)
    torch.cuda.synchronize()
    for g in range(2):
        act, _, st, _ = models[g].step(obs[:, g], S=S[g], M=done[:, g], deterministic=deterministic,
                                       noise=None if noise is None else noise[g][0])
        for name, x in (("stepwise", es), ("fused", ef)):
            assert torch.equal(x.act_dev[:, g, :A], act), (name, g)
        assert torch.equal(ss[g], st) and torch.equal(sf[g], st), g
    es.close(); ef.close()


def test_quota_and_round_bookkeeping():
    import torch
    from robosumo_selfplay_amd import matches
    env = _env("RoboSumo-Ant-vs-Ant-v0", 40)
    table = _table(env, 3, seed=1)
    pairs = [(0, 1), (1, 0), (2, 2)]
    res = matches.play_matches(env, table, pairs, rounds_per_env=2, envs_per_pair=12, deterministic=False, seed=7, chunk=128)
    assert len(res) == 3
    for r in res:
        assert r["rounds"] == 24 == r["wins"] + r["losses"] + r["draws"]
        assert r["env_steps"] > 0 and r["env_steps"] % (128 * 12) == 0
    assert env.adjust_z == -0.5
    # the same games step by step: identical results
    res2 = matches.play_matches(env, table, pairs, rounds_per_env=2, envs_per_pair=12, deterministic=False, seed=7, chunk=128, fused=False)
    assert res == res2
    # counters stop at the quota even though the envs keep playing
    env.reset_device()
    sc = torch.zeros((40, 3), dtype=torch.int32, device="cuda")
    st = _states(40)
    i = torch.zeros(40, dtype=torch.int32, device="cuda")
    for _ in range(3):
        matches.match_steps_fused_lstm(env, table, i, i, st, sc, 1, 256)
    assert sc.sum(1).max().item() == 1 and sc.sum(1).min().item() == 1
    # an index outside the table is loud
    bad = i.clone(); bad[3] = 3
    with pytest.raises(Exception, match="cut short"):
        matches.match_steps_fused_lstm(env, table, i, bad, st, sc, 1, 4)
    # the fused path plays LSTM(128) only; the step-by-step path takes LSTM(64) as well
    t64 = _table(env, 2, H=64)
    with pytest.raises(ValueError, match="LSTM\\(128\\)"):
        matches.play_matches(env, t64, [(0, 1)], 1, 8, chunk=64)
    r64 = matches.play_matches(env, t64, [(0, 1)], 1, 8, chunk=256, fused=False)
    assert r64[0]["rounds"] == 8
    env.close()


def test_refusals_on_the_device():
    import torch
    from robosumo_selfplay_amd import capi, ppo_capi
    env = _env("RoboSumo-Ant-vs-Ant-v0", 16)
    table = _table(env, 2)
    i = torch.zeros(16, dtype=torch.int32, device="cuda")
    sc = torch.zeros((16, 3), dtype=torch.int32, device="cuda")
    st = _states(16)
    env.reset_device()
    E = env.engine
    bufs = [env.act_dev.data_ptr(), env.obs_dev.data_ptr(), env.info_dev.data_ptr(), env.done_dev.data_ptr(), env.ep_r_dev.data_ptr(),
            env.ep_dr_dev.data_ptr(), env.ep_l_dev.data_ptr()]
    keep = []

    def proto(**kw):
        p = ppo_capi.LstmNet.from_buffer_copy(table.proto)
        for k, v in kw.items():
            setattr(p, k, v)
        keep.append(p)
        return C.addressof(p)

    def mo(**kw):
        m = capi.MatchLstm(proto=proto(), nets_dev=table.nets_dev.data_ptr(), idx0=i.data_ptr(), idx1=i.data_ptr(), nsnap=2,
                           state0=st[0].data_ptr(), state1=st[1].data_ptr(), T=4, s0=0, K=4, quota=1, score=sc.data_ptr())
        for k, v in kw.items():
            setattr(m, k, v)
        return m
    with pytest.raises(capi.SumoHipError, match="nsnap"):
        E.match_steps_lstm(mo(nsnap=0), *bufs)
    with pytest.raises(capi.SumoHipError, match="state"):
        E.match_steps_lstm(mo(state1=None), *bufs)
    with pytest.raises(capi.SumoHipError, match="noise"):
        E.match_steps_lstm(mo(noise0=sc.data_ptr()), *bufs)
    with pytest.raises(capi.SumoHipError, match="do not match"):
        E.match_steps_lstm(mo(proto=proto(ob_dim=table.spec.ob_dim + 1)), *bufs)
    with pytest.raises(capi.SumoHipError, match="hidden 128"):
        E.match_steps_lstm(mo(proto=proto(hidden=64)), *bufs)
    with pytest.raises(capi.SumoHipError, match="gate order"):
        E.match_steps_lstm(mo(proto=proto(gate_order=ppo_capi.LSTM_GATES_IJFO)), *bufs)
    with pytest.raises(capi.SumoHipError, match="embedding"):
        E.match_steps_lstm(mo(proto=proto(emb_dim=16, emb_w=table.params.data_ptr())), *bufs)
    with pytest.raises(capi.SumoHipError, match="observation filter"):
        E.match_steps_lstm(mo(proto=proto(obs_mean=table.params.data_ptr(), obs_invstd=table.params.data_ptr())), *bufs)
    with pytest.raises(capi.SumoHipError, match="missing weights"):
        E.match_steps_lstm(mo(proto=proto(head_w=None)), *bufs)
    with pytest.raises(capi.SumoHipError, match="missing buffer"):
        E.match_steps_lstm(mo(nets_dev=None), *bufs)
    E.set_cfrc_mode("rne_post")
    with pytest.raises(capi.SumoHipError, match="rne_post"):
        E.match_steps_lstm(mo(), *bufs)
    E.set_cfrc_mode("zero")
    E.match_steps_lstm(mo(), *bufs)
    E.rollout_status()
    env.close()


def test_compare_versions_cli_end_to_end_on_lstm_runs(tmp_path):
    import compare_versions
    from robosumo_selfplay_amd import matches
    from robosumo_selfplay_amd.lstm_model import LstmPPOModel, LstmSpec
    spec = LstmSpec(121, 8, 128)
    rng = np.random.default_rng(2)
    runs = []
    for name, n in (("p1", 3), ("p2", 2)):
        m = LstmPPOModel(policy=spec, trainable=False)
        for v in range(n + 1):
            m.set_param_list(_plist(121, 8, rng))
            m.save(str(tmp_path / name / "checkpoints" / ("%.5i" % v)))
        runs.append(str(tmp_path / name))
    with pytest.warns(UserWarning):
        rec = compare_versions.main(["--p1", runs[0], "--p2", runs[1], "--trials", "8", "--num_env", "16", "--seed", "3"])
    assert (rec["network"], rec["nlstm"]) == ("lstm", 128)
    assert rec["versions"] == [["00001", "00001"], ["00002", "00002"]]
    saved = json.load(open(os.path.join(runs[0], "compare_versions_vs_p2.json")))
    assert saved["win_rate"] == rec["win_rate"] and saved["network"] == "lstm"
    for r in rec["results"]:
        assert r["rounds"] == 8
    with pytest.warns(UserWarning):
        ref = matches.compare_history_versions(runs[0], runs[1], 8, num_env=16, seed=3, fused=False)
    assert ref["win_rate"] == rec["win_rate"] and ref["results"] == rec["results"]

    rr = compare_versions.main(["--path", runs[0], "--round_robin", "--trials", "4", "--num_env", "24", "--seed", "1"])
    assert rr["versions"] == ["00001", "00002", "00003"] and rr["network"] == "lstm"
    ref = matches.round_robin(runs[0], 1, 4, num_env=24, seed=1, fused=False)
    for i in range(3):
        for j in range(3):
            if i != j:
                assert rr["win"][i][j] == ref["win"][i, j] and rr["draw"][i][j] == ref["draw"][i, j] and rr["loss"][i][j] == ref["loss"][i, j]
                assert abs(rr["win"][i][j] + rr["draw"][i][j] + rr["loss"][i][j] - 1.0) < 1e-12
    assert json.load(open(os.path.join(runs[0], "round_robin.json")))["network"] == "lstm"
