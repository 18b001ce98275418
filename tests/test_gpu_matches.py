"""The fused match launch (include/sumo_hip.h sumo_match_steps, robosumo_selfplay_amd/matches.py) against the step-by-step path:
per step one ppo_forward launch per side and run of envs sharing a snapshot (the kernel PPOModel.step runs), env.step_device and the
score update on the host side.  Everything is compared bit for bit: observations, info rows, done flags, qpos / qvel / warm start /
counters and the score counters.  Then the quota, play_matches' round bookkeeping and compare_versions.py end to end."""
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


def _table(env, k, seed=0, scale=0.3):
    from robosumo_selfplay_amd import matches, policies
    spec = policies.PolicySpec(env.observation_space[0].shape[0], env.action_space[0].shape[0], value_network="copy", activation="relu")
    rng = np.random.default_rng(seed)
    t = matches.SnapshotTable(spec, k, env.device)
    for j in range(k):
        plist = policies.init_param_list(spec.ob_dim, spec.ac_dim)
        plist = [p + scale * rng.standard_normal(p.shape).astype(np.float32) for p in plist]
        t.set(j, policies.flatten_params(plist))
    return t


def _state(env):
    import torch
    torch.cuda.synchronize()
    host = [x.cpu().numpy().copy() for x in (env.obs_dev, env.info_dev, env.done_dev, env.act_dev)]
    return host + list(env.engine.get_state())


CASES = [("RoboSumo-Ant-vs-Ant-v0", 96, True, "random"), ("RoboSumo-Ant-vs-Ant-v0", 96, False, "random"),
         ("RoboSumo-Spider-vs-Spider-v0", 32, False, "random"), ("RoboSumo-Spider-vs-Spider-v0", 32, True, "random"),
         ("RoboSumo-Ant-vs-Ant-v0", 4096, False, "blocks")]


@pytest.mark.parametrize("env_id,N,deterministic,layout", CASES)
def test_match_launch_equals_stepwise_path(env_id, N, deterministic, layout):
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
    # start every episode near the time limit so episodes end (and auto-reset) inside the launches
    qpos, qvel, warm, cnt = ef.engine.get_state()
    cnt[:, 0] = ef.model.timestep_limit - 40 + (np.arange(N) % 37)
    for e in (ef, es):
        e.engine.set_state(qpos, qvel, warm, cnt)
    i0, i1 = torch.from_numpy(idx0).cuda(), torch.from_numpy(idx1).cuda()
    sf = torch.zeros((N, 3), dtype=torch.int32, device="cuda")
    ss = torch.zeros_like(sf)
    quota, K = 2, 24
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    A = table.spec.ac_dim
    for chunk in range(3):
        noise = None if deterministic else tuple(torch.randn((K, N, A), generator=gen, device="cuda") for _ in range(2))
        matches.match_steps_fused(ef, table, i0, i1, sf, quota, K, noise)
        matches.match_steps_stepwise(es, table, idx0, idx1, ss, quota, K, noise)
        a, b = _state(ef), _state(es)
        for name, x, y in zip(("obs", "info", "done", "actions", "qpos", "qvel", "warm", "counters"), a, b):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (name, chunk, np.argwhere(x != y)[:5])
        assert torch.equal(sf, ss), chunk
    sc = sf.cpu().numpy()
    assert sc.sum() > 0, "no episode ended inside the launches"
    assert sc.sum(1).max() <= quota
    assert ef.stats()["rollout_aborts"] == 0
    ef.close(); es.close()


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
    assert env.adjust_z == -0.5       # the env's own value is restored (it was built with -0.5)
    # the same games step by step: identical results
    res2 = matches.play_matches(env, table, pairs, rounds_per_env=2, envs_per_pair=12, deterministic=False, seed=7, chunk=128, fused=False)
    assert res == res2
    # counters stop at the quota even though the envs keep playing
    env.reset_device()
    sc = torch.zeros((40, 3), dtype=torch.int32, device="cuda")
    i = torch.zeros(40, dtype=torch.int32, device="cuda")
    for _ in range(3):
        matches.match_steps_fused(env, table, i, i, sc, 1, 256)
    assert sc.sum(1).max().item() == 1 and sc.sum(1).min().item() == 1
    # an index outside the table is loud
    bad = i.clone(); bad[3] = 3
    with pytest.raises(Exception, match="cut short"):
        matches.match_steps_fused(env, table, bad, i, sc, 1, 4)
    env.close()


def test_refusals_on_the_device():
    import torch
    from robosumo_selfplay_amd import capi, matches
    env = _env("RoboSumo-Ant-vs-Ant-v0", 16)
    table = _table(env, 2)
    i = torch.zeros(16, dtype=torch.int32, device="cuda")
    sc = torch.zeros((16, 3), dtype=torch.int32, device="cuda")
    env.reset_device()
    E = env.engine
    bufs = [env.act_dev.data_ptr(), env.obs_dev.data_ptr(), env.info_dev.data_ptr(), env.done_dev.data_ptr(), env.ep_r_dev.data_ptr(),
            env.ep_dr_dev.data_ptr(), env.ep_l_dev.data_ptr()]

    def mo(**kw):
        m = capi.Match(params=table.params.data_ptr(), idx0=i.data_ptr(), idx1=i.data_ptr(), nsnap=2, ob_dim=table.spec.ob_dim,
                       ac_dim=table.spec.ac_dim, T=4, s0=0, K=4, quota=1, score=sc.data_ptr())
        for k, v in kw.items():
            setattr(m, k, v)
        return m
    with pytest.raises(capi.SumoHipError, match="nsnap"):
        E.match_steps(mo(nsnap=0), *bufs)
    with pytest.raises(capi.SumoHipError, match="do not match"):
        E.match_steps(mo(ob_dim=table.spec.ob_dim + 1), *bufs)
    with pytest.raises(capi.SumoHipError, match="noise"):
        E.match_steps(mo(noise0=sc.data_ptr()), *bufs)
    E.set_cfrc_mode("rne_post")
    with pytest.raises(capi.SumoHipError, match="rne_post"):
        E.match_steps(mo(), *bufs)
    E.set_cfrc_mode("zero")
    E.match_steps(mo(), *bufs)
    E.rollout_status()
    env.close()


def test_compare_versions_cli_end_to_end(tmp_path):
    import compare_versions
    from robosumo_selfplay_amd import matches
    from robosumo_selfplay_amd.model import PPOModel
    from robosumo_selfplay_amd import policies
    spec = policies.PolicySpec(121, 8, value_network="copy", activation="relu")
    rng = np.random.default_rng(2)
    runs = []
    for name, n in (("p1", 3), ("p2", 2)):
        m = PPOModel(policy=spec, trainable=False)
        base = m.get_param_list()
        for v in range(n + 1):
            m.set_param_list([p + 0.3 * rng.standard_normal(p.shape).astype(np.float32) for p in base])
            m.save(str(tmp_path / name / "checkpoints" / ("%.5i" % v)))
        runs.append(str(tmp_path / name))
    with pytest.warns(UserWarning):
        rec = compare_versions.main(["--p1", runs[0], "--p2", runs[1], "--trials", "8", "--num_env", "16", "--seed", "3"])
    assert rec["versions"] == [["00001", "00001"], ["00002", "00002"]]
    assert os.path.exists(os.path.join(runs[0], "compare_versions_vs_p2.json"))
    assert json.load(open(os.path.join(runs[0], "compare_versions_vs_p2.json")))["win_rate"] == rec["win_rate"]
    for r in rec["results"]:
        assert r["rounds"] == 8
    with pytest.warns(UserWarning):
        ref = matches.compare_history_versions(runs[0], runs[1], 8, num_env=16, seed=3, fused=False)
    assert ref["win_rate"] == rec["win_rate"] and ref["results"] == rec["results"]

    rr = compare_versions.main(["--path", runs[0], "--round_robin", "--trials", "4", "--num_env", "24", "--seed", "1"])
    assert rr["versions"] == ["00001", "00002", "00003"]
    ref = matches.round_robin(runs[0], 1, 4, num_env=24, seed=1, fused=False)
    for i in range(3):
        for j in range(3):
            if i != j:
                assert rr["win"][i][j] == ref["win"][i, j] and rr["draw"][i][j] == ref["draw"][i, j] and rr["loss"][i][j] == ref["loss"][i, j]
                assert abs(rr["win"][i][j] + rr["draw"][i][j] + rr["loss"][i][j] - 1.0) < 1e-12
    assert os.path.exists(os.path.join(runs[0], "round_robin.json"))
