"""The fused launches against policy-zoo MLP nets (include/sumo_hip.h sumo_rollout_steps_zoo / sumo_match_steps_zoo) on the GPU:
against the step-by-step launches they replace (ppo_forward, ppo_forward_filtered, sumo_step, ppo_post_step) bit for bit, against
the numpy restatement of both nets on the recorded observations, their loud failures, and the drivers built on them.

Tolerances of the numpy comparison (float32 MFMA + tanhf against numpy, as tests/test_gpu_zoo.py): 2e-5 absolute on action means,
2e-5 * (1 + max |v|) on values, 1e-3 * (1 + max |neglogp|) on likelihoods."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch
    from robosumo_selfplay_amd import capi, matches, policies, policy_zoo
    from robosumo_selfplay_amd.model import PPOModel
    from robosumo_selfplay_amd.runner import Runner
    from robosumo_selfplay_amd.vec_env import SumoVecEnv
    from oracle import ppo_oracle as po

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


def _dims(env):
    return env.observation_space[0].shape[0], env.action_space[0].shape[0]


def _table(env, k, seed=0, scale=0.3):
    D, A = _dims(env)
    spec = policies.PolicySpec(D, A, value_network="copy", activation="relu")
    rng = np.random.default_rng(seed)
    t = matches.SnapshotTable(spec, k, env.device)
    for j in range(k):
        plist = [p + scale * rng.standard_normal(p.shape).astype(np.float32) for p in policies.init_param_list(D, A)]
        t.set(j, policies.flatten_params(plist))
    return t


def _zoo_table(env, k, seed=20):
    D, A = _dims(env)
    return policy_zoo.ZooTable([_synthetic_flat(D - 1, A, seed + j) for j in range(k)], A, env.device)


def _state(env):
    torch.cuda.synchronize()
    host = [x.cpu().numpy().copy() for x in (env.obs_dev, env.info_dev, env.done_dev, env.act_dev)]
    for E in env.engines:
        host += list(E.get_state())
    return host


def _near_time_limit(envs):
    """Every episode starts near the time limit, so episodes end (and auto-reset) inside the launches."""
    for g in range(envs[0].groups):
        qpos, qvel, warm, cnt = envs[0].engines[g].get_state()
        cnt[:, 0] = envs[0].model.timestep_limit - 40 + (np.arange(len(cnt)) % 37)
        for e in envs:
            e.engines[g].set_state(qpos, qvel, warm, cnt)


# ---- 5. matches: fused == step by step ------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id,N,groups", [("RoboSumo-Ant-vs-Ant-v0", 256, 2), ("RoboSumo-Bug-vs-Bug-v0", 64, 1)])
@pytest.mark.parametrize("deterministic", [False, True])
def test_zoo_match_launch_equals_stepwise_path(env_id, N, groups, deterministic):
    ef, es = [SumoVecEnv(env_id, num_envs=N, seed=11, adjust_z=-0.5, groups=groups) for _ in range(2)]
    if "Bug" in env_id:
        assert not ef.engine.static_layout()                      # the runtime-layout kernel variant
    table, zoo = _table(ef, 4), _zoo_table(ef, 2)
    assert torch.isclose(zoo.filt[:, 1], torch.tensor(10.0, device="cuda")).any()   # variances under the 1e-2 floor: 1 / std = 10
    rng = np.random.default_rng(5)
    idx0, idx1 = rng.integers(0, 4, N).astype(np.int32), rng.integers(0, 2, N).astype(np.int32)
    for e in (ef, es):
        e.reset_device()
    _near_time_limit([ef, es])
    i0, i1 = torch.from_numpy(idx0).cuda(), torch.from_numpy(idx1).cuda()
    sf = torch.zeros((N, 3), dtype=torch.int32, device="cuda")
    ss = torch.zeros_like(sf)
    quota, K, A = 2, 32, table.spec.ac_dim
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    for chunk in range(1 if deterministic else 3):
        noise = None if deterministic else tuple(torch.randn((K, N, A), generator=gen, device="cuda") for _ in range(2))
        matches.zoo_match_steps_fused(ef, table, zoo, i0, i1, sf, quota, K, noise)
        matches.zoo_match_steps_stepwise(es, table, zoo, idx0, idx1, ss, quota, K, noise)
        torch.cuda.synchronize()
        assert torch.equal(sf, ss), chunk
        for name in ("obs_dev", "act_dev", "done_dev"):
            assert torch.equal(getattr(ef, name), getattr(es, name)), (name, chunk)
        for k, (x, y) in enumerate(zip(_state(ef), _state(es))):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (k, chunk)
    assert int(sf.sum()) > 0, "no episode ended inside the launches"
    assert int(sf.sum(1).max()) <= quota
    assert ef.stats()["rollout_aborts"] == 0
    ef.close(); es.close()


# ---- 6. rollout: fused == step by step ------------------------------------------------------------------------------------
def _learner(D, A, seed):
    np.random.seed(seed)
    spec = policies.PolicySpec(D, A, value_network="copy", activation="relu")
    m = PPOModel(policy=spec, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, trainable=False)
    rng = np.random.RandomState(seed)
    pl = [p + rng.normal(0, 0.1, p.shape).astype(np.float32) for p in m.get_param_list()]
    m.set_param_list(pl)
    return m, pl


def _fix_runner(env, T, zoo_flat, seed=3):
    D, A = _dims(env)
    learner, pl = _learner(D, A, seed)
    zoo = policy_zoo.ZooMLPPolicy(zoo_flat, A)
    learner.act_model.seed(101); zoo.seed(202)
    r = Runner(env=env, models=[learner, policy_zoo.FixedOpponentModel(zoo)], nsteps=T, nagent=2, gamma=0.995, lam=0.95, rho_bar=1.0,
               c_bar=1.0, anneal_bound=500)
    r.fused_fix_opponent = True
    return r, pl


def _zoo_rollout_pair(env_id, N, T, groups, fused, monkeypatch):
    monkeypatch.setenv("SUMO_FUSED_ROLLOUT", "1" if fused else "0")
    env = SumoVecEnv(env_id, num_envs=N, seed=11, groups=groups)
    D, A = _dims(env)
    r, _ = _fix_runner(env, T, _synthetic_flat(D - 1, A, 9))
    assert r.zoo_opponent() is not None and r.fused_zoo_ok() == fused and not r.fused_ok()
    outs = [r.run(250), r.run(251)]                     # two consecutive rollouts: episode state carries over
    torch.cuda.synchronize()
    st = [E.get_state() for E in env.engines]
    env.close()
    return outs, st


@pytest.mark.parametrize("env_id,N,T,groups", [("RoboSumo-Ant-vs-Ant-v0", 96, 24, 1), ("RoboSumo-Ant-vs-Ant-v0", 64, 12, 2),
                                               ("RoboSumo-Bug-vs-Bug-v0", 32, 8, 1)])
def test_zoo_rollout_kernel_matches_stepwise_path(env_id, N, T, groups, monkeypatch):
    """Runner.run in fix mode with the opt-in: sumo_rollout_steps_zoo against the step-by-step launches fed the same noise rows --
    every returned array, the episode records and the env states are bit-identical."""
    fo, fs = _zoo_rollout_pair(env_id, N, T, groups, True, monkeypatch)
    so, ss = _zoo_rollout_pair(env_id, N, T, groups, False, monkeypatch)
    names = ["obs", "returns", "masks", "actions", "values", "neglogpacs", "rewards", "opp_neglogpacs", "opp_obs", "opp_actions", "states",
             "epinfos", "off_policy_ratio", "off_env_ratio", "total_ratio"]
    for f, s_ in zip(fo, so):
        for k, (x, y) in enumerate(zip(f, s_)):
            if torch.is_tensor(x):
                assert torch.equal(x, y), names[k]
            else:
                assert x == y, names[k]
    for a, b in zip(fs, ss):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_learn_fused_fix_opponent_equals_stepwise(tmp_path, monkeypatch):
    from robosumo_selfplay_amd import alg_ppo
    path = os.path.join(str(tmp_path), "agent-params-test.npy")
    np.save(path, _synthetic_flat(120, 8, 7))
    params = []
    for fused in (True, False):
        monkeypatch.setenv("SUMO_FUSED_ROLLOUT", "1" if fused else "0")
        env = SumoVecEnv("RoboSumo-Ant-vs-Ant-v0", num_envs=16, seed=1)
        model = alg_ppo.learn(network="mlp", env=env, seed=1, total_timesteps=16 * 16 * 2, nagent=2,
                              log_dir=os.path.join(str(tmp_path), "log%d" % fused), verbose=False, nsteps=16, nminibatches=4, noptepochs=2,
                              lr=1e-3, gamma=0.995, lam=1.0, rho_bar=10.0, c_bar=1.0, opponent_mode="fix", fix_opponent_path=path,
                              value_network="copy", num_hidden=64, activation="relu", anneal_bound=1000, fused_fix_opponent=True)
        assert len(model.history["lossvals"]) == 2 and all(np.isfinite(l).all() for l in model.history["lossvals"])
        params.append(model.params.clone())
        env.close()
    assert torch.isfinite(params[0]).all() and torch.equal(params[0], params[1])


# ---- 7. against numpy -------------------------------------------------------------------------------------------------------
def _assert_rollout_matches_numpy_nets(env_id, zoo_flat):
    """One fused rollout against ``zoo_flat`` (None: a synthetic net of the scene's width); both nets re-evaluated in numpy on the
    recorded observations, within the tolerances of the module docstring."""
    N, T = 32, 16
    env = SumoVecEnv(env_id, num_envs=N, seed=5)
    D, A = _dims(env)
    flat = _synthetic_flat(D - 1, A, 9) if zoo_flat is None else zoo_flat
    r, pl = _fix_runner(env, T, flat)
    assert r.fused_zoo_ok()
    out = r.run(250)
    torch.cuda.synchronize()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(202)                                              # the zoo net's generator: its one [T, N, A] draw of the rollout
    noise1 = torch.randn((T, N, A), generator=gen, device="cuda", dtype=torch.float32).cpu().numpy().astype(np.float64)
    noise1 = noise1.transpose(1, 0, 2).reshape(N * T, A)              # sf01 order: env-major rows
    _, p = policy_zoo.split_zoo_mlp(flat, A)
    obs = out[0].cpu().numpy()                                        # [2, N*T, D] recorded observations
    act, val, nlp, onlp = [out[k].cpu().numpy().astype(np.float64) for k in (3, 4, 5, 7)]
    ls_l, ls_z = pl[10].astype(np.float64).ravel(), p["logstd"].astype(np.float64).ravel()
    for g in range(2):
        mean_l, v_l, _ = po.forward(pl, obs[g].astype(np.float64))
        mean_z, _, _ = po.zoo_mlp_forward(p, obs[g][:, :D - 1])
        e_val = np.abs(val[g] - v_l).max()
        e_nlp = np.abs(nlp[g] - po.neglogp(mean_l, ls_l, act[g])).max()
        e_onlp = np.abs(onlp[g] - po.neglogp(mean_z.astype(np.float64), ls_z, act[g])).max()
        print("agent %d: value err %.3g (max |v| %.3g), nlp err %.3g, onlp err %.3g" % (g, e_val, np.abs(v_l).max(), e_nlp, e_onlp))
        assert e_val < 2e-5 * (1 + np.abs(v_l).max())
        assert e_nlp < 1e-3 * (1 + np.abs(nlp[g]).max())
        assert e_onlp < 1e-3 * (1 + np.abs(onlp[g]).max())
        if g == 1:      # the zoo net's mean implied by the recorded action and its noise
            e_mean = np.abs(act[1] - np.exp(ls_z) * noise1 - mean_z).max()
            print("zoo mean err %.3g" % e_mean)
            assert e_mean < 2e-5
    env.close()


def test_zoo_rollout_matches_numpy_nets():
    _assert_rollout_matches_numpy_nets("RoboSumo-Ant-vs-Ant-v0", None)


@pytest.mark.parametrize("species", ["ant", "bug", "spider"])
def test_zoo_rollout_matches_numpy_nets_of_every_species(species):
    """The same with the golden ``<species>-mlp-v3`` net on ``<Species>-vs-<Species>``: Bug is the dynamic-layout kernel, Spider the
    widest one -- A = 16 fills the head's 16-column tile, D = 209 is the widest filter stage -- and here both meet a plain numpy
    restatement instead of another path of the same code.  The tolerances are the module's, unchanged for every species.  Measured
    worst errors (ant / bug / spider): value 2.8e-6 / 2.0e-6 / 2.4e-6 against 2e-5 * (1 + max |v|), learner neglogp 6.0e-6 / 6.0e-6 /
    1.2e-5 and zoo neglogp 1.1e-3 / 1.7e-3 / 2.6e-3 against 1e-3 * (1 + max |neglogp|) with neglogps of 10 to 500, zoo mean 5.5e-7 /
    3.9e-7 / 4.2e-7 against 2e-5: Spider needs no wider bound."""
    from zoo_lstm_helpers import golden
    _assert_rollout_matches_numpy_nets("RoboSumo-%s-vs-%s-v0" % (species.title(), species.title()), golden("%s-mlp-v3" % species))


# ---- 8. loud failures ---------------------------------------------------------------------------------------------------------
def test_zoo_launch_refusals():
    N = 16
    env = SumoVecEnv("RoboSumo-Ant-vs-Ant-v0", num_envs=N, seed=2, adjust_z=-0.5)
    D, A = _dims(env)
    table, zoo = _table(env, 2), _zoo_table(env, 2)
    env.reset_device()
    i = torch.zeros(N, dtype=torch.int32, device="cuda")
    sc = torch.zeros((N, 3), dtype=torch.int32, device="cuda")
    # a zoo index outside [0, nzoo): the launch is cut short and rollout_status raises
    bad = i.clone(); bad[3] = 2
    with pytest.raises(capi.SumoHipError, match="cut short"):
        matches.zoo_match_steps_fused(env, table, zoo, i, bad, sc, 1, 4)
    bad0 = i.clone(); bad0[5] = 2                                     # idx0 is checked against nsnap
    with pytest.raises(capi.SumoHipError, match="cut short"):
        matches.zoo_match_steps_fused(env, table, zoo, bad0, i, sc, 1, 4)
    env.reset_device()
    # the same for the rollout launch's opponent_index
    T = 4
    r, _ = _fix_runner(env, T, _synthetic_flat(D - 1, A, 9))
    B = r._alloc_device(T)
    noise = [torch.randn((T, N, A), device="cuda") for _ in range(2)]
    learner = r.models[0].act_model
    bufs = env.env_ptrs(0)

    def ro(**kw):
        o = capi.Rollout(learner_params=learner.params.data_ptr(), opponent_params=None, opponent_index=None, npool=2, ob_dim=D, ac_dim=A,
                         T=T, Ntot=N, env_offset=0, s0=0, K=T, alpha=0.5, noise0=noise[0].data_ptr(), noise1=noise[1].data_ptr())
        for f in ("obs", "act", "rew", "val", "nlp", "onlp", "done", "ep_done", "ep_r", "ep_l"):
            setattr(o, f, B[f].data_ptr())
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    E = env.engine
    E.rollout_steps_zoo(ro(), zoo.struct(), *bufs)
    E.rollout_status()
    E.rollout_steps_zoo(ro(opponent_index=bad.data_ptr()), zoo.struct(), *bufs)
    with pytest.raises(capi.SumoHipError, match="cut short"):
        E.rollout_status()
    env.reset_device()

    def zs(**kw):
        z = zoo.struct()
        for k, v in kw.items():
            setattr(z, k, v)
        return z

    # refused before any launch
    with pytest.raises(capi.SumoHipError, match="ob_dim"):
        E.rollout_steps_zoo(ro(), zs(ob_dim=D + 1), *bufs)
    with pytest.raises(capi.SumoHipError, match="nzoo"):
        E.rollout_steps_zoo(ro(), zs(nzoo=1), *bufs)                  # npool != nzoo
    with pytest.raises(capi.SumoHipError, match="opponent_params"):
        E.rollout_steps_zoo(ro(opponent_params=table.params.data_ptr()), zoo.struct(), *bufs)
    with pytest.raises(capi.SumoHipError, match="obs_clip"):
        E.rollout_steps_zoo(ro(), zs(obs_clip=0.0), *bufs)
    with pytest.raises(capi.SumoHipError, match="missing"):
        E.rollout_steps_zoo(ro(), zs(filt=None), *bufs)
    mo = capi.Match(params=table.params.data_ptr(), idx0=i.data_ptr(), idx1=i.data_ptr(), nsnap=2, ob_dim=D, ac_dim=A, T=4, s0=0, K=4,
                    quota=1, score=sc.data_ptr())
    with pytest.raises(capi.SumoHipError, match="ob_dim"):
        E.match_steps_zoo(mo, zs(ob_dim=0), *bufs)
    with pytest.raises(capi.SumoHipError, match="nzoo"):
        E.match_steps_zoo(mo, zs(nzoo=0), *bufs)
    E.set_cfrc_mode("rne_post")
    with pytest.raises(capi.SumoHipError, match="rne_post"):
        E.match_steps_zoo(mo, zoo.struct(), *bufs)
    with pytest.raises(capi.SumoHipError, match="rne_post"):
        E.rollout_steps_zoo(ro(), zoo.struct(), *bufs)
    E.set_cfrc_mode("zero")
    env.cfrc_mode = "rne_post"
    with pytest.raises(ValueError, match="rne_post"):
        matches.zoo_match_steps_fused(env, table, zoo, i, i, sc, 1, 4)
    env.cfrc_mode = "zero"
    # a zoo LSTM vector, a zoo net wider than the scene's observation
    lstm_flat = np.zeros(sum(int(np.prod(s)) for s in policy_zoo.zoo_lstm_shapes(D - 1, A).values()), np.float32)
    with pytest.raises(ValueError, match="LSTM"):
        policy_zoo.ZooTable([lstm_flat], A, env.device)
    wide = policy_zoo.ZooTable([_synthetic_flat(D + 5, A, 1)], A, env.device)
    with pytest.raises(ValueError, match="ob_dim"):
        matches.zoo_match_steps_fused(env, table, wide, i, i, sc, 1, 4)
    env.close()
    # mixed match-ups stay refused
    mixed = SumoVecEnv("RoboSumo-Ant-vs-Bug-v0", num_envs=4, seed=2)
    with pytest.raises(ValueError, match="homogeneous"):
        matches.zoo_match_steps_fused(mixed, table, zoo, i[:4], i[:4], sc[:4], 1, 4)
    with pytest.raises(capi.SumoHipError, match="homogeneous"):
        mixed.engine.match_steps_zoo(mo, zoo.struct(), *mixed.env_ptrs(0))
    mixed.close()


# ---- 9. drivers ---------------------------------------------------------------------------------------------------------------
def test_evaluate_history_against_zoo_and_cli(tmp_path):
    run = str(tmp_path / "run")
    os.makedirs(os.path.join(run, "checkpoints"))
    for k in range(1, 4):
        m, _ = _learner(121, 8, 10 + k)
        m.save(os.path.join(run, "checkpoints", "%.5i" % k))
    opp = [str(tmp_path / "v3.npy"), str(tmp_path / "synthetic.npy")]
    np.save(opp[0], _golden_v3())
    np.save(opp[1], _synthetic_flat(120, 8, 7))
    res = [matches.evaluate_history_against_zoo(run, opp, trials=64, num_env=64, fused=f) for f in (True, False)]
    assert res[0] == res[1]
    r = res[0]
    assert r["checkpoints"] == [1, 2, 3] and r["opponents"] == opp and len(r["results"]) == 6
    for key, x in r["results"].items():
        assert x["rounds"] == 64 and abs(x["win"] + x["draw"] + x["lose"] - 1.0) < 1e-12, key
    sys.path.insert(0, ROOT)
    import eval_against_fix
    tab = eval_against_fix.main(["--path", run, "--opponent_path", opp[0], "--fused", "--trials", "64", "--num_env", "64"])
    with open(os.path.join(run, "eval_against_fix.json")) as f:
        js = json.load(f)
    assert len(js) == 3 and [row[0] for row in js] == [1, 2, 3] and np.allclose(tab, np.array(js))
    for row in js:
        assert len(row) == 4 and abs(sum(row[1:]) - 1.0) < 1e-12
