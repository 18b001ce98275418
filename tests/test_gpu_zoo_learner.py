"""Fine-tuning a policy-zoo MLP net on the GPU (robosumo_selfplay_amd/zoo_learner.py): ``ZooPPOModel`` acts as ``ZooMLPPolicy`` does,
steps as the float64 reference tests/zoo_grad_ref.py followed by the oracle's clip + Adam, replays its HIP graph bit for bit, writes
checkpoints that are zoo files, and ``learn(network='zoo_mlp')`` runs in self-play and against a fixed zoo net."""
import os

import numpy as np
import pytest

import zoo_grad_ref as Z
from conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch
    from oracle import ppo_oracle as po
    from robosumo_selfplay_amd import alg_ppo, policies, policy_zoo, ppo_capi, zoo_learner, zoo_pairs
    from robosumo_selfplay_amd.runner import Runner
    from robosumo_selfplay_amd.vec_env import SumoVecEnv

    DEV = torch.device("cuda:0")

HERE = os.path.dirname(os.path.abspath(__file__))
AC = {"ant": 8, "bug": 12, "spider": 16}


def _zoo(name):
    with np.load(os.path.join(HERE, "golden", "zoo_v3_params.npz"), allow_pickle=False) as z:
        return z[name].copy()


def _spec(name="ant-mlp-v3"):
    flat = _zoo(name)
    ac = AC[name.split("-")[0]]
    return zoo_learner.ZooMlpSpec(policy_zoo.infer_ob_dim(flat.size, ac) + 1, ac, flat)


def _model(spec=None, trainable=True, **kw):
    return zoo_learner.ZooPPOModel(policy=spec or _spec(), ent_coef=kw.pop("ent_coef", 0.0), vf_coef=0.5, max_grad_norm=0.5, trainable=trainable, **kw)


def _batch(spec, n, seed=3):
    """A fixed batch around the net's own statistics: raw rows of the env's width (the time feature rides along), actions near the
    net's mean, returns near its value."""
    rng = np.random.RandomState(seed)
    D, A = spec.ob_dim, spec.ac_dim
    obs = (spec.obs_mean + spec.obs_std * rng.normal(0, 1.5, (n, D))).astype(np.float32)
    obs = np.concatenate([obs, rng.uniform(0, 1, (n, 1)).astype(np.float32)], axis=1)
    filt = (spec.obs_mean, (np.float32(1.0) / spec.obs_std).astype(np.float32), 5.0)
    pl = policies.unflatten_params(policy_zoo.zoo_kernel_flat(spec.tensors), D, A)
    mean, value, _ = Z.forward(pl, obs[:, :D], filt, spec.ret_std, spec.ret_mean)
    logstd = pl[10].astype(np.float64)
    act = (mean + np.exp(logstd) * rng.normal(0, 1, (n, A))).astype(np.float32)
    old = (po.neglogp(mean, logstd, act) + rng.normal(0, 0.2, n)).astype(np.float32)
    val = value.astype(np.float32)
    ret = (value + spec.ret_std * rng.normal(0, 0.5, n)).astype(np.float32)
    return dict(obs=obs, act=act, old=old, val=val, ret=ret, w=np.ones(n, np.float32), filt=filt, pl=pl)


def test_model_starts_as_the_file_and_draws_nothing():
    np.random.seed(11)
    state = np.random.get_state()[1].copy()
    spec = _spec()
    m = _model(spec)
    assert np.array_equal(np.random.get_state()[1], state)
    assert np.array_equal(m.params.cpu().numpy(), policy_zoo.zoo_kernel_flat(spec.tensors)) and m.recurrent is False
    assert m.act_model.params is m.params and isinstance(m.act_model, policy_zoo.ZooMLPPolicy)
    with pytest.raises(NotImplementedError, match="no comm"):
        _model(spec, comm=object())


def test_act_model_is_the_zoo_policy_bit_for_bit():
    spec = _spec()
    m, zoo = _model(spec, trainable=False), policy_zoo.ZooMLPPolicy(spec.flat, spec.ac_dim)
    b = _batch(spec, 37)
    obs = torch.as_tensor(b["obs"]).to(DEV)
    noise = torch.randn((37, spec.ac_dim), device=DEV, dtype=torch.float32)
    flags = ppo_capi.FWD_PI | ppo_capi.FWD_VF
    for kw in (dict(noise=noise), dict(deterministic=True), dict(given_action=torch.as_tensor(b["act"]).to(DEV))):
        x, y = m.act_model.evaluate(obs, flags, **kw), zoo.evaluate(obs, flags, **kw)
        for k in ("action", "neglogp", "value"):
            assert torch.equal(x[k], y[k]), k
    m.act_model.seed(4); zoo.seed(4)
    for x, y in zip(m.step(b["obs"]), zoo.step(b["obs"])):
        assert x is y is None or np.array_equal(x, y)


def test_train_step_matches_the_reference():
    """One optimiser step on 64 rows: the parameters afterwards within 5e-6 of reference gradient -> clip_by_global_norm -> adam_step."""
    spec = _spec()
    m, n = _model(spec), 64
    b = _batch(spec, n)
    out = m.train(1e-3, 0.2, b["obs"], b["ret"], np.zeros(n, bool), b["act"], b["val"], b["old"], b["ret"], b["w"])
    assert len(out) == 7 and out[5].shape == (n,)
    advs = po.normalize_advantages(b["ret"], b["val"])
    _, stats, lr, grads = Z.loss_and_grads(b["pl"], b["obs"][:, :spec.ob_dim], b["act"], advs, b["ret"], b["old"], b["w"], 0.2, 0.0, 0.5,
                                           filt=b["filt"], v_scale=spec.ret_std, v_shift=spec.ret_mean)
    gc, _ = po.clip_by_global_norm([np.asarray(g, np.float64) for g in grads], 0.5)
    p64 = [p.astype(np.float64) for p in b["pl"]]
    newp, _, _ = po.adam_step(p64, [g.reshape(p.shape) for g, p in zip(gc, p64)], [np.zeros_like(p) for p in p64],
                              [np.zeros_like(p) for p in p64], 1, 1e-3)
    for k, (a, e) in enumerate(zip(m.get_param_list(), newp)):
        assert np.allclose(a, e, rtol=0, atol=5e-6), (policies.PARAM_NAMES[k], np.abs(a - e).max())
    assert float(out[0]) == pytest.approx(stats[0], rel=1e-3, abs=1e-5) and float(out[1]) == pytest.approx(stats[1], rel=1e-4)
    assert float(out[2]) == pytest.approx(stats[2], rel=1e-6) and float(out[3]) == pytest.approx(stats[3], rel=1e-3, abs=1e-5)
    assert np.allclose(out[5], lr, rtol=1e-4, atol=1e-4)


def _dev_batch(b):
    return [torch.as_tensor(b[k]).to(DEV) for k in ("obs", "ret", "act", "val", "old", "w")]


def test_graph_replay_equals_the_eager_steps_and_lr_zero_keeps_the_parameters():
    spec = _spec()
    b = _batch(spec, 96)
    batch = _dev_batch(b)
    raw = batch[0].clone()
    gen = torch.Generator(device=DEV)
    runs = []
    for use_graph in (True, False):
        m = _model(spec)
        m.use_graph = use_graph
        gen.manual_seed(9)
        m.begin_update(*batch)
        assert torch.equal(batch[0], raw)                                # the caller's rows stay raw: the model filters its own copy
        assert torch.equal(m._static["bufs"][0][:, spec.ob_dim:], raw[:, spec.ob_dim:])          # the time feature is not touched
        outs = []
        for k in range(3):
            idx = torch.randperm(96, device=DEV, generator=gen)[:48].to(torch.int32)
            outs.append(m.train_indexed(1e-3, 0.2, *batch, idx, 48, sync=False).clone())
        m.end_update()
        torch.cuda.synchronize()
        assert len(m._graphs) == (1 if use_graph else 0)                 # one captured step, replayed; none on the eager model
        runs.append((m.params.clone(), torch.stack(outs)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert not torch.equal(runs[0][0], torch.as_tensor(policy_zoo.zoo_kernel_flat(spec.tensors)).to(DEV))
    # lr = 0: the step runs and leaves every bit where it was
    m = _model(spec)
    before = m.params.clone()
    m.begin_update(*batch)
    st = m.train_indexed(0.0, 0.2, *batch, torch.arange(48, device=DEV, dtype=torch.int32), 48, sync=True)
    m.end_update()
    assert np.isfinite(st[:5]).all() and torch.equal(m.params, before) and m.t == 1
    with pytest.raises(RuntimeError, match="begin_update"):
        m.train_indexed(0.0, 0.2, *batch, None, 96)


def test_ten_steps_lower_the_reference_loss():
    spec = _spec()
    m, n = _model(spec), 64
    b = _batch(spec, n)
    advs = po.normalize_advantages(b["ret"], b["val"])
    ref = lambda pl: Z.loss(pl, b["obs"][:, :spec.ob_dim], b["act"], advs, b["ret"], b["old"], b["w"], 0.2, 0.0, 0.5, filt=b["filt"],
                            v_scale=spec.ret_std, v_shift=spec.ret_mean)
    first = ref(b["pl"])
    for _ in range(10):
        m.train(1e-3, 0.2, b["obs"], b["ret"], np.zeros(n, bool), b["act"], b["val"], b["old"], b["ret"], b["w"])
    last = ref(m.get_param_list())
    print("reference loss %.6f -> %.6f" % (first, last))
    assert np.isfinite(last) and last < first


def _rollout(spec, seed=1):
    env = SumoVecEnv("RoboSumo-Ant-vs-Ant-v0", num_envs=32, seed=seed)
    learner, opp = _model(spec, model_scope="model_0"), _model(spec, trainable=False, model_scope="model_1")
    learner.act_model.seed(5); opp.act_model.seed(6)
    r = Runner(env=env, models=[learner, opp], nsteps=8, nagent=2, gamma=0.995, lam=1.0, rho_bar=10.0, c_bar=1.0, anneal_bound=1000)
    mode = r.rollout_mode()
    assert (mode.learner, mode.opponent, mode.fused, mode.one_launch, mode.noise_rows) == ("mlp", "self", False, False, False)
    return env, learner, r, r.run(1)


def test_rollout_and_first_minibatch_log_ratio():
    """32 envs x 8 steps: the gradient kernel's forward on the filtered copy re-derives the neglogp the rollout recorded."""
    spec = _spec()
    env, learner, r, out = _rollout(spec)
    obs, returns, masks, actions, values, nlp = out[:6]
    assert obs.shape == (2, 256, 121) and all(torch.isfinite(x).all() for x in (obs, returns, values, nlp, out[14]))
    assert torch.allclose(out[14], torch.ones_like(out[14]), atol=1e-4)    # the opponent holds the learner's weights
    w = torch.ones(256, dtype=torch.float32, device=DEV)
    batch = [obs[0].contiguous(), returns[0], actions[0], values[0], nlp[0], w]
    learner.begin_update(*batch)
    idx = torch.randperm(256, device=DEV).to(torch.int32)[:128].contiguous()
    st = learner.train_indexed(1e-3, 0.2, *batch, idx, 128)
    learner.end_update()
    worst = float(st[5].abs().max())
    print("first minibatch max |log-ratio| %.3g" % worst)
    assert np.isfinite(st[:5]).all() and worst <= 1e-4
    env.close()


def test_checkpoints_are_zoo_files(tmp_path):
    spec = _spec()
    src = str(tmp_path / "agent-params-v3.npy")
    np.save(src, spec.flat)
    m = _model(zoo_learner.ZooMlpSpec(121, 8, src))
    path = str(tmp_path / "checkpoints" / "00000")
    m.save(path)
    assert os.listdir(os.path.dirname(path)) == ["00000"]
    with open(path, "rb") as f, open(src, "rb") as g:
        assert f.read() == g.read()                                      # the untouched model's file is its source, byte for byte
    b = _batch(spec, 64)
    for _ in range(2):
        m.train(1e-3, 0.2, b["obs"], b["ret"], np.zeros(64, bool), b["act"], b["val"], b["old"], b["ret"], b["w"])
    path = str(tmp_path / "checkpoints" / "00002")
    m.save(path)
    flat = np.load(path, allow_pickle=False)
    assert flat.dtype == np.float32 and flat.shape == spec.flat.shape
    _, p = policy_zoo.split_zoo_mlp(flat, 8)
    for k in policy_zoo._ZOO_MLP_ORDER:
        same = np.asarray(p[k]).tobytes() == np.asarray(spec.tensors[k]).tobytes()
        assert same == (k in zoo_learner._FILTER_KEYS), k               # the filters are frozen, every trained tensor moved
    # the file plays through every zoo path unchanged
    zoo = policy_zoo.load_zoo_policy(path, 8)
    assert type(zoo) is policy_zoo.ZooMLPPolicy and torch.equal(zoo.params, m.params)
    obs = torch.as_tensor(b["obs"]).to(DEV)
    noise = torch.randn((64, 8), device=DEV, dtype=torch.float32)
    x, y = m.act_model.evaluate(obs, 3, noise=noise), zoo.evaluate(obs, 3, noise=noise)
    assert all(torch.equal(x[k], y[k]) for k in ("action", "neglogp", "value"))
    table = policy_zoo.ZooTable([path, src], 8)
    assert torch.equal(table.params[0], m.params) and torch.equal(table.filt[0], table.filt[1]) and not torch.equal(table.params[0], table.params[1])
    seat = zoo_pairs.ZooSeat([path], 120, 8)
    assert seat.kinds == ["mlp"] and torch.equal(seat.mlp_table.params[0], m.params)
    league = policy_zoo.load_zoo_league([path, src], 8, 32)
    assert len(league.members) == 2
    # load: the round trip, the 13-tensor list, and a file with other filter statistics
    m2 = _model(spec, trainable=False)
    m2.load(path)
    assert torch.equal(m2.params, m.params)
    m2.set_param_list(_model(spec, trainable=False).get_param_list())
    assert np.array_equal(m2.params.cpu().numpy(), policy_zoo.zoo_kernel_flat(spec.tensors))
    other = flat.copy()
    other[3] += 1.0                                                      # obsfilter/sum[0]
    zoo_learner.write_zoo_vector(str(tmp_path / "other"), other)
    with pytest.raises(ValueError, match="filter statistics"):
        m2.load(str(tmp_path / "other"))
    np.save(str(tmp_path / "bug.npy"), _zoo("bug-mlp-v3"))
    with pytest.raises(ValueError, match="another species"):
        m2.load(str(tmp_path / "bug.npy"))


def _learn(tmp_path, env_id="RoboSumo-Ant-vs-Ant-v0", init="ant-mlp-v3", updates=2, **kw):
    src = str(tmp_path / "init.npy")
    np.save(src, _zoo(init))
    log = str(tmp_path / "log")
    env = SumoVecEnv(env_id, num_envs=32, seed=1)
    try:
        model = alg_ppo.learn(network="zoo_mlp", zoo_init=src, env=env, seed=1, total_timesteps=256 * updates, nagent=2, log_dir=log,
                              verbose=False, nsteps=8, nminibatches=2, noptepochs=2, lr=1e-4, **kw)
    finally:
        env.close()
    return model, log, src


def _check_run(model, log, src, ac, updates=2):
    h = model.history
    assert len(h["lossvals"]) == updates and all(np.isfinite(l).all() for l in h["lossvals"]) and sum(h["env_rollout_aborts"]) == 0
    source = np.load(src, allow_pickle=False)
    ck = os.path.join(log, "checkpoints")
    names = ["%.5i" % u for u in range(updates + 1)]
    assert sorted(os.listdir(ck)) == names
    vecs = [np.load(os.path.join(ck, n), allow_pickle=False) for n in names]
    assert vecs[0].tobytes() == source.tobytes()
    for a, b in zip(vecs, vecs[1:]):
        assert a.shape == b.shape and a.dtype == np.float32 and np.isfinite(b).all() and not np.array_equal(a, b)
    assert policy_zoo.zoo_file_kind(vecs[-1].size, ac) == "mlp"
    assert np.array_equal(policy_zoo.zoo_kernel_flat(policy_zoo.split_zoo_mlp(vecs[-1], ac)[1]), model.params.cpu().numpy())
    assert torch.isfinite(model.params).all()


def test_learn_self_play_latest(tmp_path):
    model, log, src = _learn(tmp_path, opponent_mode="latest", run_log=True, log_interval=1)
    assert isinstance(model, zoo_learner.ZooPPOModel)
    _check_run(model, log, src, 8)
    assert model.history["opponent_versions"] == [[0], [1]]
    assert all(os.path.isfile(os.path.join(log, f)) for f in ("log.txt", "progress.csv", "history.json"))


def test_learn_against_a_fixed_zoo_lstm(tmp_path):
    opp = str(tmp_path / "ant-lstm-v3.npy")
    np.save(opp, _zoo("ant-lstm-v3"))
    model, log, src = _learn(tmp_path, opponent_mode="fix", fix_opponent_path=opp)
    _check_run(model, log, src, 8)


def test_learn_bug_vs_bug_one_update(tmp_path):
    model, log, src = _learn(tmp_path, env_id="RoboSumo-Bug-vs-Bug-v0", init="bug-mlp-v3", updates=1, opponent_mode="random",
                             use_opponent_data="both")
    _check_run(model, log, src, 12, updates=1)
    assert model.spec.ob_dim == 164 and model.spec.ac_dim == 12
