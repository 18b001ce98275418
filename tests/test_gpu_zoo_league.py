"""Training against a league of policy-zoo nets, MLP and LSTM mixed (learn(opponent_mode='fix', fix_opponent_path=[files]);
include/sumo_hip.h sumo_rollout_steps_zoo_league / sumo_rollout_steps_lstm_zoo_league) on the GPU: the fused launches against the
step-by-step league path (Runner._evaluate_step: ZooLeague.score / act) bit for bit, each tile against a single-net run of its
member, leagues of one family through the existing launches' index arrays, the bad-entry status path, the refusals, learn() end to end.

Every rollout: Ant-vs-Ant, 64 envs (4 tiles of 16), T = 6 steps in two launches of 3 (SUMO_ROLLOUT_CHUNK), episodes that end
inside the window."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import has_gpu
from zoo_lstm_helpers import golden, synthetic_lstm_flat

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch
    from robosumo_selfplay_amd import capi, lstm_model, policies, policy_zoo
    from robosumo_selfplay_amd.model import PPOModel
    from robosumo_selfplay_amd.runner import Runner
    from robosumo_selfplay_amd.vec_env import SumoVecEnv

NAMES = ["obs", "returns", "masks", "actions", "values", "neglogpacs", "rewards", "opp_neglogpacs", "opp_obs", "opp_actions", "states",
         "epinfos", "off_policy_ratio", "off_env_ratio", "total_ratio"]
ANT = "RoboSumo-Ant-vs-Ant-v0"
N, T, CHUNK = 64, 6, 3
D, A = 121, 8


def synthetic_mlp_flat(Dz, A_, seed):
    """A zoo-MLP-shaped vector with a non-trivial observation filter and O(1) weights (as tests/test_gpu_zoo_fused.py builds it)."""
    rng = np.random.default_rng(seed)
    sh = policy_zoo.zoo_mlp_shapes(Dz, A_)
    cnt = 1000.0
    parts = []
    for k in policy_zoo._ZOO_MLP_ORDER:
        s = sh[k]
        if k.endswith("/count"):
            v = np.array(cnt)
        elif k.endswith("/sum"):
            v = cnt * rng.normal(0, 0.5, s)
        elif k.endswith("/sumsq"):
            v = cnt * (0.25 + rng.uniform(0.0, 2.0, s))
        elif k == "logstd":
            v = rng.normal(-1.0, 0.3, s)
        elif k.endswith("/w"):
            v = rng.normal(0, 1.0 / np.sqrt(s[0]), s)
        else:
            v = rng.normal(0, 0.1, s)
        parts.append(np.asarray(v, np.float32).ravel())
    return np.concatenate(parts)


def _members(which):
    """'mixed': golden ant-mlp-v3, two synthetic LSTM nets, one synthetic MLP net; 'mlp' / 'lstm': three nets of one family."""
    if which == "mixed":
        return [golden("ant-mlp-v3"), synthetic_lstm_flat(D - 1, A, 21), synthetic_lstm_flat(D - 1, A, 22), synthetic_mlp_flat(D - 1, A, 23)]
    if which == "mlp":
        return [golden("ant-mlp-v3"), synthetic_mlp_flat(D - 1, A, 23), synthetic_mlp_flat(D - 1, A, 24)]
    return [golden("ant-lstm-v3"), synthetic_lstm_flat(D - 1, A, 21), synthetic_lstm_flat(D - 1, A, 22)]


def _mlp_learner(seed=3):
    np.random.seed(seed)
    spec = policies.PolicySpec(D, A, value_network="copy", activation="relu")
    m = PPOModel(policy=spec, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, trainable=False)
    rng = np.random.RandomState(seed)
    m.set_param_list([p + rng.normal(0, 0.1, p.shape).astype(np.float32) for p in m.get_param_list()])
    return m


def _lstm_learner(seed=5, H=128):
    np.random.seed(seed)
    m = lstm_model.LstmPPOModel(policy=lstm_model.LstmSpec(D, A, H), nbatch_act=N, nsteps=T, trainable=False)
    rng = np.random.default_rng(seed)
    m.set_param_list([p + rng.normal(0, 0.3 if p.ndim == 2 and p.shape[0] == H else 0.02, p.shape).astype(np.float32) for p in m.get_param_list()])
    return m


def _runner(env, network, opponent, offset=0):
    """What learn(network=..., opponent_mode='fix') builds; ``opponent``: a list of flat vectors (a league, dealt with rotation
    ``offset``) or one flat vector (the single net of the existing paths).  Seeds: learner 101, agent 1's generator 202."""
    if isinstance(opponent, list):
        zoo = policy_zoo.ZooLeague([policy_zoo.load_zoo_policy_from_flat(f, A) for f in opponent], env.num_envs, env.device)
        zoo.assign(offset)
    else:
        zoo = policy_zoo.load_zoo_policy_from_flat(opponent, A)
    if network == "lstm":
        learner = _lstm_learner()
        r = Runner(env=env, models=[learner, _lstm_learner(seed=6)], nsteps=T, nagent=2, gamma=0.995, lam=0.95, rho_bar=1.0, c_bar=1.0, anneal_bound=500)
        learner.seed(101)
        r.models[1] = policy_zoo.FixedOpponentModel(zoo)
    else:
        learner = _mlp_learner()
        learner.act_model.seed(101)
        r = Runner(env=env, models=[learner, policy_zoo.FixedOpponentModel(zoo)], nsteps=T, nagent=2, gamma=0.995, lam=0.95, rho_bar=1.0,
                   c_bar=1.0, anneal_bound=500)
    zoo.seed(202)
    r.fused_fix_opponent = True
    return r, zoo


def _near_time_limit(env):
    """Episodes end (auto-reset, both agents' state resets) at different steps inside the six-step window: env e runs out of time in
    its step 7 - e % 7, so the envs with e % 7 == 0 do not reset at all."""
    for E in env.engines:
        qpos, qvel, warm, cnt = E.get_state()
        cnt[:, 0] = env.model.timestep_limit - 6 + (np.arange(len(cnt)) % 7)
        E.set_state(qpos, qvel, warm, cnt)


def _bytes_equal(x, y):
    x, y = (z.cpu().numpy() if torch.is_tensor(z) else np.asarray(z) for z in (x, y))
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


def _rollout(network, opponent, fused, monkeypatch, groups=1, offset=0):
    monkeypatch.setenv("SUMO_FUSED_ROLLOUT", "1" if fused else "0")
    monkeypatch.setenv("SUMO_ROLLOUT_CHUNK", str(CHUNK))
    env = SumoVecEnv(ANT, num_envs=N, seed=11, groups=groups)
    assert (env.observation_space[0].shape[0], env.action_space[0].shape[0]) == (D, A)
    r, zoo = _runner(env, network, opponent, offset)
    assert r.rollout_chunk == CHUNK                                   # K = 6 in two launches: s0 = 0, 3
    if isinstance(opponent, list):
        assert r.league_opponent() is zoo and r.fused_league_ok() == fused
        assert r.zoo_opponent() is None and r.lstm_zoo_opponent() is None and not r.fused_ok() and not r.fused_lstm_ok()
    else:
        assert r.league_opponent() is None and not r.fused_league_ok()
    _near_time_limit(env)
    out = r.run(250)
    torch.cuda.synchronize()
    res = dict(out=out, env=[E.get_state() for E in env.engines], aborts=env.stats()["rollout_aborts"],
               zoo_state=(zoo.state if isinstance(opponent, list) else r.zoo_state).clone(),
               states0=r.states[0].clone() if network == "lstm" else None, scores=r.league_scores,
               tiles=None if not isinstance(opponent, list) else zoo.tile_member.copy())
    env.close()
    return res


def _assert_same_rollout(f, s, network, lstm_members):
    assert f["aborts"] == 0 and s["aborts"] == 0
    for k, (x, y) in enumerate(zip(f["out"], s["out"])):
        if torch.is_tensor(x):
            assert _bytes_equal(x, y), NAMES[k]
        else:
            assert x == y, NAMES[k]
    for a, b in zip(f["env"], s["env"]):
        for x, y in zip(a, b):
            assert _bytes_equal(x, y)
    assert _bytes_equal(f["zoo_state"], s["zoo_state"])
    if lstm_members:
        assert float(f["zoo_state"].abs().max()) > 0
    if network == "lstm":
        assert _bytes_equal(f["states0"], s["states0"]) and float(f["states0"].abs().max()) > 0
    masks = f["out"][2]
    assert len(f["out"][11]) > 0 and bool(masks[0].any()) and bool(masks[1].any()), "no episode ended inside the window"
    assert not bool(masks[0].reshape(N, T)[:, 1:].any(dim=1).all()), "every env reset: the carried-over states are never exercised"
    assert all(bool(torch.isfinite(f["out"][k]).all()) for k in (3, 4, 5, 7))


# ---- 1. mixed leagues: fused == step by step ------------------------------------------------------------------------------------
@pytest.mark.parametrize("network,groups", [("mlp", 1), ("mlp", 2), ("lstm", 1), ("lstm", 2)])
def test_mixed_league_launch_matches_stepwise_path(network, groups, monkeypatch):
    """sumo_rollout_steps_zoo_league (MLP learner) / sumo_rollout_steps_lstm_zoo_league (LSTM(128) learner) against the
    step-by-step league path on the same noise rows: every returned array, the episode records, the env states, the zoo LSTM state
    rows and the learner's recurrent state are bit-identical.  groups = 2: env_offset = 32 indexes tile_entry_dev."""
    flats = _members("mixed")
    f = _rollout(network, flats, True, monkeypatch, groups)
    s = _rollout(network, flats, False, monkeypatch, groups)
    assert f["tiles"].tolist() == [0, 1, 2, 3]                        # every tile faces another member
    _assert_same_rollout(f, s, network, True)
    # only envs on LSTM tiles (1 and 2) use their rows of the league's state
    zs = f["zoo_state"].reshape(4, 16, 128)
    assert float(zs[0].abs().max()) == 0 and float(zs[3].abs().max()) == 0 and float(zs[1].abs().max()) > 0 and float(zs[2].abs().max()) > 0
    assert np.array_equal(f["scores"], s["scores"]) and f["scores"].shape == (4, 4) and f["scores"][:, 0].sum() == len(f["out"][11])


# ---- 2. each member really plays its tile ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("network", ["mlp", "lstm"])
def test_each_tile_faces_its_member(network, monkeypatch):
    """On the tile dealt to member m, agent 1's actions and the opponent neglogps of the league launch equal those of the existing
    single-net launch against m alone (same seeds, hence the same noise rows, and the same initial env state): one MLP tile, one
    LSTM tile, with a rotation so that entry != tile index."""
    flats = _members("mixed")
    lg = _rollout(network, flats, True, monkeypatch, offset=1)
    assert lg["tiles"].tolist() == [1, 2, 3, 0]
    h = lambda res, k, *tail: res["out"][k].reshape(2, N, T, *tail)   # sf01 order: env-major rows
    for tile, member in ((3, 0), (0, 1)):                             # golden MLP net on tile 3, the first LSTM net on tile 0
        one = _rollout(network, flats[member], True, monkeypatch)
        rows = slice(16 * tile, 16 * tile + 16)
        for k, tail in ((3, (A,)), (7, ()), (0, (D,)), (5, ())):
            assert _bytes_equal(h(lg, k, *tail)[:, rows], h(one, k, *tail)[:, rows]), (tile, NAMES[k])
        other = slice(16 * ((tile + 1) % 4), 16 * ((tile + 1) % 4) + 16)
        assert not _bytes_equal(h(lg, 3, A)[1, other], h(one, 3, A)[1, other])          # ... and the neighbouring tile faces another net
        if member == 1:
            assert _bytes_equal(lg["zoo_state"][rows], one["zoo_state"][rows])


# ---- 3. leagues of one family: the existing launches with their index arrays filled ------------------------------------------
@pytest.mark.parametrize("network,family", [("mlp", "mlp"), ("lstm", "lstm"), ("mlp", "lstm"), ("lstm", "mlp")])
def test_single_family_league_matches_stepwise_path(network, family, monkeypatch):
    """Three members of one family: opponent_index (modes 4 / 8) and tile_net_dev (modes 9 / 10) select rows > 0."""
    flats = _members(family)
    f = _rollout(network, flats, True, monkeypatch)
    s = _rollout(network, flats, False, monkeypatch)
    assert f["tiles"].tolist() == [0, 1, 2, 0]
    _assert_same_rollout(f, s, network, family == "lstm")
    acts = f["out"][3].reshape(2, N, T, A)[1]
    assert not _bytes_equal(acts[0:16], acts[16:32])


# ---- 4. the launches' status path and refusals --------------------------------------------------------------------------------
def _raw(env, network, zoo, r):
    """A hand-filled league launch of the whole window on engine 0."""
    B = r._alloc_device(T)
    noise = [torch.randn((T, N, A), device="cuda") for _ in range(2)]
    n = len(zoo.members)
    if network == "lstm":
        def ro(**kw):
            o = capi.RolloutLstm(learner=C.addressof(r.models[0]._net), opponents_dev=None, tile_net_dev=None, npool=n,
                                 state0=r.states[0].data_ptr(), state1=None, T=T, Ntot=N, env_offset=0, s0=0, K=T, alpha=0.5,
                                 noise0=noise[0].data_ptr(), noise1=noise[1].data_ptr())
            for f in ("obs", "act", "rew", "val", "nlp", "onlp", "done", "ep_done", "ep_r", "ep_l"):
                setattr(o, f, B[f].data_ptr())
            for k, v in kw.items():
                setattr(o, k, v)
            return o
        launch = env.engine.rollout_steps_lstm_zoo_league
    else:
        learner = r.models[0].act_model
        def ro(**kw):
            o = capi.Rollout(learner_params=learner.params.data_ptr(), opponent_params=None, opponent_index=None, npool=n, ob_dim=D, ac_dim=A,
                             T=T, Ntot=N, env_offset=0, s0=0, K=T, alpha=0.5, noise0=noise[0].data_ptr(), noise1=noise[1].data_ptr())
            for f in ("obs", "act", "rew", "val", "nlp", "onlp", "done", "ep_done", "ep_r", "ep_l"):
                setattr(o, f, B[f].data_ptr())
            for k, v in kw.items():
                setattr(o, k, v)
            return o
        launch = env.engine.rollout_steps_zoo_league
    return ro, launch, (B, noise)


@pytest.mark.parametrize("network", ["mlp", "lstm"])
def test_bad_entry_and_refusals(network):
    """A tile entry = nmlp + nlstm: the launch's abort flag, sumo_rollout_status -20 as capi.SumoHipError('... cut short ...'); the
    process and the env stay usable.  Then what is refused before any launch."""
    env = SumoVecEnv(ANT, num_envs=N, seed=2)
    r, zoo = _runner(env, network, _members("mixed"))
    ro, launch, keep = _raw(env, network, zoo, r)
    bufs = env.env_ptrs(0)
    E = env.engine

    def zs(tile_entry=None, **kw):
        z = zoo.struct(zoo.state)
        if tile_entry is not None:
            z.tile_entry_dev = tile_entry.data_ptr()
        for k, v in kw.items():
            obj, f = (z.mlp, k[4:]) if k.startswith("mlp_") else (z.lstm, k[5:]) if k.startswith("lstm_") else (z, k)
            setattr(obj, f, v)
        return z

    launch(ro(), zs(), *bufs)                                         # a good launch
    assert E.rollout_status()["aborted"] == 0
    bad = zoo.tile_entry.clone(); bad[2] = zoo.nmlp + zoo.nlstm
    launch(ro(), zs(bad), *bufs)
    with pytest.raises(capi.SumoHipError, match="cut short"):
        E.rollout_status()
    env.reset_device()
    launch(ro(), zs(), *bufs)                                         # the env and the process stay usable
    assert E.rollout_status()["aborted"] == 0
    for field, rkw, zkw in (("npool", dict(npool=3), {}), ("npool", dict(npool=5), {}), ("nzoo", dict(npool=2), dict(mlp_nzoo=0)),
                            ("nzoo", dict(npool=2), dict(lstm_nzoo=0)), ("params", {}, dict(mlp_params=None)), ("filt", {}, dict(lstm_filt=None)),
                            ("state", {}, dict(lstm_state=None)), ("ob_dim", {}, dict(mlp_ob_dim=D + 1)), ("hidden", {}, dict(lstm_hidden=128)),
                            ("obs_clip", {}, dict(mlp_obs_clip=0.0)), ("missing", dict(noise1=None), {}), ("outside", dict(K=T + 1), {}),
                            ("multiples of 16", dict(env_offset=8, Ntot=N + 8), {})):
        with pytest.raises(capi.SumoHipError, match=field):
            launch(ro(**rkw), zs(**zkw), *bufs)
    extra = dict(tile_net_dev=zoo.tile_entry.data_ptr()) if network == "lstm" else dict(opponent_index=zoo.env_entry.data_ptr())
    with pytest.raises(capi.SumoHipError, match="must be NULL"):
        launch(ro(**extra), zs(), *bufs)
    E.set_cfrc_mode("rne_post")
    with pytest.raises(capi.SumoHipError, match="rne_post"):
        launch(ro(), zs(), *bufs)
    E.set_cfrc_mode("zero")
    with pytest.raises(ValueError, match="one family"):
        policy_zoo.ZooLeague([policy_zoo.load_zoo_policy_from_flat(f, A) for f in _members("mlp")], N, env.device).struct(zoo.state)
    env.reset_device()
    del keep
    env.close()


def test_league_falls_back_to_the_stepwise_path(monkeypatch):
    """Without the opt-in, and with rne_post, a league plays step by step (on whole-buffer noise rows all the same)."""
    monkeypatch.setenv("SUMO_FUSED_ROLLOUT", "1")
    env = SumoVecEnv(ANT, num_envs=N, seed=3)
    r, zoo = _runner(env, "mlp", _members("mixed"))
    assert r.fused_league_ok()
    r.fused_fix_opponent = False
    assert r.league_opponent() is zoo and not r.fused_league_ok()
    out = r.run(250)
    assert torch.isfinite(out[4]).all() and torch.isfinite(out[7]).all() and float(zoo.state.abs().max()) > 0
    # LSTM members of another width are refused at construction: the league keeps one [N][128] state for all of them
    wide = policy_zoo.ZooLSTMPolicy(np.zeros(policy_zoo.zoo_lstm_param_count(D - 1, A, 64, 32), np.float32) + 1.0, A, emb=64, hidden=32)
    with pytest.raises(ValueError, match="embedding and cell of 64"):
        policy_zoo.ZooLeague([zoo.members[0], wide], N, env.device)
    # a Runner that kept no tally (host mode) leaves a None row and no log note
    from robosumo_selfplay_amd import alg_ppo
    hist = dict(league_scores=[], league_tiles=[])
    r.league_scores = None
    assert alg_ppo.league_note(hist, r, zoo) == "" and hist["league_scores"] == [None] and hist["league_tiles"] == [[0, 1, 2, 3]]
    # a member change zeroes the rows of the tiles concerned, and only those
    zoo.state.fill_(1.0)
    zoo.assign(4)                                                     # 4 members: the same deal
    assert float(zoo.state.min()) == 1.0
    zoo.assign(1)
    assert float(zoo.state.abs().max()) == 0.0
    env.close()


# ---- 5. learn end to end ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("network", ["mlp", "lstm"])
def test_learn_against_a_league(network, tmp_path, monkeypatch):
    from robosumo_selfplay_amd import alg_ppo
    monkeypatch.setenv("SUMO_FUSED_ROLLOUT", "1")
    paths = [os.path.join(str(tmp_path), n) for n in ("mlp.npy", "lstm.npy")]
    np.save(paths[0], golden("ant-mlp-v3")); np.save(paths[1], synthetic_lstm_flat(D - 1, A, 7))
    env = SumoVecEnv(ANT, num_envs=N, seed=1)
    kw = dict(nlstm=128) if network == "lstm" else dict(value_network="copy", num_hidden=64, activation="relu")
    seen = []
    log = os.path.join(str(tmp_path), "log")
    with pytest.raises(ValueError, match="fixed opponent"):
        alg_ppo.learn(network=network, env=env, seed=1, total_timesteps=N * 8, nagent=2, log_dir=os.path.join(str(tmp_path), "pool"), verbose=False,
                      nsteps=8, opponent_mode="fix", fix_opponent_path=paths, opponent_pool=2, **kw)
    model = alg_ppo.learn(network=network, env=env, seed=1, total_timesteps=N * 8 * 2, nagent=2, log_dir=log, verbose=False, nsteps=8,
                          nminibatches=4, noptepochs=2, lr=1e-3, gamma=0.995, lam=1.0, rho_bar=10.0, c_bar=1.0, opponent_mode="fix",
                          fix_opponent_path=paths, anneal_bound=1000, fused_fix_opponent=True, **kw)
    hist = model.history
    assert len(hist["lossvals"]) == 2 and all(np.isfinite(l).all() for l in hist["lossvals"]) and sum(hist["env_rollout_aborts"]) == 0
    assert torch.isfinite(model.params).all()
    assert len(hist["league_scores"]) == 2 and all(np.asarray(sc).shape == (2, 4) for sc in hist["league_scores"])
    assert hist["league_tiles"][0] == [0, 1, 0, 1] and hist["league_tiles"][1] == [1, 0, 1, 0]       # the deal rotates per update
    assert sorted(os.listdir(os.path.join(log, "checkpoints")))[:3] == ["00000", "00001", "00002"]
    env.close()
    with pytest.raises(ValueError, match=r"3 members.*nenvs = 32"):
        small = SumoVecEnv(ANT, num_envs=32, seed=1)
        try:
            alg_ppo.learn(network=network, env=small, seed=1, total_timesteps=32 * 8, nagent=2, log_dir=os.path.join(str(tmp_path), "small"),
                          verbose=False, nsteps=8, opponent_mode="fix", fix_opponent_path=paths + paths[:1], **kw)
        finally:
            small.close()
