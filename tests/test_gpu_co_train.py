"""Two species co-trained on RoboSumo-Ant-vs-Bug-v0 (robosumo_selfplay_amd/co_train.py): the PairRunner's fused step against its
definition, who plays which table row in which half of the envs, ``co_train.learn`` end to end and run to run, and the matches between
the two sides' checkpoints (``play_checkpoint_pairs``, ``compare_versions.py``, ``eval_against_fix.py`` on ``<log_dir>/agent0``)."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import has_gpu

pytestmark = pytest.mark.gpu
if has_gpu():
    import torch
    from robosumo_selfplay_amd import co_train, mixed, policies, ppo_capi
    from robosumo_selfplay_amd.model import PPOModel
    from robosumo_selfplay_amd.vec_env import SumoVecEnv

HERE = os.path.dirname(os.path.abspath(__file__))
ENV_ID = "RoboSumo-Ant-vs-Bug-v0"
DIMS = ((121, 8), (165, 12))
LEARN = dict(total_timesteps=3 * 16 * 8, nsteps=8, nminibatches=2, noptepochs=1, verbose=False)


def _models(seed=5):
    np.random.seed(seed)
    out = []
    for s, (D, A) in enumerate(DIMS):
        spec = policies.PolicySpec(D, A, value_network="copy", activation="relu")
        m = PPOModel(policy=spec, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, trainable=False)
        m.act_model.seed(100 + 17 * s)
        out.append(m)
    return out


def _frozen(seed):
    rng = np.random.default_rng(seed)
    return [(0.1 * rng.standard_normal(ppo_capi.lib().ppo_param_count(D, A))).astype(np.float32) for D, A in DIMS]


def _rollouts(N, T, groups, fused, nrollouts):
    env = SumoVecEnv(ENV_ID, num_envs=N, seed=3, groups=groups)
    models = _models()
    r = co_train.PairRunner(env, models, T, 0.995, 0.95, anneal_bound=10, fused=fused)
    for s, v in enumerate(_frozen(9)):
        r.set_frozen(s, v)
    outs = [r.run(u + 1) for u in range(nrollouts)]
    torch.cuda.synchronize()
    bufs = r.last_buffers
    env.close()
    return outs, bufs, r


def _assert_same_rollout(a, b):
    assert len(a) == len(b) == 15
    for k, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, tuple):
            assert torch.equal(x[0], y[0]) and x[1] is None and y[1] is None, k
        elif x is None:
            assert y is None, k
        elif torch.is_tensor(x):
            assert torch.equal(x, y), k
        else:
            assert list(x) == list(y), k                        # the episode records


@pytest.mark.parametrize("N,T,groups,nroll", [(32, 6, 1, 2), (64, 4, 2, 1)], ids=["32x6-two-rollouts", "64x4-two-groups"])
def test_runner_fused_equals_definition(N, T, groups, nroll):
    f, bf, rf = _rollouts(N, T, groups, True, nroll)
    d, bd, rd = _rollouts(N, T, groups, False, nroll)
    assert rf.fused and not rd.fused
    for u in range(nroll):
        for side in range(2):
            _assert_same_rollout(f[u][side], d[u][side])
            ro = f[u][side]
            D, A = DIMS[side]
            n = N // 2 * T
            assert tuple(ro[0][0].shape) == (n, D) and tuple(ro[3][0].shape) == (n, A)
            for k in (1, 2, 4, 5, 6, 7):
                assert tuple(ro[k].shape) == (2, n), k
            for k in (12, 13, 14):
                assert tuple(ro[k].shape) == (n,) and bool((ro[k] == 1.0).all()), k
            assert torch.isfinite(ro[1][0]).all() and bool((ro[1][1] == 0).all()) and bool(torch.isinf(ro[5][1]).all())
    if groups == 2:          # the number of env groups does not change the numbers
        one, _, _ = _rollouts(N, T, 1, True, nroll)
        for side in range(2):
            _assert_same_rollout(f[0][side], one[0][side])


def test_who_plays_which_row():
    N, T = 32, 2
    _, B, r = _rollouts(N, T, 1, True, 1)
    models, frozen = _models(), _frozen(9)
    L = ppo_capi.lib()
    st = torch.cuda.current_stream().cuda_stream
    for side, (D, A) in enumerate(DIMS):
        b = B["side"][side]
        assert torch.equal(r.seats[side].table[0], models[side].params)         # the live row is the model's vector
        assert torch.equal(r.seats[side].table[1].cpu(), torch.from_numpy(frozen[side]))
        live_half = co_train.own_envs(N, side)
        for half in (slice(0, N // 2), slice(N // 2, N)):
            row = 0 if half == live_half else 1
            for s in range(T):
                obs = b["obs"][s, half].contiguous()
                act, nlp, val = torch.empty((16, A), device="cuda"), torch.empty(16, device="cuda"), torch.empty(16, device="cuda")
                ppo_capi.chk(L.ppo_forward(r.seats[side].table[row].data_ptr(), obs.data_ptr(), 16, D, D, A, ppo_capi.FWD_PI | ppo_capi.FWD_VF,
                                           b["noise"][s, half].contiguous().data_ptr(), None, act.data_ptr(), nlp.data_ptr(), val.data_ptr(),
                                           None, st))
                torch.cuda.synchronize()
                assert torch.equal(b["act"][s, half], act) and torch.equal(b["nlp"][s, half], nlp) and torch.equal(b["val"][s, half], val)
                other = torch.empty((16, A), device="cuda")
                ppo_capi.chk(L.ppo_forward(r.seats[side].table[1 - row].data_ptr(), obs.data_ptr(), 16, D, D, A, ppo_capi.FWD_PI,
                                           b["noise"][s, half].contiguous().data_ptr(), None, other.data_ptr(), nlp.data_ptr(), None, None, st))
                torch.cuda.synchronize()
                assert not torch.equal(other, act)              # and the rows do differ


def _learn(log, seed=4, mode="latest"):
    env = SumoVecEnv(ENV_ID, num_envs=32, seed=1)
    try:
        return co_train.learn(env=env, seed=seed, opponent_mode=mode, log_dir=log, log_interval=1, value_network="copy", num_hidden=64,
                              activation="relu", **LEARN)
    finally:
        env.close()


def _checkpoint_bytes(log):
    out = {}
    for s in range(2):
        ck = os.path.join(log, "agent%d" % s, "checkpoints")
        assert sorted(os.listdir(ck)) == ["00000", "00001", "00002", "00003"]
        for f in sorted(os.listdir(ck)):
            out[(s, f)] = open(os.path.join(ck, f), "rb").read()
    return out


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """The training run the tests below look at: three updates of 32 envs x 8 steps, 'latest'."""
    tmp = tmp_path_factory.mktemp("co_train")
    log = os.path.join(str(tmp), "log")
    models = _learn(log)
    return dict(models=models, log=log, tmp=str(tmp))


def test_learn_trains_both_species(run):
    data = _checkpoint_bytes(run["log"])
    for s, (D, A) in enumerate(DIMS):
        m = run["models"][s]
        assert (m.spec.ob_dim, m.spec.ac_dim) == (D, A) and torch.isfinite(m.params).all()
        probe = PPOModel(policy=policies.PolicySpec(D, A, value_network="copy", activation="relu"), trainable=False)
        rows = []
        for name in ("00000", "00001", "00002", "00003"):
            probe.load(os.path.join(run["log"], "agent%d" % s, "checkpoints", name))
            rows.append(probe.params.clone())
        assert torch.equal(rows[3], m.params) and all(not torch.equal(rows[k], rows[k + 1]) for k in range(3))
        h = m.history
        for k, v in h.items():
            assert len(v) == 3 or k == "version_gap", k          # 'latest' notes a gap at update 1 only, as alg_ppo.select_opponents
        assert h["opponent_versions"] == [[0], [1], [2]] and h["version_gap"] == [0]
        assert h["useful_ratio"] == [0.0] * 3 and h["total_ratio_mean"] == [1.0] * 3
        assert all(np.isfinite(l).all() for l in h["lossvals"])
        assert data[(s, "00000")] != data[(s, "00003")]


def test_learn_is_reproducible_and_the_definition_trains_the_same(run, tmp_path, monkeypatch):
    base = _checkpoint_bytes(run["log"])
    again = os.path.join(str(tmp_path), "again")
    _learn(again)
    assert _checkpoint_bytes(again) == base
    monkeypatch.setenv("SUMO_MIXED_STEP", "0")
    stepwise = os.path.join(str(tmp_path), "stepwise")
    _learn(stepwise)
    assert _checkpoint_bytes(stepwise) == base


def test_random_mode_records_the_predicted_versions(tmp_path):
    from test_co_train_cpu import predicted_random_versions
    seed = 6
    m0, m1 = _learn(os.path.join(str(tmp_path), "random"), seed=seed, mode="random")
    np.random.seed(seed)                                        # learn's draws before the first selection: the two models' initial weights
    for D, A in DIMS:
        policies.init_param_list(D, A)
    rng = np.random.RandomState()
    rng.set_state(np.random.get_state())
    want = predicted_random_versions(rng, 3)
    assert m0.history["opponent_versions"] == want[0] and m1.history["opponent_versions"] == want[1]
    assert m0.history["version_gap"] == [0] + [u - 1 - want[0][u - 1][0] for u in (2, 3)]
    assert all(len(v) == 3 for m in (m0, m1) for v in m.history.values())


def _seats(log, ids=("00001", "00003")):
    return [mixed.LearnerSeat(D, A, [os.path.join(log, "agent%d" % s, "checkpoints", c) for c in ids], device=0) for s, (D, A) in enumerate(DIMS)]


def test_play_checkpoint_pairs(run):
    env = SumoVecEnv(ENV_ID, num_envs=32, seed=2)
    seat0, seat1 = _seats(run["log"])
    pairs = [(0, 1), (1, 0)]
    kw = dict(rounds_per_env=1, envs_per_pair=16, deterministic=False, seed=3, chunk=32)
    res = co_train.play_checkpoint_pairs(env, seat0, seat1, pairs, fused=True, **kw)
    for r in res:
        assert r["wins"] + r["losses"] + r["draws"] == r["rounds"] == 16 and r["env_steps"] > 0
    assert co_train.play_checkpoint_pairs(env, seat0, seat1, pairs, fused=False, **kw) == res
    # a pair played alone sits in the first env block with the first batch's seeds: pair 0 of the batch
    alone = co_train.play_checkpoint_pairs(env, seat0, seat1, pairs[:1], fused=True, **kw)
    assert {k: alone[0][k] for k in ("wins", "losses", "draws", "rounds")} == {k: res[0][k] for k in ("wins", "losses", "draws", "rounds")}
    with pytest.raises(ValueError, match="non-existent net"):
        co_train.play_checkpoint_pairs(env, seat0, seat1, [(0, 2)], **kw)
    with pytest.raises(ValueError, match="another species"):
        mixed.LearnerSeat(165, 12, [os.path.join(run["log"], "agent0", "checkpoints", "00001")], device=0)
    env.close()


def test_compare_versions_cli(run, tmp_path):
    sys.path.insert(0, os.path.dirname(HERE))
    import compare_versions
    out = os.path.join(str(tmp_path), "cmp.json")
    rec = compare_versions.main(["--p1", os.path.join(run["log"], "agent0"), "--p2", os.path.join(run["log"], "agent1"), "--env", ENV_ID,
                                 "--trials", "16", "--num_env", "32", "--interval", "2", "--out", out])
    assert rec == json.load(open(out))
    assert rec["mode"] == "paired" and rec["network"] == "mlp" and rec["versions"] == [["00001", "00001"], ["00003", "00003"]]
    for w, r in zip(rec["win_rate"], rec["results"]):
        assert r["rounds"] == 16 and r["wins"] + r["losses"] + r["draws"] == 16 and w == r["wins"] / 16.0


def test_eval_against_fix_reads_an_agent_directory(run, tmp_path):
    sys.path.insert(0, os.path.dirname(HERE))
    import eval_against_fix
    with np.load(os.path.join(HERE, "golden", "zoo_v3_params.npz"), allow_pickle=False) as z:
        bug = os.path.join(str(tmp_path), "bug-mlp.npy")
        np.save(bug, z["bug-mlp-v3"])
    path = os.path.join(run["log"], "agent0")
    tab = eval_against_fix.main(["--path", path, "--env", ENV_ID, "--fused", "--trials", "16", "--num_env", "32", "--interval", "3",
                                 "--opponent_path", bug])
    assert tab.shape == (2, 4) and tab[:, 0].tolist() == [0, 3] and np.allclose(tab[:, 1:4].sum(1), 1.0)
    assert os.path.isfile(os.path.join(path, "eval_against_fix.json"))


def test_run_py_co_train(tmp_path):
    sys.path.insert(0, os.path.dirname(HERE))
    import run as run_py
    m0, m1 = run_py.main(["--co_train", "--env", ENV_ID, "--num_env", "32", "--num_timesteps", "256", "--seed", "4", "--log_path", str(tmp_path),
                          "--suffix", "t", "--nsteps=8", "--nminibatches=2", "--noptepochs=1", "--opponent_mode=random", "--verbose=False"])
    log = os.path.join(str(tmp_path), ENV_ID + "-t")
    assert os.path.isfile(os.path.join(log, "config.pkl"))
    for s, m in enumerate((m0, m1)):
        assert sorted(os.listdir(os.path.join(log, "agent%d" % s, "checkpoints"))) == ["00000", "00001", "00002"]
        assert (m.spec.ob_dim, m.spec.ac_dim) == DIMS[s] and len(m.history["opponent_versions"]) == 2 and torch.isfinite(m.params).all()
