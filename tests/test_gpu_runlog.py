"""The run's files and the evaluation inside learn() on the GPU (robosumo_selfplay_amd/runlog.py, train_eval.py): that they leave
training exactly as it was, that an evaluation returns what the offline evaluator returns on the checkpoint of the same update
(dict equality, no tolerance), that the files hold what ``history`` holds, and the other learners (LSTM(128), LSTM(64) step by
step, A2C).  Episodes are cut at 40 steps so that an evaluation ends within one 64-step launch."""
import dataclasses
import json
import os
import pickle

import numpy as np
import pytest

from conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch
    from robosumo_selfplay_amd import alg_ac, alg_ppo, matches, mjcf, policy_zoo, runlog, runner as runner_mod, train_eval
    from robosumo_selfplay_amd.vec_env import SumoVecEnv

HERE = os.path.dirname(os.path.abspath(__file__))
ENV_ID = "RoboSumo-Ant-vs-Ant-v0"
TIMING = ("fps", "rollout_s", "update_s", "select_s", "eval")
MLP_KW = dict(value_network="copy", num_hidden=64, activation="relu")


def _golden(name):
    with np.load(os.path.join(HERE, "golden", "zoo_v3_params.npz"), allow_pickle=False) as z:
        return z[name].copy()


def _env(num_envs, limit, seed=3):
    return SumoVecEnv(ENV_ID, num_envs=num_envs, seed=seed, model=dataclasses.replace(mjcf.load_model(ENV_ID), timestep_limit=limit))


def _ppo(log_dir, env, **kw):
    args = dict(network="mlp", env=env, seed=3, total_timesteps=32 * 8 * 3, nagent=2, log_dir=log_dir, verbose=False, nsteps=8, nminibatches=2,
                noptepochs=1, lr=3e-4, gamma=0.995, lam=0.95, rho_bar=1.0, c_bar=1.0, opponent_mode="random", anneal_bound=1000, log_interval=1)
    args.update(MLP_KW if kw.get("network", "mlp") == "mlp" else {})
    args.update(kw)
    return alg_ppo.learn(**args)


def _rates(r):
    n = float(r["rounds"])
    return dict(win=r["wins"] / n, draw=r["draws"] / n, lose=r["losses"] / n, rounds=r["rounds"], env_steps=r["env_steps"])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The common setup twice: with the run log and an evaluation at every update, and with the defaults.  Training episodes are
    cut at 6 steps so that every rollout harvests some; ``counts`` holds len(epinfos) per update, ``rows_seen`` the monitor
    file's rows when ``update_fn`` ran (the update's own episodes are flushed after it) and ``stats`` the training env's counters
    before and after every evaluation."""
    root = tmp_path_factory.mktemp("runlog")
    zoo = str(root / "ant-mlp-v3.npy")
    np.save(zoo, _golden("ant-mlp-v3"))
    out = dict(zoo=zoo, eval_env=_env(16, 40, seed=0))
    for name in ("logged", "plain"):
        log_dir = str(root / name)
        env = _env(32, 6)
        counts, rows_seen, stats = [], [], []
        run0, eval0 = runner_mod.Runner.run, train_eval.Evaluator.evaluate

        def run(self, update, _run0=run0):
            res = _run0(self, update)
            counts.append(len(res[11]))
            return res

        def evaluate(self, update, timesteps, _eval0=eval0, _env=env):
            before = _env.stats()
            entry = _eval0(self, update, timesteps)
            stats.append((before, _env.stats(), _env.adjust_z, self.env.adjust_z))
            return entry

        def update_fn(update, _dir=log_dir):
            path = os.path.join(_dir, runlog.MONITOR_FILE)
            rows_seen.append(len(open(path).read().splitlines()) - 2 if os.path.exists(path) else None)

        runner_mod.Runner.run, train_eval.Evaluator.evaluate = run, evaluate
        try:
            kw = dict(run_log=True, eval_interval=1, eval_opponents=[zoo, "00000"], eval_trials=16, eval_num_env=16,
                      eval_env=out["eval_env"]) if name == "logged" else {}
            model = _ppo(log_dir, env, update_fn=update_fn, **kw)
        finally:
            runner_mod.Runner.run, train_eval.Evaluator.evaluate = run0, eval0
        out[name] = dict(dir=log_dir, model=model, counts=counts, rows_seen=rows_seen, stats=stats, adjust_z=env.adjust_z)
        env.close()
    yield out
    out["eval_env"].close()


def _same_series(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same_series(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def test_logging_and_evaluation_leave_training_as_it_was(runs):
    a, b = runs["logged"], runs["plain"]
    names = sorted(os.listdir(os.path.join(a["dir"], "checkpoints")))
    assert names == sorted(os.listdir(os.path.join(b["dir"], "checkpoints"))) == ["00000", "00001", "00002", "00003"]
    for n in names:
        with open(os.path.join(a["dir"], "checkpoints", n), "rb") as f, open(os.path.join(b["dir"], "checkpoints", n), "rb") as g:
            assert f.read() == g.read(), n
    assert torch.equal(a["model"].params, b["model"].params)
    ha, hb = a["model"].history, b["model"].history
    assert set(ha) - set(hb) == {"eval"} and set(hb) <= set(ha) and len(ha["eval"]) == 3
    for k in hb:
        if k not in TIMING:
            assert _same_series(ha[k], hb[k]), k
    assert a["counts"] == b["counts"] and sum(a["counts"]) > 0
    # with the defaults the run writes what it wrote before: config-free directory, checkpoints only
    assert os.listdir(b["dir"]) == ["checkpoints"] and b["rows_seen"] == [None, None, None]


def test_evaluation_equals_the_offline_evaluator(runs):
    a, env = runs["logged"], runs["eval_env"]
    spec = a["model"].spec
    A = spec.ac_dim
    zoo_table = policy_zoo.ZooTable([runs["zoo"]], A, env.device)
    for entry in a["model"].history["eval"]:
        u = entry["update"]
        ck = os.path.join(a["dir"], "checkpoints")
        table = matches.SnapshotTable.from_checkpoints(spec, [os.path.join(ck, "%.5i" % u), os.path.join(ck, "00000")], env.device)
        off_zoo = matches.play_against_zoo(env, table, zoo_table, [(0, 0)], 1, 16, deterministic=True, seed=0)[0]
        off_ck = matches.play_matches(env, table, [(0, 1)], 1, 16, deterministic=True, seed=0)[0]
        got = [{k: r[k] for k in ("win", "draw", "lose", "rounds", "env_steps")} for r in entry["results"]]
        assert got == [_rates(off_zoo), _rates(off_ck)], u
        assert [r["opponent"] for r in entry["results"]] == [runs["zoo"], "00000"] and [r["network"] for r in entry["results"]] == ["mlp", "mlp"]
        assert entry["timesteps"] == u * 32 * 8 and entry["seconds"] > 0 and all(r["rounds"] == 16 for r in entry["results"])


def test_files_hold_what_history_holds(runs):
    pandas = pytest.importorskip("pandas")
    a = runs["logged"]
    d, h, model = a["dir"], a["model"].history, a["model"]
    for name in ("log.txt", "progress.csv", runlog.MONITOR_FILE, "history.json", "early_stop_info.pkl", "ratio_summary.pkl",
                 "eval_against_fix.json", "eval_against_fix.pkl"):
        assert os.path.getsize(os.path.join(d, name)) > 0, name
    plain = pandas.read_csv(os.path.join(d, "progress.csv"))
    # pandas' default float parser is not exact on 17-digit values: the table's shape is checked on it, equality on its exact parser
    df = pandas.read_csv(os.path.join(d, "progress.csv"), float_precision="round_trip")
    assert plain.shape == df.shape and list(plain.columns) == list(df.columns) and not plain.isna().any().any()
    assert len(df) == 3 and list(df["misc/nupdates"]) == [1, 2, 3] and list(df["misc/total_timesteps"]) == [256, 512, 768]
    assert list(df["fps"]) == [float(x) for x in h["fps"]]
    for j, name in enumerate(model.loss_names):
        assert list(df["loss/" + name]) == [float(l[j]) for l in h["lossvals"]]
    for k in range(2):
        for name in ("win", "draw", "lose"):
            assert list(df["eval/%d/%s" % (k, name)]) == [e["results"][k][name] for e in h["eval"]]
    assert list(df["opponent_version"]) == [v[0] for v in h["opponent_versions"]] and list(df["version_gap"]) == list(h["version_gap"])
    assert np.isfinite(df["misc/explained_variance"]).all() and list(df["eprewmean"]) == list(df["epdenserewmean"])
    # eprewmean: the mean over the last 100 harvested episodes, i.e. over the monitor file's rows so far
    with open(os.path.join(d, runlog.MONITOR_FILE)) as f:
        head = json.loads(f.readline()[1:])
        mon = pandas.read_csv(f, index_col=None, float_precision="round_trip")
    assert head["env_id"] == ENV_ID and head["eval_opponents"] == [runs["zoo"], "00000"] and list(mon.columns) == ["r", "l", "t"]
    assert len(mon) == sum(a["counts"]) and a["rows_seen"] == [0, a["counts"][0], a["counts"][0] + a["counts"][1]]
    assert list(mon["t"]) == sorted(mon["t"]) and len(set(mon["t"])) == len([c for c in a["counts"] if c])
    done = np.cumsum(a["counts"])
    for i in range(3):
        assert df["eprewmean"][i] == np.mean(list(mon["r"][:done[i]])[-100:]) and df["eplenmean"][i] == np.mean(list(mon["l"][:done[i]])[-100:])
    with open(os.path.join(d, "eval_against_fix.pkl"), "rb") as f:
        assert pickle.load(f) == [[e["update"], e["results"][0]["win"], e["results"][0]["draw"], e["results"][0]["lose"]] for e in h["eval"]]
    with open(os.path.join(d, "eval_against_fix.json")) as f:
        assert json.load(f) == json.loads(json.dumps(runlog.to_jsonable(h["eval"])))
    with open(os.path.join(d, "history.json")) as f:
        back = json.load(f)
    assert back["fps"] == [float(x) for x in h["fps"]] and back["eval_opponents"] == [runs["zoo"], "00000"] and len(back["eval"]) == 3
    with open(os.path.join(d, "early_stop_info.pkl"), "rb") as f:
        assert pickle.load(f) == [None, None, None]
    with open(os.path.join(d, "ratio_summary.pkl"), "rb") as f:          # written at update 1 (random mode): one entry per list
        rs = pickle.load(f)
    assert len(rs) == 9 and rs[0] == [0] and rs[2] == rs[4] == h["off_env_ratio_clip_frac"][:1] and rs[6] == h["total_ratio_clip_frac"][0]
    keys = sorted(df.columns)
    with open(os.path.join(d, "log.txt")) as f:
        lines = f.readlines()
    for k in keys:                      # plot.py::parse_log on every key: three values, those of progress.csv to three digits
        got = [float(l.split("|")[2].strip()) for l in lines if k in l]
        assert len(got) == 3, k
        for g, w in zip(got, df[k]):
            exp = float(w) if float(w).is_integer() and k.split("/")[-1] in ("nupdates", "total_timesteps", "serial_timesteps") else float("%-8.3g" % w)
            assert g == exp or (np.isnan(g) and np.isnan(exp)), (k, g, w)


def test_training_env_untouched_by_evaluation(runs):
    a = runs["logged"]
    assert len(a["stats"]) == 3 and a["adjust_z"] == 0.0 and runs["eval_env"].adjust_z == 0.0
    for before, after, train_z, eval_z in a["stats"]:
        assert before == after and train_z == 0.0 and eval_z == 0.0          # the drivers restore the shared eval env's adjust_z


def _check_files(d, model, n_opponents):
    h = model.history
    assert len(h["eval"]) == 1 and len(h["eval"][0]["results"]) == n_opponents
    for r in h["eval"][0]["results"]:
        assert r["rounds"] == 16 and np.isfinite([r["win"], r["draw"], r["lose"]]).all() and abs(r["win"] + r["draw"] + r["lose"] - 1.0) < 1e-12
    for name in ("log.txt", "progress.csv", runlog.MONITOR_FILE, "history.json", "eval_against_fix.json", "eval_against_fix.pkl"):
        assert os.path.getsize(os.path.join(d, name)) > 0, name
    with open(os.path.join(d, "progress.csv")) as f:
        head, row = f.read().splitlines()
    kv = dict(zip(head.split(","), row.split(",")))
    assert float(kv["eval/0/win"]) == h["eval"][0]["results"][0]["win"] and float(kv["fps"]) == float(h["fps"][0])
    for name in model.loss_names:
        assert np.isfinite(float(kv["loss/" + name]))


@pytest.mark.parametrize("nlstm", [128, 64])
def test_lstm_learner_logs_and_evaluates(tmp_path, monkeypatch, nlstm):
    """LSTM(128) evaluates in the fused launches, LSTM(64) step by step (the fused match launches hold LSTM(128) only)."""
    zoo = str(tmp_path / "ant-lstm-v3.npy")
    np.save(zoo, _golden("ant-lstm-v3"))
    fused_flags, steps0 = [], matches.pairing_steps
    monkeypatch.setattr(matches, "pairing_steps", lambda *a, **k: fused_flags.append(a[9]) or steps0(*a, **k))
    env, eval_env = _env(16, 6), _env(16, 40, seed=0)
    try:
        model = _ppo(str(tmp_path / "run"), env, network="lstm", nlstm=nlstm, total_timesteps=16 * 8, run_log=True, eval_interval=1,
                     eval_opponents=[zoo, "00000"], eval_trials=16, eval_env=eval_env, opponent_mode="latest")
    finally:
        env.close()
        eval_env.close()
    _check_files(str(tmp_path / "run"), model, 2)
    assert [r["network"] for r in model.history["eval"][0]["results"]] == ["lstm", "lstm"]
    assert fused_flags and all(f is (nlstm == 128) for f in fused_flags)


def test_a2c_learner_logs_and_evaluates(tmp_path):
    """alg_ac.learn with an env of the evaluation's own (``eval_num_env`` envs of the training env's id and model)."""
    zoo = str(tmp_path / "ant-mlp-v3.npy")
    np.save(zoo, _golden("ant-mlp-v3"))
    env = _env(32, 40)
    try:
        model = alg_ac.learn(network="mlp", env=env, seed=3, total_timesteps=32 * 5, nagent=2, log_dir=str(tmp_path / "run"), verbose=False, nsteps=5,
                             log_interval=1, run_log=True, eval_interval=1, eval_opponents=[zoo, "00000"], eval_trials=16, eval_num_env=16, **MLP_KW)
        assert env.adjust_z == 0.0
    finally:
        env.close()
    _check_files(str(tmp_path / "run"), model, 2)
    assert "early_stop_info.pkl" not in os.listdir(str(tmp_path / "run"))          # the A2C learner has no KL early stop
