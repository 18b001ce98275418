"""CPU checks of the run's files (robosumo_selfplay_amd/runlog.py), of the evaluation plan (train_eval.plan_evaluation), of the
new run.py flags and of plot_run.py.  The files are parsed with the few lines below, which restate the loading rules of the
reference's analysis code: plot.py::parse_log, pandas.read_csv on progress.csv, baselines' monitor loader."""
import json
import math
import os
import pickle
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ANT_OB, ANT_AC = 121, 8          # RoboSumo-Ant-vs-Ant-v0: observation and action width of either agent


# ---- the reference's loading rules, restated -------------------------------------------------------------------------------
def parse_log(path, element):
    out = []
    with open(path) as f:
        for line in f.readlines():
            if element in line:
                out.append(float(line.split("|")[2].strip()))
    return np.array(out)


def load_monitor(path):
    import pandas
    with open(path, "rt") as fh:
        first = fh.readline()
        assert first[0] == "#"
        header = json.loads(first[1:])
        df = pandas.read_csv(fh, index_col=None)
    return header, df


def golden(name):
    with np.load(os.path.join(HERE, "golden", "zoo_v3_params.npz"), allow_pickle=False) as z:
        return z[name].copy()


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


ROWS = [{"eprewmean": -1.5, "misc/nupdates": 1, "loss/value_loss": 1e-9, "fps": 123456.0, "misc/explained_variance": float("nan"),
         "useful_ratio": None},
        {"eprewmean": np.float32(0.25), "misc/nupdates": np.int64(2), "loss/value_loss": 0.001391924834024394, "fps": 98765.4321,
         "misc/explained_variance": 0.5, "useful_ratio": None},
        {"eprewmean": 7.0, "misc/nupdates": 3, "loss/value_loss": 0.125, "fps": 1e6, "misc/explained_variance": -0.75,
         "eval/0/win": 0.4375, "eval/0/draw": 0.5, "eval/0/lose": 0.0625, "useful_ratio": None}]


# ---- log.txt -----------------------------------------------------------------------------------------------------------------
def test_log_txt_round_trips_through_the_split_rule(tmp_path):
    from robosumo_selfplay_amd import runlog
    log = runlog.RunLog(str(tmp_path), "RoboSumo-Ant-vs-Ant-v0")
    for r in ROWS:
        log.row(r)
    keys = sorted({k for r in ROWS for k, v in r.items() if v is not None})
    assert "eval/0/win" in keys and "fps" in keys
    for k in keys:
        want = [r[k] for r in ROWS if r.get(k) is not None]
        got = parse_log(str(tmp_path / "log.txt"), k)
        assert len(got) == len(want), k
        for g, w in zip(got, want):          # three significant digits for floats (%-8.3g), integers in full
            exp = float(int(w)) if isinstance(w, (int, np.integer)) else float("%-8.3g" % float(w))
            assert same(float(g), exp), (k, g, w)
    assert parse_log(str(tmp_path / "log.txt"), "fps")[0] == 1.23e5 and parse_log(str(tmp_path / "log.txt"), "loss/value_loss")[0] == 1e-9
    text = (tmp_path / "log.txt").read_text().splitlines()
    assert set(text[0]) == {"-"} and text[1].startswith("| ") and text[1].endswith(" |")
    body = [l for l in text[1:1 + len([v for v in ROWS[0].values() if v is not None])]]
    assert [l.split("|")[1].strip() for l in body] == sorted(k for k, v in ROWS[0].items() if v is not None)      # sorted by key
    assert len({len(l) for l in text[:len(body) + 2]}) == 1                                                        # one table, one width


def test_log_keys_are_never_truncated(tmp_path):
    from robosumo_selfplay_amd import runlog
    hist = dict(fps=[1.0], rollout_s=[1.0], update_s=[1.0], useful_ratio=[0.5], off_policy_ratio_mean=[1.0], off_env_ratio_mean=[1.0],
                total_ratio_mean=[1.0], off_policy_ratio_clip_frac=[0.0], off_env_ratio_clip_frac=[0.0], total_ratio_clip_frac=[0.0],
                opponent_versions=[[3]], env_diverged=[0], env_dropped_contacts=[0], env_rollout_aborts=[0])
    entry = dict(results=[dict(win=0.5, draw=0.25, lose=0.25)] * 12)
    kv = runlog.training_row(update=7, nsteps=8, nbatch=256, explained_variance=0.1, epinfobuf=[{"r": 1.0, "l": 5}, {"r": 2.0, "l": 7}],
                             time_elapsed=3.0, loss_names=["policy_loss", "value_loss", "policy_entropy", "approxkl", "clipfrac"],
                             lossvals=[0.1, 0.2, 0.3, 0.4, 0.5], history=hist, league_scores=[[4, 1, 2, 1], [0, 0, 0, 0]], eval_entry=entry)
    assert max(len(k) for k in kv) <= runlog.KEY_WIDTH
    assert kv["eprewmean"] == 1.5 == kv["epdenserewmean"] and kv["eplenmean"] == 6.0        # the reference's line 449 averages 'r' again
    assert kv["misc/serial_timesteps"] == 56 and kv["misc/total_timesteps"] == 7 * 256 and kv["misc/nupdates"] == 7
    assert kv["opponent_version"] == 3 and kv["version_gap"] == 3 and kv["env/dropped_contacts"] == 0
    assert kv["league/0/win"] == 0.25 and math.isnan(kv["league/1/win"]) and kv["eval/11/lose"] == 0.25 and kv["loss/clipfrac"] == 0.5
    with pytest.raises(ValueError, match="longer than 30"):
        runlog.RunLog(str(tmp_path), "x").row({"k" * 31: 1.0})
    assert len(runlog.format_table({"a": "v" * 40}).splitlines()[1].split("|")[2].strip()) == 30


# ---- progress.csv --------------------------------------------------------------------------------------------------------------
def test_progress_csv_stays_rectangular_when_keys_appear_late(tmp_path):
    pandas = pytest.importorskip("pandas")
    from robosumo_selfplay_amd import runlog
    log = runlog.RunLog(str(tmp_path), "RoboSumo-Ant-vs-Ant-v0")
    for i, r in enumerate(ROWS):
        log.row(r)
        assert len(pandas.read_csv(str(tmp_path / "progress.csv"))) == i + 1            # a table after every row
    # (pandas' default float parser may miss the last place of a 17-digit value such as ROWS[1]'s loss: its exact one is asked for)
    df = pandas.read_csv(str(tmp_path / "progress.csv"), float_precision="round_trip")
    assert len(df) == 3 and list(df.columns)[-3:] == ["eval/0/draw", "eval/0/lose", "eval/0/win"] and "useful_ratio" not in df.columns
    for late in ("eval/0/win", "eval/0/draw", "eval/0/lose"):
        assert np.isnan(df[late][0]) and np.isnan(df[late][1]) and df[late][2] == ROWS[2][late]
    for i, r in enumerate(ROWS):
        for k, v in r.items():
            if v is not None:
                assert same(float(df[k][i]), float(str(runlog.plain_number(v)))), (i, k)
                assert same(float(df[k][i]), float(v))


# ---- monitor file ------------------------------------------------------------------------------------------------------------
def test_monitor_file(tmp_path):
    pytest.importorskip("pandas")
    from robosumo_selfplay_amd import runlog
    from robosumo_selfplay_amd.runner import EpInfoList
    log = runlog.RunLog(str(tmp_path), "RoboSumo-Ant-vs-Ant-v0", header=dict(eval_opponents=["a.npy", "00000"]))
    a = EpInfoList([1.25, -2.5, 1e-6], [10, 20, 30])
    b = [{"r": 3.0, "l": 7, "t": 0.0}, {"r": -1000.123456, "l": 501, "t": 0.0}]
    assert log.episodes(a) == 3 and log.episodes([]) == 0 and log.episodes(b) == 2
    header, df = load_monitor(str(tmp_path / runlog.MONITOR_FILE))
    assert header["env_id"] == "RoboSumo-Ant-vs-Ant-v0" and isinstance(header["t_start"], float) and header["eval_opponents"] == ["a.npy", "00000"]
    assert list(df.columns) == ["r", "l", "t"] and len(df) == len(a) + len(b)
    assert list(df["r"]) == [1.25, -2.5, 1e-6, 3.0, -1000.123456] and list(df["l"]) == [10, 20, 30, 7, 501]
    t = list(df["t"])
    assert all(y >= x for x, y in zip(t, t[1:])) and t[0] == t[2] and t[3] == t[4] and t[0] >= 0.0     # one time per harvested rollout


# ---- history.json and the pickles ----------------------------------------------------------------------------------------------
def test_history_json_round_trip(tmp_path):
    from robosumo_selfplay_amd import runlog
    hist = dict(fps=[np.float32(1.5), np.float32(2.25)], version_gap=[np.int64(0), np.int64(3)], opponent_versions=[[0], [1, 2]],
                early_stop_info=[None, [1, 2]], lossvals=[np.array([0.5, float("nan")]), np.array([1.0, 2.0])], approxkl=[float("nan")],
                league_scores=[None, np.arange(8).reshape(2, 4)], eval=[dict(update=1, results=[dict(win=np.float64(0.5), rounds=np.int32(16))])])
    log = runlog.RunLog(str(tmp_path), "x")
    log.history(hist, eval_opponents=("a", "b"))
    assert not os.path.exists(str(tmp_path / "history.json.tmp"))
    with open(str(tmp_path / "history.json")) as f:
        back = json.load(f)
    assert back["fps"] == [1.5, 2.25] and back["version_gap"] == [0, 3] and back["opponent_versions"] == [[0], [1, 2]]
    assert back["early_stop_info"] == [None, [1, 2]] and back["league_scores"] == [None, [[0, 1, 2, 3], [4, 5, 6, 7]]]
    assert back["lossvals"][0][0] == 0.5 and math.isnan(back["lossvals"][0][1]) and math.isnan(back["approxkl"][0])
    assert back["eval"] == [dict(update=1, results=[dict(win=0.5, rounds=16)])] and back["eval_opponents"] == ["a", "b"]
    torch = pytest.importorskip("torch")
    assert runlog.to_jsonable(dict(a=torch.tensor([1.0, 2.0]), b=torch.tensor(3))) == dict(a=[1.0, 2.0], b=3)


def test_reference_pickles(tmp_path):
    from robosumo_selfplay_amd import runlog
    log = runlog.RunLog(str(tmp_path), "x")
    log.early_stop_info([None, [0, 3]])
    with open(str(tmp_path / "early_stop_info.pkl"), "rb") as f:
        assert pickle.load(f) == [None, [0, 3]]
    h = dict(version_gap=[0, 1], off_policy_ratio_mean=[1.0, 1.1], off_policy_ratio_clip_frac=[0.0, 0.1], off_env_ratio_mean=[2.0, 2.1],
             off_env_ratio_clip_frac=[0.2, 0.3], total_ratio_mean=[3.0, 3.1], total_ratio_clip_frac=[0.4, 0.5], ppo_clip_frac=[0.6, 0.7],
             approxkl=[0.8, 0.9])
    log.ratio_summary(h)
    with open(str(tmp_path / "ratio_summary.pkl"), "rb") as f:
        got = pickle.load(f)
    # alg_ppo.py:469-472: [version_gap, off_policy_ratio_mean, off_env_ratio_clip_frac, off_env_ratio_mean, off_env_ratio_clip_frac,
    #                      total_ratio_mean, total_clip_frac (the last update's scalar), ppo_clip_frac, approxkl]
    assert got == [[0, 1], [1.0, 1.1], [0.2, 0.3], [2.0, 2.1], [0.2, 0.3], [3.0, 3.1], 0.5, [0.6, 0.7], [0.8, 0.9]]
    entries = [dict(update=1, results=[dict(win=0.25, draw=0.5, lose=0.25), dict(win=1.0, draw=0.0, lose=0.0)]),
               dict(update=5, results=[dict(win=0.5, draw=0.5, lose=0.0), dict(win=0.0, draw=0.0, lose=1.0)])]
    log.evaluation(entries)
    with open(str(tmp_path / "eval_against_fix.pkl"), "rb") as f:
        assert pickle.load(f) == [[1, 0.25, 0.5, 0.25], [5, 0.5, 0.5, 0.0]]
    with open(str(tmp_path / "eval_against_fix.json")) as f:
        assert json.load(f) == entries


# ---- the evaluation plan -------------------------------------------------------------------------------------------------------
def _files(tmp_path):
    import joblib
    from robosumo_selfplay_amd import policies
    out = {}
    for name in ("ant-mlp-v3", "ant-lstm-v3", "bug-mlp-v3"):
        out[name] = str(tmp_path / (name + ".npy"))
        np.save(out[name], golden(name))
    rng = np.random.RandomState(0)
    for name, shapes in (("mlp_ckpt", policies.param_shapes(ANT_OB, ANT_AC)), ("lstm128_ckpt", policies.lstm_param_shapes(ANT_OB, ANT_AC, 128)),
                         ("lstm64_ckpt", policies.lstm_param_shapes(ANT_OB, ANT_AC, 64))):
        out[name] = str(tmp_path / name)
        joblib.dump([rng.normal(0, 0.1, s).astype(np.float32) for s in shapes], out[name])
    return out


def _plan(**kw):
    from robosumo_selfplay_amd import train_eval
    args = dict(network="mlp", ob_dim=ANT_OB, ac_dim=ANT_AC, eval_interval=5, eval_trials=16, eval_num_env=16)
    args.update(kw)
    return train_eval.plan_evaluation(**args)


def test_eval_plan_off_by_default():
    assert _plan(eval_interval=0, eval_opponents=None) is None and _plan(eval_interval=0, eval_opponents=[]) is None


def test_eval_plan_mlp_learner(tmp_path):
    f = _files(tmp_path)
    plan = _plan(eval_opponents=[f["ant-lstm-v3"], "00000", f["ant-mlp-v3"], f["mlp_ckpt"]], eval_trials=48, eval_num_env=32)
    opp = plan["opponents"]
    assert [o["name"] for o in opp] == [f["ant-lstm-v3"], "00000", f["ant-mlp-v3"], f["mlp_ckpt"]]
    assert [o["family"] for o in opp] == ["lstm", "mlp", "mlp", "mlp"] and [o["source"] for o in opp] == ["zoo", "first", "zoo", "checkpoint"]
    assert [o["driver"] for o in opp] == ["play_against_zoo", "play_matches", "play_against_zoo", "play_matches"]
    assert [o["entry"] for o in opp] == ["sumo_match_steps_zoo_lstm", "sumo_match_steps", "sumo_match_steps_zoo", "sumo_match_steps"]
    assert all(o["fused"] for o in opp)
    assert (plan["envs_per_pair"], plan["rounds_per_env"], plan["interval"], plan["trials"]) == (24, 2, 5, 48)
    # the offline evaluator's launches: zoo MLP files, zoo LSTM files, then the checkpoints on rows 1.. of the learner's table
    assert [(g["driver"], g["family"], g["positions"], g["pairs"]) for g in plan["groups"]] == [
        ("play_against_zoo", "mlp", [2], [(0, 0)]), ("play_against_zoo", "lstm", [0], [(0, 0)]), ("play_matches", "mlp", [1, 3], [(0, 1), (0, 2)])]
    assert opp[3]["data"].shape == (sum(int(np.prod(s)) for s in __import__("robosumo_selfplay_amd.policies", fromlist=["x"]).param_shapes(ANT_OB, ANT_AC)),)


def test_eval_plan_lstm_learners(tmp_path):
    f = _files(tmp_path)
    plan = _plan(network="lstm", nlstm=128, eval_opponents=[f["ant-lstm-v3"], "00000", f["lstm128_ckpt"]])
    assert [o["entry"] for o in plan["opponents"]] == ["sumo_match_steps_lstm_zoo_lstm", "sumo_match_steps_lstm", "sumo_match_steps_lstm"]
    assert all(o["fused"] for o in plan["opponents"]) and plan["nlstm"] == 128
    plan = _plan(network="lstm", nlstm=64, eval_opponents=[f["ant-lstm-v3"], "00000", f["lstm64_ckpt"]])
    assert not any(o["fused"] for o in plan["opponents"]) and not any(g["fused"] for g in plan["groups"])        # LSTM(64): step by step
    plan = _plan(network="lstm", eval_opponents=[f["ant-mlp-v3"]], eval_cross_family=True)
    assert plan["opponents"][0]["entry"] == "sumo_match_steps_lstm_zoo" and plan["cross_family"] and plan["opponents"][0]["fused"]


def test_eval_plan_refusals(tmp_path):
    f = _files(tmp_path)
    ok = dict(eval_opponents=["00000"])
    with pytest.raises(ValueError, match="LSTM checkpoints do not play against zoo MLP nets"):
        _plan(network="lstm", eval_opponents=[f["ant-mlp-v3"]])
    with pytest.raises(ValueError, match="fit neither zoo policy with 8 actions"):          # a zoo file of another species
        _plan(eval_opponents=[f["bug-mlp-v3"]])
    with pytest.raises(ValueError, match="is an LSTM checkpoint: it plays in an LstmSnapshotTable"):
        _plan(eval_opponents=[f["lstm128_ckpt"]])
    with pytest.raises(ValueError, match="is an MLP\\(64,64\\) checkpoint"):
        _plan(network="lstm", eval_opponents=[f["mlp_ckpt"]])
    with pytest.raises(ValueError, match="is an LSTM\\(64\\) checkpoint, the table holds LSTM\\(128\\) policies"):
        _plan(network="lstm", nlstm=128, eval_opponents=[f["lstm64_ckpt"]])
    for bad in (dict(eval_trials=0), dict(eval_num_env=0), dict(eval_interval=-1), dict(eval_trials=2.5)):
        with pytest.raises(ValueError, match="%s must be an integer >= 1" % list(bad)[0]):
            _plan(**dict(ok, **bad))
    with pytest.raises(ValueError, match="refuses cfrc_mode 'rne_post'"):
        _plan(cfrc_mode="rne_post", **ok)
    with pytest.raises(ValueError, match="eval_opponents given with eval_interval=0"):
        _plan(eval_interval=0, **ok)
    with pytest.raises(ValueError, match="without eval_opponents"):
        _plan(eval_opponents=None)
    with pytest.raises(ValueError, match="is a list"):
        _plan(eval_opponents="00000")


def test_learn_refuses_before_touching_the_env():
    """learn() checks the evaluation first: the env below has dimensions and nothing else."""
    from robosumo_selfplay_amd import alg_ac, alg_ppo
    from robosumo_selfplay_amd.spaces import Box

    class DimsOnly(object):
        observation_space = [Box(-np.ones(ANT_OB), np.ones(ANT_OB))] * 2
        action_space = [Box(-np.ones(ANT_AC), np.ones(ANT_AC))] * 2
        cfrc_mode = "rne_post"
        num_envs = 4

    for learn in (alg_ppo.learn, alg_ac.learn):
        with pytest.raises(ValueError, match="refuses cfrc_mode 'rne_post'"):
            learn(network="mlp", env=DimsOnly(), total_timesteps=64, eval_interval=1, eval_opponents=["00000"])
        with pytest.raises(ValueError, match="eval_opponents given with eval_interval=0"):
            learn(network="mlp", env=DimsOnly(), total_timesteps=64, eval_opponents=["00000"])
    env = DimsOnly()
    with pytest.raises(ValueError, match="eval_env is the training env"):
        alg_ppo.learn(network="mlp", env=env, eval_env=env, total_timesteps=64, eval_interval=1, eval_opponents=["00000"])


def test_evaluation_schedule():
    from robosumo_selfplay_amd import train_eval
    plan = dict(interval=5)
    assert [u for u in range(1, 13) if train_eval.due(plan, u, 12)] == [1, 5, 10, 12]
    assert not any(train_eval.due(None, u, 12) for u in range(1, 13))


# ---- run.py --------------------------------------------------------------------------------------------------------------------
class _FakeEnv(object):
    agents = (0, 1)

    def close(self):
        self.closed = True


def _run_main(monkeypatch, tmp_path, argv):
    sys.path.insert(0, ROOT)
    import run
    from robosumo_selfplay_amd import alg_ac, alg_ppo, vec_env
    calls = []
    monkeypatch.setattr(vec_env, "make_vec_env", lambda *a, **k: _FakeEnv())
    monkeypatch.setattr(alg_ac, "learn", lambda **kw: calls.append(("ac", kw)) or "ac-model")
    monkeypatch.setattr(alg_ppo, "learn", lambda **kw: calls.append(("ppo", kw)) or "ppo-model")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    run.main(argv + ["--log_path", str(tmp_path)])
    return calls[0]


def test_run_forwards_the_new_flags(monkeypatch, tmp_path):
    algo, kw = _run_main(monkeypatch, tmp_path, ["--num_env", "8", "--num_timesteps", "80", "--eval_interval", "5", "--eval_opponent", "00000",
                                                 "--eval_opponent", "zoo/v1.npy", "--eval_trials", "32", "--eval_num_env", "16", "--eval_stochastic",
                                                 "--eval_cross_family", "--nsteps=16"])
    assert algo == "ppo" and kw["run_log"] is True and kw["eval_interval"] == 5 and kw["eval_opponents"] == ["00000", "zoo/v1.npy"]
    assert kw["eval_trials"] == 32 and kw["eval_num_env"] == 16 and kw["eval_deterministic"] is False and kw["eval_cross_family"] is True
    assert kw["nsteps"] == 16                                               # unknown --key=value forwarding as before
    algo, kw = _run_main(monkeypatch, tmp_path, ["--algo", "ac", "--num_env", "8", "--num_timesteps", "80", "--no_run_log", "--save_interval=7"])
    assert algo == "ac" and kw["run_log"] is False and not [k for k in kw if k.startswith("eval_")]
    # without the new flags: the keys tests/test_a2c_cpu.py checks, unchanged
    assert kw["nsteps"] == 5 and kw["lam"] == 0.95 and kw["save_interval"] == 7 and kw["nagent"] == 2 and kw["comm"] is None
    algo, kw = _run_main(monkeypatch, tmp_path, ["--num_env", "8", "--num_timesteps", "80"])
    assert algo == "ppo" and kw["run_log"] is True and not [k for k in kw if k.startswith("eval_")]


# ---- plot_run.py ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["train_reward", "eval_against_fix", "losses"])
def test_plot_run_writes_a_picture(tmp_path, kind):
    pytest.importorskip("matplotlib")
    pytest.importorskip("pandas")
    sys.path.insert(0, ROOT)
    import plot_run
    from robosumo_selfplay_amd import runlog
    runs = []
    for seed in range(2):
        d = str(tmp_path / ("run-%d" % seed))
        log = runlog.RunLog(d, "RoboSumo-Ant-vs-Ant-v0")
        entries = []
        for u in range(1, 5):
            e = dict(update=u, timesteps=256 * u, seconds=0.1, results=[dict(opponent="00000", win=0.1 * u + 0.05 * seed, draw=0.5, lose=0.5 - 0.1 * u),
                                                                      dict(opponent="zoo/v1.npy", win=0.05 * u, draw=0.9, lose=0.1 - 0.05 * u)])
            entries.append(e)
            log.row({"misc/total_timesteps": 256 * u, "misc/nupdates": u, "eprewmean": -3.0 + u + seed, "eplenmean": 40.0, "misc/explained_variance": 0.1 * u,
                     "loss/policy_loss": 0.01 * u, "loss/value_loss": 1.0 / u, "eval/0/win": e["results"][0]["win"]})
            log.evaluation(entries)
        runs.append(d)
    out = str(tmp_path / (kind + ".png"))
    assert plot_run.main(["--runs"] + runs + ["--type", kind, "--out", out]) == out
    with open(out, "rb") as f:
        data = f.read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and len(data) > 2000
    one = str(tmp_path / (kind + "-one.png"))
    plot_run.main(["--runs", runs[0], "--type", kind, "--out", one])
    assert os.path.getsize(one) > 2000
    x = [np.arange(3.0), np.arange(3.0)]
    assert len(plot_run.curves(x, [np.ones(3), 3 * np.ones(3)], ["a", "b"])) == 1 and plot_run.curves(x, [np.ones(3), 3 * np.ones(3)], "ab")[0][1][0] == 2.0
    assert len(plot_run.curves([np.arange(3.0), np.arange(4.0)], [np.ones(3), np.ones(4)], ["a", "b"])) == 2
