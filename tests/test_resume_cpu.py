"""CPU checks of resuming an interrupted ``learn()`` (robosumo_selfplay_amd/resume.py): what ``learn`` and run.py refuse before a
device or an env is touched, the fingerprint, the state file (version, truncation, atomic write), the capture / apply round trip on
stub objects, the declaration of the three snapshot exports and the run log's continuation."""
import csv
import json
import os
import re
from collections import deque

import numpy as np
import pytest

from robosumo_selfplay_amd import alg_ppo, capi, resume, runlog
from robosumo_selfplay_amd.spaces import Box, Tuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Env:
    """An env as ``learn`` looks at it before the first rollout; Ant-vs-Ant by default."""

    def __init__(self, obs_dims=(121, 121), act_dims=(8, 8), num_envs=32, snapshot=True):
        self.model = type("Model", (), {"obs_dims": tuple(obs_dims), "act_dims": tuple(act_dims)})()
        self.num_envs, self.device, self.groups = num_envs, "cuda:0", 1
        self.observation_space = Tuple([Box(-np.inf * np.ones(d), np.inf * np.ones(d)) for d in obs_dims])
        self.action_space = Tuple([Box(-np.ones(a), np.ones(a)) for a in act_dims])
        self.spec = type("Spec", (), {"id": "RoboSumo-Ant-vs-Ant-v0"})()
        if snapshot:
            self.snapshot = lambda: {}


class _NotALearner:
    def __init__(self, **kw):
        pytest.fail("the custom model_fn was called")


REFUSALS = [
    (dict(comm=object()), "comm"),
    (dict(opponent_pool=2), "opponent_pool > 1"),
    (dict(fused_selector=True), "fused_selector=True"),
    (dict(env=_Env((121, 165), (8, 12)), opponent_mode="fix", fix_opponent_path="unused.npy"), "mixed match-up"),
    (dict(model_fn=_NotALearner), "custom model_fn"),
    (dict(env=_Env(snapshot=False)), "SumoVecEnv"),
]


@pytest.mark.parametrize("how", [dict(resume=True), dict(resume_interval=2)], ids=["resume", "resume_interval"])
@pytest.mark.parametrize("kw,msg", REFUSALS, ids=[m.split()[0] for _, m in REFUSALS])
def test_learn_refusals_come_before_the_device(kw, msg, how, tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the device was asked for"))
    args = dict(network="mlp", env=_Env(), total_timesteps=1024, opponent_mode="ours", nsteps=8, log_dir=str(tmp_path), verbose=False)
    args.update(kw)
    args.update(how)
    with pytest.raises(NotImplementedError, match=re.escape(msg)) as e:
        alg_ppo.learn(**args)
    assert str(e.value).startswith("resume / resume_interval")
    assert os.listdir(str(tmp_path)) == []                              # nothing was written either


def test_every_refusal_has_its_own_message():
    assert len({m for _, m in REFUSALS}) == len(REFUSALS)
    msgs = []
    for kw, _ in REFUSALS:
        args = dict(env=_Env(), opponent_mode="ours")
        args.update({k: v for k, v in kw.items() if k in ("env", "comm", "opponent_pool", "fused_selector", "model_fn")})
        with pytest.raises(NotImplementedError) as e:
            resume.check_supported(**args)
        msgs.append(str(e.value))
    assert len(set(msgs)) == len(msgs)
    resume.check_supported(env=_Env(), opponent_mode="ours")             # the supported case passes
    # the model_fn rule is the class: a Learner subclass passes as it stands and behind functools.partial, a plain factory does not
    import functools
    from robosumo_selfplay_amd.model import PPOModel
    resume.check_supported(env=_Env(), opponent_mode="ours", model_fn=PPOModel)
    resume.check_supported(env=_Env(), opponent_mode="ours", model_fn=functools.partial(functools.partial(PPOModel, ent_coef=0.0), vf_coef=0.5))
    for fn in (lambda **kw: PPOModel(**kw), functools.partial(_NotALearner)):
        with pytest.raises(NotImplementedError, match="custom model_fn"):
            resume.check_supported(env=_Env(), opponent_mode="ours", model_fn=fn)


def test_negative_interval_is_refused(tmp_path):
    with pytest.raises(ValueError, match="resume_interval must be >= 0"):
        alg_ppo.learn(network="mlp", env=_Env(), total_timesteps=1024, nsteps=8, log_dir=str(tmp_path), resume_interval=-1)


RUN_REFUSALS = [
    (["--algo", "ac", "--resume"], "belong to --algo ppo"),
    (["--co_train", "--env", "RoboSumo-Ant-vs-Bug-v0", "--resume_interval", "2"], "not available with --co_train"),
    (["--env", "RoboSumo-Ant-vs-Bug-v0", "--resume"], "not available on a mixed match-up"),
    (["--resume_interval", "3"], "single GPU"),
]


@pytest.mark.parametrize("argv,msg", RUN_REFUSALS, ids=["ac", "co_train", "mixed", "world"])
def test_run_py_refusals_come_before_an_env_is_built(argv, msg, tmp_path, monkeypatch):
    import run
    from robosumo_selfplay_amd import vec_env
    monkeypatch.setattr(vec_env, "make_vec_env", lambda *a, **k: pytest.fail("an env was built"))
    monkeypatch.setattr(vec_env, "SumoVecEnv", lambda *a, **k: pytest.fail("an env was built"))
    if msg == "single GPU":
        monkeypatch.setenv("WORLD_SIZE", "2")
        monkeypatch.setenv("RANK", "0")
    with pytest.raises(SystemExit, match=msg):
        run.main(argv + ["--log_path", str(tmp_path)])
    assert os.listdir(str(tmp_path)) == []
    assert len({m for _, m in RUN_REFUSALS}) == len(RUN_REFUSALS)


def test_run_py_flags_reach_learn():
    import run
    args = run.build_parser().parse_args(["--resume_interval", "5", "--resume"])
    assert args.resume_interval == 5 and args.resume is True
    d = run.build_parser().parse_args([])
    assert d.resume_interval == 0 and d.resume is False
    run.check_resume(d, 8)                                               # off: nothing is refused


# ---- fingerprint and file ----------------------------------------------------------------------------------------------------
def _fp(**kw):
    args = dict(env=_Env(), nsteps=8, total_timesteps=1024, network="mlp", network_kwargs=dict(num_hidden=64, activation="relu"),
                opponent_mode="ours", use_opponent_data=None, seed=3, nminibatches=4, noptepochs=2, lr=lambda f: 1e-3 * f,
                cliprange=lambda f: 0.2, fix_opponent_path=None)
    args.update(kw)
    return resume.fingerprint(**args)


def test_fingerprint_names_the_first_differing_key_with_both_values():
    a = _fp()
    assert list(a)[0] == "format_version" and a["lr"] == [1e-3, 0.0] and a["cliprange"] == [0.2, 0.2]
    assert a["env_id"] == "RoboSumo-Ant-vs-Ant-v0" and a["num_envs"] == 32 and a["groups"] == 1
    resume.check_fingerprint(dict(a), _fp())
    with pytest.raises(resume.ResumeError, match=r"nsteps=8; this call has nsteps=16"):
        resume.check_fingerprint(dict(a), _fp(nsteps=16, noptepochs=7))          # two differ: the first in the fingerprint's order is named
    with pytest.raises(resume.ResumeError, match=r"noptepochs=2; this call has noptepochs=7"):
        resume.check_fingerprint(dict(a), _fp(noptepochs=7))
    with pytest.raises(resume.ResumeError, match=r"lr=\[0\.001, 0\.0\]; this call has lr=\[0\.001, 0\.001\]"):
        resume.check_fingerprint(dict(a), _fp(lr=lambda f: 1e-3))
    with pytest.raises(resume.ResumeError, match=r"network_kwargs=.*'num_hidden': 64.*'num_hidden': 32"):
        resume.check_fingerprint(dict(a), _fp(network_kwargs=dict(num_hidden=32, activation="relu")))
    with pytest.raises(resume.ResumeError, match=r"fix_opponent_path=None; this call has fix_opponent_path=\['a.npy', 'b.npy'\]"):
        resume.check_fingerprint(dict(a), _fp(fix_opponent_path=("a.npy", "b.npy")))
    with pytest.raises(resume.ResumeError, match="format version 99"):
        resume.check_fingerprint(dict(a, format_version=99), _fp())


def _state(update=2, **kw):
    return resume.capture(fingerprint=_fp(), update=update, **kw)


def test_state_file_round_trip_unknown_version_and_truncation(tmp_path):
    d = str(tmp_path)
    assert resume.read_state(d) is None                                  # no file: None, the caller starts from update 1
    path, size = resume.write_state(d, _state(history=dict(lossvals=[np.arange(5.0)], version_gap=[0, 1])))
    assert path == os.path.join(d, "resume", "state.pt") == resume.state_path(d) and size == os.path.getsize(path)
    assert not os.path.exists(path + ".tmp")
    st = resume.read_state(d)
    assert list(st)[0] == "fingerprint" and st["update"] == 2 and st["history"]["version_gap"] == [0, 1]
    assert np.array_equal(st["history"]["lossvals"][0], np.arange(5.0))
    # an unknown version is refused by name
    bad = _state()
    bad["fingerprint"]["format_version"] = resume.FORMAT_VERSION + 1
    resume.write_state(d, bad)
    with pytest.raises(resume.ResumeError, match=r"state\.pt has format version %d; this code reads version %d" % (resume.FORMAT_VERSION + 1,
                                                                                                                 resume.FORMAT_VERSION)):
        resume.read_state(d)
    # so is a truncated file, and a file that is something else
    resume.write_state(d, _state())
    raw = open(path, "rb").read()
    with open(path, "wb") as f:
        f.write(raw[:len(raw) // 2])
    with pytest.raises(resume.ResumeError, match=r"state\.pt does not load"):
        resume.read_state(d)
    import torch
    torch.save([1, 2, 3], path)
    with pytest.raises(resume.ResumeError, match=r"state\.pt holds no fingerprint"):
        resume.read_state(d)


def test_learn_refuses_a_state_that_does_not_load_and_other_arguments(tmp_path, monkeypatch):
    """``learn(resume=True)`` meets the file before it builds a model: never silently ignored."""
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the device was asked for"))
    d = str(tmp_path)
    args = dict(network="mlp", env=_Env(), total_timesteps=1024, opponent_mode="ours", nsteps=8, log_dir=d, verbose=False, seed=3,
                nminibatches=4, noptepochs=2, lr=1e-3, num_hidden=64, activation="relu", resume=True)
    fp = _fp(lr=lambda f: 1e-3, network_kwargs=dict(num_hidden=64, activation="relu"))
    resume.write_state(d, resume.capture(fingerprint=fp, update=1))
    with pytest.raises(resume.ResumeError, match=r"nsteps=8; this call has nsteps=16"):
        alg_ppo.learn(**dict(args, nsteps=16))
    with pytest.raises(resume.ResumeError, match=r"seed=3; this call has seed=4"):
        alg_ppo.learn(**dict(args, seed=4))
    with open(resume.state_path(d), "wb") as f:
        f.write(b"not a state")
    with pytest.raises(resume.ResumeError, match=r"state\.pt does not load"):
        alg_ppo.learn(**args)


def test_write_is_atomic(tmp_path, monkeypatch):
    d = str(tmp_path)
    resume.write_state(d, _state(update=2))
    monkeypatch.setattr(os, "replace", lambda *a: (_ for _ in ()).throw(OSError("killed before the rename")))
    with pytest.raises(OSError, match="killed before the rename"):
        resume.write_state(d, _state(update=3))
    monkeypatch.undo()
    assert resume.read_state(d)["update"] == 2                            # the old state still loads
    with open(resume.state_path(d) + ".tmp", "wb") as f:                  # nor does half a temporary file disturb it
        f.write(b"half")
    assert resume.read_state(d)["update"] == 2
    resume.write_state(d, _state(update=4))
    assert resume.read_state(d)["update"] == 4


# ---- capture / apply on stub objects -------------------------------------------------------------------------------------------
class _StubPolicy:
    def __init__(self, seed):
        import torch
        self.gen = torch.Generator()
        self.gen.manual_seed(seed)


class _StubModel:
    def __init__(self, seed, trainable):
        import torch
        self.params = torch.arange(6, dtype=torch.float32) + seed
        self.act_model = _StubPolicy(seed)
        self.trainable = trainable
        if trainable:
            self.m, self.v, self.t = torch.full((6,), 0.5), torch.full((6,), 0.25), 7


class _StubRunner:
    def __init__(self):
        import torch
        self.models = [_StubModel(1, True), _StubModel(2, False)]
        self.env = object()
        self.device = torch.device("cpu")
        self.dones = torch.tensor([[0, 1], [1, 0]], dtype=torch.uint8)
        self.states = [torch.ones(2, 4), None]
        self.shadow_state, self.shadow_state0, self.zoo_state = torch.full((2, 4), 3.0), None, torch.zeros(2, 128)
        self.league_scores = None


def _draws(runner, shuffle_gen):
    import torch
    return ([np.random.rand(3).tolist(), np.random.choice(10, 4).tolist(), torch.rand(3).tolist(), torch.randperm(9, generator=shuffle_gen).tolist()]
            + [torch.randn(4, generator=m.act_model.gen).tolist() for m in runner.models])


def test_capture_apply_round_trip_on_stubs():
    import torch
    np.random.seed(11)
    torch.manual_seed(12)
    runner, gen = _StubRunner(), torch.Generator()
    gen.manual_seed(13)
    _draws(runner, gen)                                                  # somewhere in the streams
    epinfobuf = deque([{"r": 1.5, "l": 20, "t": 0.0}, {"r": -2.0, "l": 7, "t": 0.0}], maxlen=100)
    history = dict(version_gap=[0, 1], lossvals=[np.array([1.0, 2.0])], early_stop_info=[None, [1, 2]])
    od = (torch.arange(12.0).reshape(4, 3), torch.ones(4, 2))
    st = resume.capture(fingerprint=_fp(), update=5, runner=runner, shuffle_gen=gen, opponent_data=od, epinfobuf=epinfobuf, history=history,
                        time_elapsed=12.5, run_log=dict(keys=["a"], rows=[{"a": 1}], monitor_rows=2, t_start=0.0))
    after_capture = _draws(runner, gen)
    # the run goes on and changes everything the state was taken of
    runner.models[0].params.add_(1.0); runner.models[0].m.zero_(); runner.models[0].t = 99
    runner.models[1].params.zero_()
    runner.dones.zero_(); runner.states[0].zero_(); runner.shadow_state.zero_(); runner.zoo_state.fill_(5.0)
    epinfobuf.append({"r": 0.0, "l": 1, "t": 0.0}); history["version_gap"].append(2); od[0].zero_()
    _draws(runner, gen)
    assert torch.equal(st["models"][0]["params"], torch.arange(6, dtype=torch.float32) + 1)      # the state aliased none of it
    # ... through a file, into the objects a fresh set-up built
    fresh, gen2, buf2, hist2 = _StubRunner(), torch.Generator(), deque(maxlen=100), dict(version_gap=[], eval=[])
    fresh.models[0].params.zero_(); fresh.models[0].t = 0
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        resume.write_state(d, st)
        st2 = resume.read_state(d)
    update, od2 = resume.apply(st2, runner=fresh, shuffle_gen=gen2, epinfobuf=buf2, history=hist2, device=None)
    assert update == 5 and torch.equal(od2[0], torch.arange(12.0).reshape(4, 3)) and torch.equal(od2[1], torch.ones(4, 2))
    assert _draws(fresh, gen2) == after_capture                          # every stream continues where the capture left it
    m0, m1 = fresh.models
    assert torch.equal(m0.params, torch.arange(6, dtype=torch.float32) + 1) and torch.equal(m1.params, torch.arange(6, dtype=torch.float32) + 2)
    assert torch.equal(m0.m, torch.full((6,), 0.5)) and torch.equal(m0.v, torch.full((6,), 0.25)) and m0.t == 7
    assert torch.equal(fresh.dones, torch.tensor([[0, 1], [1, 0]], dtype=torch.uint8))
    assert torch.equal(fresh.states[0], torch.ones(2, 4)) and fresh.states[1] is None
    assert torch.equal(fresh.shadow_state, torch.full((2, 4), 3.0)) and torch.equal(fresh.zoo_state, torch.zeros(2, 128))
    assert list(buf2) == [{"r": 1.5, "l": 20, "t": 0.0}, {"r": -2.0, "l": 7, "t": 0.0}] and buf2.maxlen == 100
    assert hist2["version_gap"] == [0, 1] and hist2["early_stop_info"] == [None, [1, 2]] and "eval" not in hist2
    assert np.array_equal(hist2["lossvals"][0], np.array([1.0, 2.0]))
    assert st2["time_elapsed"] == 12.5 and st2["run_log"]["monitor_rows"] == 2


def test_later_checkpoints_are_dropped(tmp_path):
    d = str(tmp_path)
    for name in ("00000", "00001", "00002", "00003", "00004", "notes.txt"):
        open(os.path.join(d, name), "w").close()
    assert resume.drop_later_checkpoints(d, 2) == ["00003", "00004"]
    assert sorted(os.listdir(d)) == ["00000", "00001", "00002", "notes.txt"]
    assert resume.drop_later_checkpoints(os.path.join(d, "missing"), 2) == []


# ---- the exports ---------------------------------------------------------------------------------------------------------------
def test_snapshot_exports_are_declared_bound_and_exported():
    """The three exports are declared in include/sumo_hip.h, named in capi's table of them and exported by the built library.
    (``capi.EXPORTS`` itself is the tuple tests/test_match_pairing_cpu.py pins entry by entry: the snapshot exports have a table of
    their own, as the co-training launch has.)"""
    import ctypes
    from robosumo_selfplay_amd import build
    header = open(os.path.join(ROOT, "include", "sumo_hip.h")).read()
    assert capi.SNAPSHOT_EXPORTS == ("sumo_snapshot_bytes", "sumo_snapshot_save", "sumo_snapshot_load")
    assert "size_t sumo_snapshot_bytes(sumo_handle_t h);" in header
    assert "int sumo_snapshot_save(sumo_handle_t h, void* dst_host, size_t bytes);" in header
    assert "int sumo_snapshot_load(sumo_handle_t h, const void* src_host, size_t bytes);" in header
    assert "#define SUMO_SNAPSHOT_HEADER_BYTES %d" % capi.SNAPSHOT_HEADER_BYTES in header
    build.build_all()
    L = ctypes.CDLL(build.lib_path("libsumo_hip.so"))
    for n in capi.SNAPSHOT_EXPORTS:
        assert hasattr(L, n), n
    assert callable(capi.Engine.snapshot) and callable(capi.Engine.restore)
    # a NULL handle is refused by each of them without a device
    L.sumo_snapshot_bytes.restype = ctypes.c_size_t
    L.sumo_last_error.restype = ctypes.c_char_p
    assert L.sumo_snapshot_bytes(None) == 0
    buf = ctypes.create_string_buffer(64)
    assert L.sumo_snapshot_save(None, buf, ctypes.c_size_t(64)) == -1 and b"NULL" in L.sumo_last_error()
    assert L.sumo_snapshot_load(None, buf, ctypes.c_size_t(64)) == -1 and b"NULL" in L.sumo_last_error()


# ---- the run log ---------------------------------------------------------------------------------------------------------------
def _row(update, **kw):
    return dict({"misc/nupdates": update, "misc/total_timesteps": update * 256, "eprewmean": 0.5 * update, "fps": 1000.0 + update}, **kw)


def _progress(d):
    with open(os.path.join(d, "progress.csv")) as f:
        return list(csv.DictReader(f))


def test_run_log_is_cut_to_the_saved_update_and_continued(tmp_path):
    """Files that hold rows to update 5 are cut to update 3 -- the state's -- and update 4 is appended once."""
    d = str(tmp_path)
    log = runlog.RunLog(d, "RoboSumo-Ant-vs-Ant-v0", header=dict(eval_opponents=[]))
    history, states, files_at = dict(version_gap=[], lossvals=[]), {}, {}
    for u in range(1, 6):
        history["version_gap"].append(u - 1); history["lossvals"].append(np.array([float(u), 2.0]))
        log.episodes([{"r": float(u), "l": 10 + u, "t": 0.0}] * u)
        log.row(_row(u, **({"eval/0/win": 0.25} if u == 2 else {})))       # a key that appears late rewrites the table
        log.history(history, loss_names=["a", "b"])
        states[u] = (log.state(), json.loads(json.dumps(runlog.to_jsonable(history))))
        files_at[u] = {n: open(os.path.join(d, n)).read() for n in ("log.txt", "progress.csv", runlog.MONITOR_FILE, "history.json")}
    assert [int(r["misc/nupdates"]) for r in _progress(d)] == [1, 2, 3, 4, 5]
    st, hist3 = states[3]
    assert st["monitor_rows"] == 6 and len(st["rows"]) == 3
    # the killed process left updates 4 and 5 behind; the resumed one continues from the state of update 3
    cont = runlog.RunLog(d, "RoboSumo-Ant-vs-Ant-v0", header=dict(eval_opponents=[]), resume=st)
    cont.history(hist3, loss_names=["a", "b"])
    now = {n: open(os.path.join(d, n)).read() for n in files_at[3]}
    assert now == files_at[3]                                            # byte for byte what update 3 left, the monitor's header included
    assert cont.t_start == log.t_start and cont.keys == st["keys"]
    hist3["version_gap"].append(3); hist3["lossvals"].append([4.0, 2.0])
    cont.episodes([{"r": 4.0, "l": 14, "t": 0.0}] * 4)
    cont.row(_row(4))
    cont.history(hist3, loss_names=["a", "b"])
    rows = _progress(d)
    assert [int(r["misc/nupdates"]) for r in rows] == [1, 2, 3, 4]      # no update twice, none lost
    assert rows[1]["eval/0/win"] == "0.25" and rows[3]["eval/0/win"] == "" and float(rows[3]["eprewmean"]) == 2.0
    assert open(os.path.join(d, "progress.csv")).read() == files_at[4]["progress.csv"]
    assert open(os.path.join(d, "log.txt")).read() == files_at[4]["log.txt"]
    assert json.load(open(os.path.join(d, "history.json")))["version_gap"] == [0, 1, 2, 3]
    mon = open(os.path.join(d, runlog.MONITOR_FILE)).read().splitlines()
    assert mon[:2] == files_at[5][runlog.MONITOR_FILE].splitlines()[:2] and len(mon) == 2 + 10
    assert [ln.split(",")[1] for ln in mon[2:]] == ["11"] + ["12"] * 2 + ["13"] * 3 + ["14"] * 4
    assert cont.state()["monitor_rows"] == 10
    # a monitor file that holds fewer episodes than the state is not continued quietly
    with open(os.path.join(d, runlog.MONITOR_FILE), "w") as f:
        f.write("\n".join(mon[:4]) + "\n")
    with pytest.raises(ValueError, match="holds 2 episodes, the saved state 6"):
        runlog.RunLog(d, "RoboSumo-Ant-vs-Ant-v0", resume=st)
