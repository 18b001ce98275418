"""Continue an interrupted ``alg_ppo.learn`` bit for bit.

``learn(resume_interval=k)`` writes, after every k-th update, everything its loop carries from one update to the next into
``log_dir/resume/state.pt``; ``learn(resume=True)`` builds the same objects as always, lets :func:`apply` overwrite what set-up drew and
continues at the saved update + 1.  Training U updates in one go, or training some, being killed and resuming, leaves the same
checkpoints, ``history`` and run-log rows.

The file is one ``torch.save`` of a dict whose first entry is the run's :func:`fingerprint`; it is written to ``state.pt.tmp``,
fsynced and ``os.replace``d, so a kill in mid-write leaves the previous state.  What is in it (:func:`capture`): the update number;
per model of the Runner its parameters, Adam moments and step count, its noise generator and (policy-zoo nets) its own recurrent rows;
the minibatch shuffle generator; numpy's global state and torch's CPU and device generator states; the Runner's carried tensors; the
previous rollout's agent-1 rows where the next update's selector scores them (``opponent_mode='ours'``); ``epinfobuf``; ``history``;
the run log's rows; the env snapshot (``SumoVecEnv.snapshot``).  Everything is moved to the host.  Plain Python and torch: the
functions here run without a GPU on objects that hold CPU tensors (tests/test_resume_cpu.py).
"""
import functools
import os
from collections import OrderedDict

import numpy as np

FORMAT_VERSION = 1
STATE_DIR, STATE_FILE = "resume", "state.pt"


class ResumeError(RuntimeError):
    pass


def state_path(log_dir):
    return os.path.join(str(log_dir), STATE_DIR, STATE_FILE)


# ---- what resuming refuses ---------------------------------------------------------------------------------------------------
def check_supported(*, env, opponent_mode, comm=None, opponent_pool=1, fused_selector=False, model_fn=None):
    """What ``learn(resume_interval=..., resume=...)`` refuses, before anything touches the device: each with its own message, naming
    the argument."""
    from . import mixed
    from .learner import Learner
    if comm is not None:
        raise NotImplementedError("resume / resume_interval: single GPU only -- comm (a torch.distributed group) is not supported; every "
                                  "rank would have to write and restore its own env shard")
    if int(opponent_pool) > 1:
        raise NotImplementedError("resume / resume_interval: opponent_pool > 1 is not supported (the pool's resident snapshots and its "
                                  "tile assignment are not part of the saved state)")
    if fused_selector:
        raise NotImplementedError("resume / resume_interval: fused_selector=True is not supported (the selector's device table of "
                                  "checkpoints is not part of the saved state)")
    if mixed.is_mixed(env):
        raise NotImplementedError("resume / resume_interval: a mixed match-up (env %s, trained through mixed.MixedRunner) is not supported"
                                  % getattr(getattr(env, "spec", None), "id", "?"))
    # the params / Adam attributes cannot be read off a model_fn before it is called, and nothing may be built before this refusal: the
    # rule is the class -- a learner.Learner subclass, as it stands or behind functools.partial
    cls = model_fn
    while isinstance(cls, functools.partial):
        cls = cls.func
    if model_fn is not None and not (isinstance(cls, type) and issubclass(cls, Learner)):
        raise NotImplementedError("resume / resume_interval: a custom model_fn must be a learner.Learner subclass (or a functools.partial "
                                  "of one): its flat ``params`` and Adam ``m`` / ``v`` / ``t`` are what is saved and restored")
    if not hasattr(env, "snapshot"):
        raise NotImplementedError("resume / resume_interval: env must be a SumoVecEnv (the env state is saved by SumoVecEnv.snapshot)")


# ---- fingerprint -------------------------------------------------------------------------------------------------------------
def _plain(x):
    """A fingerprint value as plain Python: numbers, strings, None, lists of them."""
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    if isinstance(x, dict):
        return {str(k): _plain(v) for k, v in sorted(x.items())}
    if isinstance(x, (np.integer,)):
        return int(x)
    if isinstance(x, (np.floating,)):
        return float(x)
    if x is None or isinstance(x, (str, bool, int, float)):
        return x
    return repr(x)


def fingerprint(*, env, nsteps, total_timesteps, network, network_kwargs, opponent_mode, use_opponent_data, seed, nminibatches, noptepochs,
                lr, cliprange, fix_opponent_path):
    """What a resumed run must share with the run that wrote the state, in the order it is compared.  ``lr`` / ``cliprange``: the
    schedules as ``learn`` calls them (functions of the remaining fraction); their values at 1 and 0 stand for them."""
    fp = OrderedDict()
    fp["format_version"] = FORMAT_VERSION
    fp["env_id"] = getattr(getattr(env, "spec", None), "id", None)
    fp["num_envs"] = int(env.num_envs)
    fp["groups"] = int(getattr(env, "groups", 1))
    fp["nsteps"] = int(nsteps)
    fp["total_timesteps"] = int(total_timesteps)
    fp["network"] = network if isinstance(network, str) else repr(network)
    fp["network_kwargs"] = _plain(dict(network_kwargs))
    fp["opponent_mode"] = opponent_mode
    fp["use_opponent_data"] = use_opponent_data
    fp["seed"] = seed
    fp["nminibatches"] = int(nminibatches)
    fp["noptepochs"] = int(noptepochs)
    fp["lr"] = [float(lr(1.0)), float(lr(0.0))]
    fp["cliprange"] = [float(cliprange(1.0)), float(cliprange(0.0))]
    fp["fix_opponent_path"] = _plain(fix_opponent_path)
    return fp


def check_fingerprint(saved, now, path="the resume state"):
    """Refuse a resume whose arguments differ from the saved run's: the first differing key, with both values."""
    if saved.get("format_version") != now["format_version"]:
        raise ResumeError("%s has format version %r; this code reads version %r" % (path, saved.get("format_version"), now["format_version"]))
    for k, v in now.items():
        if k not in saved:
            raise ResumeError("%s: the saved fingerprint has no %r (now %r)" % (path, k, v))
        if saved[k] != v:
            raise ResumeError("%s was written by a run with %s=%r; this call has %s=%r: resume with the arguments of the interrupted run"
                              % (path, k, saved[k], k, v))


# ---- the file ------------------------------------------------------------------------------------------------------------------
def write_state(log_dir, state):
    """``state`` to ``log_dir/resume/state.pt``: written next to it, fsynced, then renamed over it.  Returns (path, bytes)."""
    import torch
    path = state_path(log_dir)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        torch.save(state, f)
        f.flush()
        os.fsync(f.fileno())
    size = os.path.getsize(tmp)
    os.replace(tmp, path)
    return path, size


def read_state(log_dir):
    """The state of ``log_dir`` or None where there is no state file.  A file that does not load, or of another format version, is
    refused by name."""
    import torch
    path = state_path(log_dir)
    if not os.path.exists(path):
        return None
    try:
        state = torch.load(path, map_location="cpu", weights_only=False)
    except Exception as e:
        raise ResumeError("resume state %s does not load (%s: %s): delete it to start from update 1" % (path, type(e).__name__, e))
    fp = state.get("fingerprint") if isinstance(state, dict) else None
    if not isinstance(fp, dict) or "format_version" not in fp:
        raise ResumeError("resume state %s holds no fingerprint: not a state file of this project" % path)
    if fp["format_version"] != FORMAT_VERSION:
        raise ResumeError("resume state %s has format version %r; this code reads version %r" % (path, fp["format_version"], FORMAT_VERSION))
    return state


# ---- capture / apply -----------------------------------------------------------------------------------------------------------
def _host(x):
    """``x`` with every tensor in it as a host copy of its own (the saved state must not alias buffers the run goes on writing)."""
    import torch
    if torch.is_tensor(x):
        return x.detach().to("cpu", copy=True).contiguous()
    if isinstance(x, np.ndarray):
        return x.copy()
    if isinstance(x, dict):
        return {k: _host(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_host(v) for v in x)
    return x


def _put(dst, src):
    """``src`` (host) into the tensor ``dst`` in place; shapes must agree."""
    if tuple(dst.shape) != tuple(src.shape) or dst.dtype != src.dtype:
        raise ResumeError("saved tensor %s %s does not fit %s %s" % (tuple(src.shape), src.dtype, tuple(dst.shape), dst.dtype))
    dst.copy_(src)


def _gen_of(m):
    am = getattr(m, "act_model", None)
    return getattr(am, "gen", None) if am is not None else getattr(m, "gen", None)


def model_state(m):
    """One model of the Runner: flat parameters; Adam moments and step count of a trainable one; its noise generator; a policy-zoo
    net's (or league's) own recurrent rows."""
    import torch
    s = {}
    if torch.is_tensor(getattr(m, "params", None)):
        s["params"] = _host(m.params)
    if getattr(m, "trainable", False) and torch.is_tensor(getattr(m, "m", None)):
        s.update(m=_host(m.m), v=_host(m.v), t=int(m.t))
    gen = _gen_of(m)
    if gen is not None:
        s["gen"] = gen.get_state().clone()
    rows = getattr(getattr(m, "act_model", None), "state", None)
    if torch.is_tensor(rows) and not torch.is_tensor(getattr(m, "params", None)):
        s["zoo_rows"] = _host(rows)
    return s


def apply_model_state(m, s):
    if "params" in s:
        _put(m.params, s["params"])
    if "m" in s:
        _put(m.m, s["m"]); _put(m.v, s["v"])
        m.t = int(s["t"])
    if "gen" in s:
        _gen_of(m).set_state(s["gen"])
    if "zoo_rows" in s:
        zoo = m.act_model
        if getattr(zoo, "state", None) is None or tuple(zoo.state.shape) != tuple(s["zoo_rows"].shape):
            zoo.state = s["zoo_rows"].to(zoo.device)
        else:
            zoo.state.copy_(s["zoo_rows"])


RUNNER_TENSORS = ("shadow_state", "shadow_state0", "zoo_state")


def runner_state(runner):
    """What a device-mode Runner carries between two ``run`` calls besides the env's own buffers (its ``obs`` / ``dones`` ARE the
    env's after the first rollout): the done flags, the recurrent states, the shadow state, the zoo LSTM rows, the league tally."""
    import torch
    s = dict(dones=_host(runner.dones), dones_are_env=getattr(runner.env, "done_dev", None) is runner.dones,
             states=[_host(x) if torch.is_tensor(x) else (None if x is None else np.array(x, copy=True)) for x in runner.states])
    for k in RUNNER_TENSORS:
        v = getattr(runner, k, None)
        s[k] = _host(v) if torch.is_tensor(v) else None
    sc = getattr(runner, "league_scores", None)
    s["league_scores"] = None if sc is None else np.array(sc, copy=True)
    return s


def apply_runner_state(runner, s):
    import torch
    env = runner.env
    if hasattr(env, "obs_dev"):
        runner.obs = env.obs_dev
    if s["dones_are_env"]:
        runner.dones = env.done_dev
    elif torch.is_tensor(runner.dones):
        _put(runner.dones, s["dones"])
    else:
        runner.dones = np.array(s["dones"])
    for i, x in enumerate(s["states"]):
        if torch.is_tensor(x) and torch.is_tensor(runner.states[i]):
            _put(runner.states[i], x)
        else:
            runner.states[i] = x
    for k in RUNNER_TENSORS:
        v = s.get(k)
        if v is None:
            continue
        cur = getattr(runner, k, None)
        if torch.is_tensor(cur) and tuple(cur.shape) == tuple(v.shape):
            cur.copy_(v)
        else:
            setattr(runner, k, v.to(runner.device))
    runner.league_scores = s.get("league_scores")


def rng_state(device=None):
    """numpy's global state, torch's CPU generator and (``device``) that device's default generator."""
    import torch
    s = dict(numpy=np.random.get_state(), torch_cpu=torch.get_rng_state().clone())
    if device is not None:
        s["torch_device"] = torch.cuda.get_rng_state(device).clone()
    return s


def apply_rng_state(s, device=None):
    import torch
    np.random.set_state(s["numpy"])
    torch.set_rng_state(s["torch_cpu"])
    if device is not None and "torch_device" in s:
        torch.cuda.set_rng_state(s["torch_device"], device)


def capture(*, fingerprint, update, runner=None, env=None, shuffle_gen=None, opponent_data=None, epinfobuf=(), history=None,
            time_elapsed=0.0, run_log=None, device=None):
    """The state after ``update``, on the host.  Every part is optional so that the pieces can be exercised on their own; ``learn``
    passes all of them.  ``opponent_data``: the (obs, actions) rows of agent 1 that the next update's selector scores, or None."""
    state = OrderedDict(fingerprint=dict(fingerprint))
    state["update"] = int(update)
    state["rng"] = rng_state(device)
    state["models"] = [model_state(m) for m in runner.models] if runner is not None else []
    state["runner"] = runner_state(runner) if runner is not None else None
    state["shuffle_gen"] = None if shuffle_gen is None else shuffle_gen.get_state().clone()
    state["opponent_data"] = None if opponent_data is None else tuple(_host(x) for x in opponent_data)
    state["epinfobuf"] = [dict(e) for e in epinfobuf]
    state["history"] = _host(dict(history)) if history is not None else None
    state["time_elapsed"] = float(time_elapsed)
    state["run_log"] = run_log
    state["env"] = _host(env.snapshot()) if env is not None else None
    return state


def apply(state, *, runner=None, env=None, shuffle_gen=None, epinfobuf=None, history=None, device=None):
    """Overwrite what set-up built with ``state``: the env first (the Runner's ``obs`` / ``dones`` are its buffers), then the models, the
    Runner, the generators, ``epinfobuf`` and ``history`` (both in place: the loop's other objects hold them), and the global random
    streams last, so that nothing done here draws from them afterwards.  Returns (update, opponent_data on ``device`` or None)."""
    import torch
    if env is not None:
        env.restore(state["env"])
    if runner is not None:
        if len(state["models"]) != len(runner.models):
            raise ResumeError("the saved state holds %d models, the Runner %d" % (len(state["models"]), len(runner.models)))
        league = getattr(runner.models[-1], "act_model", None)
        if hasattr(league, "assign") and hasattr(league, "tile_member"):      # a league: the deal of the saved update, then its rows
            league.assign(state["update"] - 1)
        for m, s in zip(runner.models, state["models"]):
            apply_model_state(m, s)
        apply_runner_state(runner, state["runner"])
    if shuffle_gen is not None and state["shuffle_gen"] is not None:
        shuffle_gen.set_state(state["shuffle_gen"])
    if epinfobuf is not None:
        epinfobuf.clear()
        epinfobuf.extend(state["epinfobuf"])
    if history is not None and state["history"] is not None:
        history.clear()
        history.update(state["history"])
    od = state["opponent_data"]
    if od is not None and device is not None:
        od = tuple(x.to(device) for x in od)
    apply_rng_state(state["rng"], device)
    return state["update"], od


def drop_later_checkpoints(checkdir, update):
    """Checkpoints of updates after ``update``, left by the interrupted process: removed, so that the selection of the next update lists
    the files the uninterrupted run listed (they are written again, identically).  Returns the names removed."""
    gone = []
    if os.path.isdir(checkdir):
        for name in sorted(os.listdir(checkdir)):
            if name.isdigit() and int(name) > int(update):
                os.remove(os.path.join(checkdir, name))
                gone.append(name)
    return gone
