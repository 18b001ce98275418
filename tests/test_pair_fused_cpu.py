"""CPU checks of the co-training rollout in the engine's fused launch (``sumo_rollout_steps_pair``): the ctypes
mirrors of its two structs against the C compiler's layout, its place in the binding, ``run.py --co_train --fused_rollout``, and what
``co_train.learn`` / ``PairRunner`` refuse before they touch the device."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from robosumo_selfplay_amd import build, capi, co_train
from test_co_train_cpu import _Env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STRUCTS = [("sumo_pair_side", capi.PairSideRollout), ("sumo_rollout_pair", capi.RolloutPair)]


def test_ctypes_mirrors_match_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sumo_hip.h"', 'int main(void) {']
    for cname, st in STRUCTS:
        lines.append('  printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in st._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    table = {}
    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        a, b, v = ln.split()
        table[(a, b)] = int(v)
    for cname, st in STRUCTS:
        assert C.sizeof(st) == table[(cname, "size")], cname
        for fname, _ in st._fields_:
            assert getattr(st, fname).offset == table[(cname, fname)], (cname, fname)
        last = st._fields_[-1][0]                   # both structs end in a pointer: every field of the header is mirrored
        assert getattr(st, last).offset + getattr(st, last).size == table[(cname, "size")], cname
    assert C.sizeof(capi.RolloutPair) == 2 * C.sizeof(capi.PairSideRollout) + 64
    assert capi.RolloutPair.side.offset == 0 and capi.RolloutPair.side.size == 2 * C.sizeof(capi.PairSideRollout)


def test_the_entry_is_bound_beside_the_pinned_tables():
    assert "sumo_rollout_steps_pair" not in capi.FUSED_ENTRIES and "sumo_rollout_steps_pair" not in capi.EXPORTS
    assert len(capi.FUSED_ENTRIES) == 16 and capi.EXPORTS[6:22] == tuple(capi.FUSED_ENTRIES)
    assert capi.PAIR_ENTRIES == {"sumo_rollout_steps_pair": (capi.RolloutPair, None)}
    build.build_all()
    L = capi.lib()
    fn = L.sumo_rollout_steps_pair
    assert fn.restype is C.c_int and len(fn.argtypes) == 10 and fn.argtypes[1] is C.POINTER(capi.RolloutPair)
    assert callable(capi.Engine.rollout_steps_pair)
    from robosumo_selfplay_amd.vec_env import SumoVecEnv
    assert callable(SumoVecEnv.rollout_steps_pair_group)
    header = open(os.path.join(ROOT, "include", "sumo_hip.h")).read()
    assert "int sumo_rollout_steps_pair(sumo_handle_t h, const sumo_rollout_pair* r" in header


class _Reached(Exception):
    pass


def test_run_py_passes_fused_rollout_to_learn(tmp_path, monkeypatch):
    import run
    from robosumo_selfplay_amd import vec_env
    seen = {}

    class Env(_Env):
        def close(self):
            seen["closed"] = True

    def make(env_id, num_env, seed, **kw):
        seen["env"] = dict(kw, env_id=env_id, num_env=num_env)
        e = Env(num_envs=num_env)
        e.spec.id = env_id
        return e

    def learn(**kw):
        seen["learn"] = kw
        raise _Reached()

    monkeypatch.setattr(vec_env, "make_vec_env", make)
    monkeypatch.setattr(co_train, "learn", learn)
    monkeypatch.setenv("WORLD_SIZE", "1")
    argv = ["--co_train", "--env", "RoboSumo-Ant-vs-Bug-v0", "--num_env", "64", "--log_path", str(tmp_path), "--nsteps=8", "--nminibatches=2"]
    with pytest.raises(_Reached):
        run.main(argv + ["--fused_rollout"])
    assert seen["learn"]["fused_rollout"] is True and seen["closed"]
    assert seen["env"]["groups"] == 1                           # one fused launch balances its envs itself
    seen.clear()
    with pytest.raises(_Reached):
        run.main(argv)
    assert "fused_rollout" not in seen["learn"] and seen["env"]["groups"] == 2


CLI_REFUSALS = [
    ("no-co-train", ["--fused_rollout"], "--fused_rollout belongs to --co_train"),
    ("cfrc", ["--co_train", "--fused_rollout", "--cfrc_mode", "rne_post"], "--co_train --fused_rollout: not with --cfrc_mode rne_post"),
]


@pytest.mark.parametrize("name,argv,msg", CLI_REFUSALS, ids=[r[0] for r in CLI_REFUSALS])
def test_cli_refusals_come_before_an_env_is_built(name, argv, msg, tmp_path, monkeypatch):
    import torch
    import run
    from robosumo_selfplay_amd import alg_ppo, vec_env
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the device was asked for"))
    monkeypatch.setattr(vec_env, "make_vec_env", lambda *a, **kw: pytest.fail("an env was built"))
    monkeypatch.setattr(alg_ppo, "learn", lambda **kw: pytest.fail("a learner was started"))
    monkeypatch.setenv("WORLD_SIZE", "1")
    with pytest.raises(SystemExit) as e:
        run.main(["--env", "RoboSumo-Ant-vs-Bug-v0", "--num_env", "32", "--log_path", str(tmp_path)] + argv)
    assert msg in str(e.value)
    assert os.listdir(str(tmp_path)) == []


def _cfrc_env():
    env = _Env()
    env.cfrc_mode = "rne_post"
    return env


def test_cfrc_refusals_come_before_the_device(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the device was asked for"))
    kw = dict(network="mlp", opponent_mode="latest", nsteps=8, nminibatches=2)
    with pytest.raises(ValueError, match=r"fused_rollout=True \(--fused_rollout\) is not available on an env with cfrc_mode='rne_post'.*use fused_rollout=False"):
        co_train.check_learn(_cfrc_env(), fused_rollout=True, **kw)
    co_train.check_learn(_cfrc_env(), **kw)                      # the step-by-step path keeps running that mode
    co_train.check_learn(_Env(), fused_rollout=True, **kw)
    with pytest.raises(ValueError, match="fused_rollout=True"):
        co_train.learn(env=_cfrc_env(), total_timesteps=512, log_dir=str(tmp_path), verbose=False, fused_rollout=True, **kw)
    assert os.listdir(str(tmp_path)) == []
    with pytest.raises(ValueError, match=r"PairRunner\(engine_fused=True\) is not available on an env with cfrc_mode='rne_post'.*use engine_fused=False"):
        co_train.PairRunner(_cfrc_env(), [None, None], 8, 0.99, 0.95, engine_fused=True)


def test_every_new_message_is_distinct():
    msgs = [m for _, _, m in CLI_REFUSALS]
    for what, instead in (("co-training: fused_rollout=True (--fused_rollout)", "fused_rollout=False"), ("PairRunner(engine_fused=True)", "engine_fused=False")):
        with pytest.raises(ValueError) as e:
            co_train.check_engine_fused(_cfrc_env(), True, what, instead)
        msgs.append(str(e.value))
    assert len(set(msgs)) == len(msgs) == 4
    # the launch's own refusals: one code each, the sides named
    src = open(os.path.join(ROOT, "robosumo_selfplay_amd", "csrc", "engine_host_fused.h")).read()
    body = src[src.index("static int check_pair_rollout("):src.index('extern "C" int sumo_rollout_steps_pair(')]
    import re
    fails = re.findall(r'FAIL\((-\d+), "([^"]*)"', body)
    assert len(fails) == 12 and len({c for c, _ in fails}) == 12 and len({m for _, m in fails}) == 12
    assert sum(m.startswith("side %d:") for _, m in fails) == 8
