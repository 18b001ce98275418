"""CPU checks of the mixed match-up learner (robosumo_selfplay_amd/mixed.py): what ``learn`` refuses before it touches a device, the
learner seat's shape check, the league deal, the ctypes mirrors of the new C structs, the status encoding, and which Runner class
``learn`` picks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from robosumo_selfplay_amd import alg_ppo, matches, mixed, policies, ppo_capi, zoo_pairs
from robosumo_selfplay_amd.spaces import Box, Tuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


class _Env:
    """An env as ``learn`` looks at it before the first rollout; Ant-vs-Bug by default."""

    def __init__(self, obs_dims=(121, 165), act_dims=(8, 12), num_envs=32):
        self.model = type("Model", (), {"obs_dims": tuple(obs_dims), "act_dims": tuple(act_dims)})()
        self.num_envs, self.device = num_envs, "cuda:0"
        self.observation_space = Tuple([Box(-np.inf * np.ones(d), np.inf * np.ones(d)) for d in obs_dims])
        self.action_space = Tuple([Box(-np.ones(a), np.ones(a)) for a in act_dims])
        self.spec = type("Spec", (), {"id": "stub"})()


def _zoo_file(tmp_path, key):
    with np.load(os.path.join(HERE, "golden", "zoo_v3_params.npz"), allow_pickle=False) as z:
        p = os.path.join(str(tmp_path), key + ".npy")
        np.save(p, z[key])
    return p


REFUSALS = [
    (dict(use_opponent_data="direct"), NotImplementedError, "cannot score another species' action"),
    (dict(network="lstm"), NotImplementedError, "the learner's seat holds MLP"),
    (dict(opponent_pool=2), ValueError, "opponent_pool > 1"),
    (dict(fused_fix_opponent=True), NotImplementedError, "engine's fused rollout launch"),
    (dict(fused_selector=True), ValueError, "fused_selector serves opponent_mode='ours'"),
    (dict(eval_interval=1), NotImplementedError, "evaluation while training"),
    (dict(comm=object()), NotImplementedError, "single GPU"),
    (dict(env=_Env(num_envs=40)), ValueError, "num_envs = 40 is not a multiple of 16"),
    (dict(fix_opponent_path=None), ValueError, "needs fix_opponent_path"),
]


@pytest.mark.parametrize("kw,exc,msg", REFUSALS, ids=[sorted(k)[0] for k, _, _ in REFUSALS])
def test_learn_refusals_come_before_the_device(kw, exc, msg, tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the device was asked for"))
    args = dict(network="mlp", env=_Env(), total_timesteps=512, opponent_mode="fix", fix_opponent_path=_zoo_file(tmp_path, "bug-mlp-v3"),
                nsteps=8, log_dir=str(tmp_path), verbose=False)
    args.update(kw)
    with pytest.raises(exc, match=msg) as e:
        alg_ppo.learn(**args)
    assert "mixed match-up" in str(e.value) or "fix_opponent_path" in str(e.value)
    assert not os.path.exists(os.path.join(str(tmp_path), "checkpoints"))      # nothing was written either


def test_every_refusal_has_its_own_message():
    assert len({m for _, _, m in REFUSALS}) == len(REFUSALS)


def test_zoo_file_of_the_wrong_species_is_refused(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the device was asked for"))
    for key in ("ant-mlp-v3", "spider-lstm-v3"):
        with pytest.raises(ValueError, match=r"another species"):
            alg_ppo.learn(network="mlp", env=_Env(), total_timesteps=512, opponent_mode="fix", fix_opponent_path=[_zoo_file(tmp_path, key)],
                          nsteps=8, log_dir=str(tmp_path), verbose=False)


def test_learner_seat_refuses_another_shape():
    ant = np.zeros(matches.param_count(121, 8), np.float32)
    with pytest.raises(ValueError, match=r"121 observations and 8 actions.*165 observations and 12 actions"):
        mixed.LearnerSeat(165, 12, [ant])
    plist = [np.zeros(s, np.float32) for s in policies.param_shapes(121, 8)]
    with pytest.raises(ValueError, match=r"121 observations and 8 actions.*165 observations and 12 actions"):
        mixed.LearnerSeat(165, 12, [plist])
    with pytest.raises(ValueError, match="at least one net"):
        mixed.LearnerSeat(165, 12, [])
    assert mixed._shape_of_count(matches.param_count(209, 16)) == (209, 16) and mixed._shape_of_count(17) is None


def test_is_mixed():
    assert mixed.is_mixed(_Env()) and not mixed.is_mixed(_Env((121, 121), (8, 8))) and not mixed.is_mixed(object())
    assert mixed.is_mixed(_Env((121, 121), (8, 12)))


def test_league_deal_rotates_by_one_tile_per_update():
    a, b, c = (mixed.league_tiles(3, 80, u) for u in (1, 2, 3))
    assert a.tolist() == [0, 1, 2, 0, 1] and b.tolist() == [1, 2, 0, 1, 2] and c.tolist() == [2, 0, 1, 2, 0]
    assert a.dtype == np.int32 and np.array_equal(mixed.league_tiles(3, 80, 4), a)
    assert mixed.league_tiles(1, 32, 7).tolist() == [0, 0]
    with pytest.raises(ValueError, match="at least as many 16-env tiles"):
        mixed.league_tiles(3, 32, 1)


STRUCTS = [("ppo_learner_seat", ppo_capi.LearnerSeat), ("ppo_mixed_record", ppo_capi.MixedRecord), ("ppo_zoo_seat", ppo_capi.ZooSeat)]


def test_ctypes_mirrors_match_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sumo_ppo.h"', 'int main(void) {']
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
        last = st._fields_[-1][0]
        assert getattr(st, last).offset + getattr(st, last).size + 8 > table[(cname, "size")], cname     # every field is mirrored


@pytest.mark.parametrize("n", [16, 48, 4096])
def test_status_round_trip(n):
    seen = set()
    for tile in range(n // 16):
        for side in (0, 1):
            s = ppo_capi.mixed_status(tile, side)
            assert 0 < s < 2 ** 31 and ppo_capi.mixed_status_decode(s) == (tile, side)
            seen.add(s)
    assert len(seen) == 2 * (n // 16)
    with pytest.raises(ValueError):
        ppo_capi.mixed_status_decode(0)


def test_export_is_declared():
    assert "ppo_mixed_step" in ppo_capi.EXPORTS and "ppo_mixed_step" in open(os.path.join(ROOT, "include", "sumo_ppo.h")).read()


class _Chosen(Exception):
    pass


class _StubModel:
    def __init__(self, **kw):
        import torch
        self.params = torch.zeros(4)
        self.act_model = type("Pi", (), {"seed": lambda self, s: None})()

    def save(self, path):
        pass

    def load(self, path):
        pass


@pytest.mark.parametrize("dims,mode,want", [(((121, 121), (8, 8)), "fix", "Runner"), (((121, 121), (8, 8)), "ours", "Runner"),
                                            (((121, 165), (8, 12)), "fix", "MixedRunner"), (((121, 165), (8, 12)), "latest", "Runner")])
def test_which_runner_learn_builds(dims, mode, want, tmp_path, monkeypatch):
    def chosen(name):
        def build(*a, **kw):
            raise _Chosen(name)
        return build
    monkeypatch.setattr(alg_ppo, "Runner", chosen("Runner"))
    monkeypatch.setattr(mixed, "MixedRunner", chosen("MixedRunner"))
    monkeypatch.setattr(zoo_pairs, "seat_for", lambda env, side, sources: "seat")
    with pytest.raises(_Chosen, match="^%s$" % want):
        alg_ppo.learn(network="mlp", env=_Env(*dims), total_timesteps=512, opponent_mode=mode, fix_opponent_path="zoo.npy", nsteps=8,
                      nagent=2, log_dir=str(tmp_path), verbose=False, model_fn=_StubModel, value_network="copy", num_hidden=64,
                      activation="relu")
