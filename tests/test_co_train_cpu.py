"""CPU checks of two-species co-training (robosumo_selfplay_amd/co_train.py): what ``co_train.learn`` and ``run.py --co_train`` refuse
before they touch a device or write a file, the tile halves, the selection law, the ctypes mirror of ``ppo_pair_side``, and that
``alg_ppo.learn`` keeps meeting the Runner on a mixed env in the self-play modes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from robosumo_selfplay_amd import alg_ppo, co_train, mixed, ppo_capi
from robosumo_selfplay_amd.spaces import Box, Tuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class _Env:
    """An env as ``learn`` looks at it before the first rollout; Ant-vs-Bug by default."""

    def __init__(self, obs_dims=(121, 165), act_dims=(8, 12), num_envs=32):
        self.model = type("Model", (), {"obs_dims": tuple(obs_dims), "act_dims": tuple(act_dims)})()
        self.num_envs, self.device = num_envs, "cuda:0"
        self.observation_space = Tuple([Box(-np.inf * np.ones(d), np.inf * np.ones(d)) for d in obs_dims])
        self.action_space = Tuple([Box(-np.ones(a), np.ones(a)) for a in act_dims])
        self.spec = type("Spec", (), {"id": "stub"})()


REFUSALS = [
    ("homogeneous", dict(env=_Env((121, 121), (8, 8))), ValueError, "homogeneous match-up, which alg_ppo.learn trains"),
    ("ours", dict(opponent_mode="ours"), ValueError, "opponent_mode must be 'latest' or 'random', got 'ours'"),
    ("fix", dict(opponent_mode="fix"), ValueError, "opponent_mode must be 'latest' or 'random', got 'fix'"),
    ("lstm", dict(network="lstm"), NotImplementedError, "both seats hold MLP"),
    ("num_envs", dict(env=_Env(num_envs=48)), ValueError, "num_envs = 48 is not a multiple of 32"),
    ("minibatches", dict(nminibatches=5), ValueError, r"128 rows does not split into nminibatches = 5"),
]


@pytest.mark.parametrize("name,kw,exc,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_learn_refusals_come_before_the_device(name, kw, exc, msg, tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the device was asked for"))
    args = dict(env=_Env(), total_timesteps=512, opponent_mode="latest", nsteps=8, nminibatches=2, log_dir=str(tmp_path), verbose=False)
    args.update(kw)
    with pytest.raises(exc, match=msg):
        co_train.learn(**args)
    assert os.listdir(str(tmp_path)) == []                                 # nothing was written either


def test_every_learn_refusal_has_its_own_message():
    assert len({m for _, _, _, m in REFUSALS}) == len(REFUSALS)


def test_cfrc_mode_is_not_refused():
    env = _Env()
    env.cfrc_mode = "rne_post"
    co_train.check_learn(env, network="mlp", opponent_mode="random", nsteps=8, nminibatches=4)


CLI_REFUSALS = [
    ("algo", ["--algo", "ac"], "--algo ac is not available"),
    ("lstm", ["--network", "lstm"], "--network lstm is not available"),
    ("fix", ["--opponent_mode=fix"], "--opponent_mode=fix: a learner against policy-zoo nets"),
    ("ours", ["--opponent_mode=ours"], "--opponent_mode=ours: the selector would have to score"),
    ("reuse", ["--use_opponent_data=direct"], "--use_opponent_data is not available"),
    ("pool", ["--opponent_pool=4"], "--opponent_pool is not available"),
    ("selector", ["--fused_selector"], "--fused_selector serves opponent_mode=ours"),
    ("eval", ["--eval_interval", "2"], "evaluation while training"),
    ("ranks", [], "runs on a single GPU"),
]


@pytest.mark.parametrize("name,argv,msg", CLI_REFUSALS, ids=[r[0] for r in CLI_REFUSALS])
def test_cli_refusals_come_before_an_env_is_built(name, argv, msg, tmp_path, monkeypatch):
    import torch
    import run
    from robosumo_selfplay_amd import vec_env
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the device was asked for"))
    monkeypatch.setattr(vec_env, "make_vec_env", lambda *a, **kw: pytest.fail("an env was built"))
    monkeypatch.setenv("WORLD_SIZE", "2" if name == "ranks" else "1")
    with pytest.raises(SystemExit) as e:
        run.main(["--co_train", "--env", "RoboSumo-Ant-vs-Bug-v0", "--num_env", "32", "--log_path", str(tmp_path)] + argv)
    assert msg in str(e.value) and "--co_train" in str(e.value)
    assert os.listdir(str(tmp_path)) == []


def test_every_cli_refusal_has_its_own_message():
    assert len({m for _, _, m in CLI_REFUSALS}) == len(CLI_REFUSALS)


def test_tile_halves():
    r0, r1 = co_train.tile_halves(32)
    assert r0.tolist() == [0, 1] and r1.tolist() == [1, 0] and r0.dtype == np.int32 and r1.dtype == np.int32
    r0, r1 = co_train.tile_halves(96)
    assert r0.tolist() == [0, 0, 0, 1, 1, 1] and r1.tolist() == [1, 1, 1, 0, 0, 0]
    for n in (48, 16, 0):
        with pytest.raises(ValueError, match="not a multiple of 32"):
            co_train.tile_halves(n)
    # a learner's own envs are the half in which its live row (0) plays
    for side, rows in enumerate(co_train.tile_halves(96)):
        sl = co_train.own_envs(96, side)
        assert np.repeat(rows, 16)[sl].tolist() == [0] * 48 and sl.stop - sl.start == 48


def _run_dirs(tmp_path, n0, n1):
    dirs = []
    for s, n in enumerate((n0, n1)):
        d = tmp_path / ("agent%d" % s) / "checkpoints"
        d.mkdir(parents=True)
        for k in range(n):
            (d / ("%.5i" % k)).write_bytes(b"")
        dirs.append(str(d))
    return dirs


def _histories():
    return [dict(version_gap=[], opponent_versions=[]) for _ in range(2)]


def predicted_random_versions(rng, updates):
    """The versions 'random' records when numpy's global stream stands where ``rng`` (a ``RandomState``) stands: per update from 2 on,
    one draw per side in side order, each among the ``update`` files present."""
    out = [[[0]], [[0]]]
    for u in range(2, updates + 1):
        for s in range(2):
            out[s].append([int(rng.choice(u))])
    return out


def test_selection_law(tmp_path):
    dirs = _run_dirs(tmp_path, 4, 3)
    h = _histories()
    # update 1: 00000 of the OTHER side, whatever the mode and the directories hold
    for mode in ("latest", "random"):
        got = co_train.choose_frozen(1, mode, dirs, h)
        assert got == [os.path.join(dirs[1], "00000"), os.path.join(dirs[0], "00000")]
    assert h[0]["opponent_versions"] == [[0], [0]] and h[1]["version_gap"] == [0, 0]
    # latest: the newest file of the other side's directory
    h = _histories()
    got = co_train.choose_frozen(4, "latest", dirs, h)
    assert got == [os.path.join(dirs[1], "00002"), os.path.join(dirs[0], "00003")]
    assert h[0]["opponent_versions"] == [[2]] and h[1]["opponent_versions"] == [[3]] and h[0]["version_gap"] == []
    with pytest.raises(ValueError, match="opponent_mode"):
        co_train.choose_frozen(2, "ours", dirs, _histories())


def test_random_selection_draws_in_side_order(tmp_path):
    dirs = [str(tmp_path / "agent0" / "checkpoints"), str(tmp_path / "agent1" / "checkpoints")]
    for d in dirs:
        os.makedirs(d)
        open(os.path.join(d, "00000"), "wb").close()
    h = _histories()
    state = np.random.get_state()                                       # the global stream is put back: other tests draw from it
    np.random.seed(11)
    try:
        for u in range(1, 6):
            got = co_train.choose_frozen(u, "random", dirs, h)
            for s in range(2):
                assert got[s] == os.path.join(dirs[1 - s], "%.5i" % h[s]["opponent_versions"][-1][0])
            for d in dirs:                                              # what learn saves after the update
                open(os.path.join(d, "%.5i" % u), "wb").close()
    finally:
        np.random.set_state(state)
    want = predicted_random_versions(np.random.RandomState(11), 5)
    assert h[0]["opponent_versions"] == want[0] and h[1]["opponent_versions"] == want[1]
    assert h[0]["version_gap"] == [0] + [u - 1 - want[0][u - 1][0] for u in range(2, 6)]


def test_pair_side_mirrors_the_header():
    """``ppo_pair_side`` (include/sumo_ppo.h) on an LP64 target, by hand: seat {table 0, tile_row 8, nrows 16, row_stride 20, ob_dim 24,
    ac_dim 28} = 32 bytes; obs 32, noise 40, done 48, action 56; record {obs, action, neglogp, value, done} = 40 bytes at 64."""
    P = ppo_capi.PairSide
    assert C.sizeof(ppo_capi.LearnerSeat) == 32 and C.sizeof(ppo_capi.MixedRecord) == 40
    want = dict(seat=0, obs=32, noise=40, done=48, action=56, record=64)
    assert [f for f, _ in P._fields_] == list(want)
    for f, off in want.items():
        assert getattr(P, f).offset == off, f
    assert C.sizeof(P) == 104 and C.sizeof(P * 2) == 208
    seat = dict(table=0, tile_row=8, nrows=16, row_stride=20, ob_dim=24, ac_dim=28)
    for f, off in seat.items():
        assert getattr(ppo_capi.LearnerSeat, f).offset == off, f
    header = open(os.path.join(ROOT, "include", "sumo_ppo.h")).read()
    assert "ppo_mixed_pair_step" in ppo_capi.EXPORTS and "int ppo_mixed_pair_step(const ppo_pair_side sides[2]" in header
    decl = header[header.index("typedef struct ppo_pair_side {"):header.index("} ppo_pair_side;")]
    order = [decl.index(w) for w in ("ppo_learner_seat seat;", "*obs, *noise;", "uint8_t* done;", "float* action;", "ppo_mixed_record record;")]
    assert order == sorted(order)


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


@pytest.mark.parametrize("mode", ["latest", "random"])
def test_alg_ppo_learn_still_meets_the_runner_on_a_mixed_env(mode, tmp_path, monkeypatch):
    def build(*a, **kw):
        raise _Chosen("Runner")
    monkeypatch.setattr(alg_ppo, "Runner", build)
    monkeypatch.setattr(co_train, "PairRunner", lambda *a, **kw: pytest.fail("alg_ppo.learn reached co-training"))
    monkeypatch.setattr(mixed, "MixedRunner", lambda *a, **kw: pytest.fail("alg_ppo.learn reached the fix-mode runner"))
    with pytest.raises(_Chosen, match="^Runner$"):
        alg_ppo.learn(network="mlp", env=_Env(), total_timesteps=512, opponent_mode=mode, nsteps=8, nagent=2, log_dir=str(tmp_path),
                      verbose=False, model_fn=_StubModel, value_network="copy", num_hidden=64, activation="relu")


def test_agent_1_episode_sums_carry_across_rollouts():
    import torch
    rew = torch.tensor([[1.0, 10.0], [2.0, 20.0], [4.0, 40.0]], dtype=torch.float32)            # [T = 3][N = 2]
    done = torch.tensor([[False, False], [True, False], [False, False]])
    sums, carry = co_train.running_episode_sums(rew, done, torch.tensor([0.5, 0.0], dtype=torch.float64))
    assert sums.dtype == torch.float64 and sums.tolist() == [[1.5, 10.0], [3.5, 30.0], [4.0, 70.0]]
    assert sums[done].tolist() == [3.5] and carry.tolist() == [4.0, 70.0]           # env 0 closed 0.5 + 1 + 2 and restarted; env 1 stays open
    sums2, carry2 = co_train.running_episode_sums(rew[:1], torch.tensor([[True, True]]), carry)
    assert sums2.tolist() == [[5.0, 80.0]] and carry2.tolist() == [0.0, 0.0]        # the next rollout closes both, the carry included
