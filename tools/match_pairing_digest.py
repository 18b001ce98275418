#!/usr/bin/env python3
"""One SHA-256 per match pairing, path and driver call of ``robosumo_selfplay_amd/matches.py``, to compare two commits bit for bit.

    python tools/match_pairing_digest.py > pairings.txt               # one GPU; on each commit, the two files must be identical
    python tools/match_pairing_digest.py --refusals > refusals.txt    # no GPU: what every public entry refuses, and in which order

The fused-vs-stepwise tests compare two paths of ONE commit; a change that rewrites both passes them.  This tool anchors a rewrite
of ``matches.py`` against its parent: it drives only what both sides have -- the twelve public ``*_match_steps_*`` functions,
``match_steps`` and the public drivers.

Step functions: Ant-vs-Ant, 64 envs, step counters near the time limit (tests/test_gpu_zoo_league.py ``_near_time_limit``) so that
episodes end, scores move and recurrent states are masked inside the window; K = 3, two calls in a row; quota 2 with a score tensor
that starts at 0, 1 or 2 finished games per env, so the cut-off is reached in some envs, passed in others and not reached in the
rest.  Every pairing fused and step by step, with noise and deterministic; one MLP and one LSTM pairing also on two env groups;
LSTM(64) checkpoints step by step only.  ``<pairing> <path> <noise> groups<g> call<k> <sha256>`` over the score, every state
tensor, ``env.act_dev``, ``env.obs_dev``, ``env.done_dev`` and every engine's ``get_state()``.

Drivers: 4 trials on 8 envs in launches of 16 steps, fused and step by step; the hash covers ``repr`` of the returned dict.

Checkpoint nets are the seeded builders of tests/test_gpu_matches_cross.py, zoo nets the golden ``ant-mlp-v3`` / ``ant-lstm-v3``
(tests/zoo_lstm_helpers.py) next to a synthetic one.

``--refusals`` prints ``case -> exception type: message`` for a fixed list of bad inputs to every public step function and play
driver on stand-in envs and CPU tables: every refusal the match tests pin, and per function inputs that violate two checks at once
(the check named first in the case is the one that must fire)."""
import hashlib
import os
import pathlib
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

ANT = "RoboSumo-Ant-vs-Ant-v0"
N, K, QUOTA, CALLS = 64, 3, 2, 2
N_MLP, N_LSTM, N_ZOO = 3, 2, 2
RECURRENT = ("lstm", "lstm_zoo_lstm", "cross_lstm0", "cross_lstm1", "lstm_zoo")   # the pairings that hold an LSTM checkpoint table


# ---- the GPU digest -----------------------------------------------------------------------------------------------------------------
def _zoo_tables(env, D, A):
    from zoo_lstm_helpers import golden, synthetic_lstm_flat
    import test_gpu_matches_cross as X
    from robosumo_selfplay_amd import policy_zoo
    return X._zoo_table(env), policy_zoo.ZooLstmTable([golden("ant-lstm-v3"), synthetic_lstm_flat(D - 1, A, 21)], A, env.device)


def _pairings(M, mt, lt, zoo, zl):
    """name -> (rows of agent 0's table, of agent 1's, state widths per agent, call(fused, env, idx0, idx1, states, score, noise));
    ``states`` holds the tensors of the non-None widths, in agent order."""
    W = 2 * lt.spec.nlstm
    two = lambda fused, a, b: a if fused else b
    return {
        "mlp": (N_MLP, N_MLP, (None, None), lambda f, e, i0, i1, st, sc, nz: M.match_steps(e, mt, i0, i1, None, sc, QUOTA, K, nz, fused=f)),
        "lstm": (N_LSTM, N_LSTM, (W, W), lambda f, e, i0, i1, st, sc, nz: M.match_steps(e, lt, i0, i1, tuple(st), sc, QUOTA, K, nz, fused=f)),
        "zoo": (N_MLP, N_ZOO, (None, None), lambda f, e, i0, i1, st, sc, nz: two(f, M.zoo_match_steps_fused, M.zoo_match_steps_stepwise)(
            e, mt, zoo, i0, i1, sc, QUOTA, K, nz)),
        "zoo_lstm": (N_MLP, N_ZOO, (None, 128), lambda f, e, i0, i1, st, sc, nz: two(f, M.zoo_lstm_match_steps_fused, M.zoo_lstm_match_steps_stepwise)(
            e, mt, zl, i0, i1, st[0], sc, QUOTA, K, nz)),
        "lstm_zoo_lstm": (N_LSTM, N_ZOO, (W, 128), lambda f, e, i0, i1, st, sc, nz: two(f, M.zoo_lstm_match_steps_fused, M.zoo_lstm_match_steps_stepwise)(
            e, lt, zl, i0, i1, tuple(st), sc, QUOTA, K, nz)),
        "cross_lstm0": (N_LSTM, N_MLP, (W, None), lambda f, e, i0, i1, st, sc, nz: two(f, M.cross_match_steps_fused, M.cross_match_steps_stepwise)(
            e, mt, lt, 0, i0, i1, st[0], sc, QUOTA, K, nz)),
        "cross_lstm1": (N_MLP, N_LSTM, (None, W), lambda f, e, i0, i1, st, sc, nz: two(f, M.cross_match_steps_fused, M.cross_match_steps_stepwise)(
            e, mt, lt, 1, i0, i1, st[0], sc, QUOTA, K, nz)),
        "lstm_zoo": (N_LSTM, N_ZOO, (W, None), lambda f, e, i0, i1, st, sc, nz: two(f, M.lstm_zoo_match_steps_fused, M.lstm_zoo_match_steps_stepwise)(
            e, lt, zoo, i0, i1, st[0], sc, QUOTA, K, nz)),
    }


def _sha(items):
    import numpy as np
    import torch
    h = hashlib.sha256()
    for x in items:
        x = np.ascontiguousarray(x.cpu().numpy() if torch.is_tensor(x) else x)
        h.update(("%s%s" % (x.dtype, x.shape)).encode())
        h.update(x.tobytes())
    return h.hexdigest()


def step_functions():
    import numpy as np
    import torch
    import test_gpu_matches_cross as X
    import test_gpu_zoo_league as L
    from robosumo_selfplay_amd import matches as M
    for groups, names in ((1, None), (2, ("mlp", "lstm"))):
        np.random.seed(groups)                                   # the MLP builder starts from numpy's global generator
        env = X._env(ANT, N, groups)
        D, A = X._dims(env)
        mt, zoo_zl = X._mlp_table(env), _zoo_tables(env, D, A)
        for H in (128, 64) if groups == 1 else (128,):
            pairings = _pairings(M, mt, X._lstm_table(env, H=H), *zoo_zl)
            for name, (n0, n1, widths, call) in pairings.items():
                if (names is not None and name not in names) or (H == 64 and name not in RECURRENT):
                    continue
                rng = np.random.default_rng(5)
                idx0, idx1 = rng.integers(0, n0, N).astype(np.int32), rng.integers(0, n1, N).astype(np.int32)
                assert idx0.max() == n0 - 1 and idx1.max() == n1 - 1
                i0, i1 = torch.from_numpy(idx0).cuda(), torch.from_numpy(idx1).cuda()
                for fused in (True, False) if H == 128 else (False,):
                    for deterministic in (False, True):
                        env._needs_seed = True
                        env.reset_device()
                        L._near_time_limit(env)
                        states = [torch.zeros((N, w), dtype=torch.float32, device="cuda") for w in widths if w is not None]
                        score = torch.zeros((N, 3), dtype=torch.int32, device="cuda")
                        e = torch.arange(N, device="cuda")
                        score[e, e % 3] = (e % 3).to(torch.int32)          # 0, 1 or 2 games finished before the window
                        gen = torch.Generator(device="cuda")
                        gen.manual_seed(3)
                        for k in range(CALLS):
                            noise = None if deterministic else tuple(torch.randn((K, N, A), generator=gen, device="cuda") for _ in range(2))
                            call(fused, env, i0 if fused else idx0, i1 if fused else idx1, states, score, noise)
                            torch.cuda.synchronize()
                            assert env.stats()["rollout_aborts"] == 0, name
                            state = [score] + states + [env.act_dev, env.obs_dev, env.done_dev] + [x for E in env.engines for x in E.get_state()]
                            print("%s%s" % (name, "" if H == 128 else "-lstm64"), "fused" if fused else "step", "det" if deterministic else "noise",
                                  "groups%d" % groups, "call%d" % k, _sha(state), flush=True)
                        assert int(score.sum(1).max()) == QUOTA
        env.close()


def drivers():
    import numpy as np
    import test_gpu_matches_cross as X
    from zoo_lstm_helpers import golden
    from robosumo_selfplay_amd import matches as M
    np.random.seed(8)                                            # the MLP builder starts from numpy's global generator
    env = X._env(ANT, 8)
    D, A = X._dims(env)
    mt, lt = X._mlp_table(env), X._lstm_table(env)
    zoo, zl = _zoo_tables(env, D, A)
    epp, rpe = M.split_trials(4, 8)
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        mlp, lstm = X._save_runs(tmp, np.random.default_rng(2), n_mlp=2, n_lstm=2)
        mlp_b, lstm_b = X._save_runs(tmp, np.random.default_rng(3), n_mlp=2, n_lstm=2, suffix="_b")
        files = [str(tmp / "zoo-mlp.npy"), str(tmp / "zoo-lstm.npy")]
        np.save(files[0], golden("ant-mlp-v3"))
        np.save(files[1], golden("ant-lstm-v3"))
        kw, ckw = dict(seed=7, chunk=16), dict(num_env=8, seed=3, chunk=16)
        calls = [
            ("play_matches-mlp", lambda f: M.play_matches(env, mt, [(2, 1), (0, 0), (1, 2)], rpe, epp, fused=f, **kw)),
            ("play_matches-lstm", lambda f: M.play_matches(env, lt, [(1, 0), (0, 0), (0, 1)], rpe, epp, fused=f, **kw)),
            ("play_cross_matches-lstm1", lambda f: M.play_cross_matches(env, mt, lt, [(2, 1), (0, 0), (1, 1)], rpe, epp, fused=f, **kw)),
            ("play_cross_matches-lstm0", lambda f: M.play_cross_matches(env, lt, mt, [(1, 2), (0, 0), (1, 1)], rpe, epp, fused=f, **kw)),
            ("play_against_zoo-mlp-zoo_mlp", lambda f: M.play_against_zoo(env, mt, zoo, [(2, 1), (0, 0), (1, 1)], rpe, epp, fused=f, **kw)),
            ("play_against_zoo-mlp-zoo_lstm", lambda f: M.play_against_zoo(env, mt, zl, [(2, 1), (0, 0), (1, 1)], rpe, epp, fused=f, **kw)),
            ("play_against_zoo-lstm-zoo_lstm", lambda f: M.play_against_zoo(env, lt, zl, [(1, 1), (0, 0), (1, 0)], rpe, epp, fused=f, **kw)),
            ("play_against_zoo-lstm-zoo_mlp", lambda f: M.play_against_zoo(env, lt, zoo, [(1, 1), (0, 0), (1, 0)], rpe, epp, fused=f,
                                                                         cross_family=True, **kw)),
            ("compare_history_versions-mlp", lambda f: M.compare_history_versions(mlp, mlp_b, 4, fused=f, **ckw)),
            ("compare_history_versions-lstm", lambda f: M.compare_history_versions(lstm, lstm_b, 4, fused=f, **ckw)),
            ("compare_history_versions-cross-lstm1", lambda f: M.compare_history_versions(mlp, lstm, 4, fused=f, cross_family=True, **ckw)),
            ("compare_history_versions-cross-lstm0", lambda f: M.compare_history_versions(lstm, mlp, 4, fused=f, cross_family=True, **ckw)),
            ("evaluate_history_against_zoo-mlp", lambda f: M.evaluate_history_against_zoo(mlp, files, 4, start=1, fused=f, **ckw)),
            ("evaluate_history_against_zoo-lstm", lambda f: M.evaluate_history_against_zoo(lstm, files, 4, start=1, fused=f, cross_family=True,
                                                                                          **ckw)),
        ]
        for name, call in calls:
            for fused in (True, False):
                res = call(fused)
                if isinstance(res, dict):                        # the run directories are temporary: their paths stay out of the hash
                    res = {k: v for k, v in res.items() if k != "opponents"}
                print(name, "fused" if fused else "step", hashlib.sha256(repr(res).encode()).hexdigest(), flush=True)
    assert env.stats()["rollout_aborts"] == 0
    env.close()


# ---- the refusals, on the CPU -------------------------------------------------------------------------------------------------------
D, A = 121, 8


class _Model:
    timestep_limit = 500

    def __init__(self, obs, act):
        self.obs_dims, self.act_dims = obs, act


class _Env:
    """What the checks touch of a SumoVecEnv."""

    def __init__(self, n=8, obs=(D, D), act=(A, A), cfrc_mode="zero"):
        import numpy as np
        import torch
        self.num_envs, self.device, self.model, self.cfrc_mode = n, torch.device("cpu"), _Model(obs, act), cfrc_mode
        self.seeds, self.adjust_z = np.zeros(n, np.uint64), -0.5

    def reset_device(self):
        pass


class _WideZoo:
    recurrent, ac_dim, ob_dim, capacity = False, A, D + 1, 2


class _WideZooLstm:
    recurrent, ac_dim, ob_dim, capacity, hidden = True, A, D + 1, 2, 64


def refusals():
    import numpy as np
    import torch
    from zoo_lstm_helpers import golden
    from robosumo_selfplay_amd import matches as M, policies, policy_zoo
    from robosumo_selfplay_amd.lstm_model import LstmSpec
    rng = np.random.default_rng(3)

    def mlp_table(n, d=D, filled=None):
        t = M.SnapshotTable(policies.PolicySpec(d, A, value_network="copy", activation="relu"), n, "cpu")
        for k in range(n if filled is None else filled):
            t.set(k, [rng.standard_normal(s).astype(np.float32) for s in policies.param_shapes(d, A)])
        return t

    def lstm_table(n, H=128, filled=None):
        t = M.LstmSnapshotTable(LstmSpec(D, A, H), n, "cpu")
        for k in range(n if filled is None else filled):
            t.set(k, [rng.standard_normal(s).astype(np.float32) for s in policies.lstm_param_shapes(D, A, H)])
        return t

    mt, mt_b, mt_small, lt, lt_b, lt64 = mlp_table(4, filled=3), mlp_table(2), mlp_table(2, d=60), lstm_table(3, filled=2), lstm_table(2), lstm_table(2, 64)
    cpu = torch.device("cpu")
    zoo, zl = policy_zoo.ZooTable([golden("ant-mlp-v3")] * 2, A, cpu), policy_zoo.ZooLstmTable([golden("ant-lstm-v3")] * 2, A, cpu)
    wide, wide_l = _WideZoo(), _WideZooLstm()
    ok, het, rne = _Env(), _Env(obs=(D, 100)), _Env(cfrc_mode="rne_post")
    n = ok.num_envs
    i, sc = np.zeros(n, np.int32), torch.zeros((n, 3), dtype=torch.int32)
    s256, s128, s64 = (torch.zeros((n, w)) for w in (256, 128, 64))
    strided = torch.zeros((n, 512))[:, ::2]
    tail = (sc, 1, 1)
    cases = []

    def both(name, fn_f, fn_s, *args):
        """A case for the fused function and its step-by-step twin."""
        cases.append((name % "fused", lambda: fn_f(*args, *tail)))
        cases.append((name % "stepwise", lambda: fn_s(*args, *tail)))

    F, S = M.match_steps_fused, M.match_steps_stepwise
    both("match_steps_%s: heterogeneous env", F, S, het, mt, i, i)
    both("match_steps_%s: table of another observation space", F, S, ok, mt_small, i, i)
    both("match_steps_%s: rne_post", F, S, rne, mt, i, i)
    both("match_steps_%s: heterogeneous env, then table of another observation space", F, S, het, mt_small, i, i)
    F, S = M.match_steps_fused_lstm, M.match_steps_stepwise_lstm
    both("match_steps_%s_lstm: rne_post", F, S, rne, lt, i, i, (s256, s256))
    both("match_steps_%s_lstm: second state of the wrong shape", F, S, ok, lt, i, i, (s256, s128))
    both("match_steps_%s_lstm: first state not contiguous", F, S, ok, lt, i, i, (strided, s256))
    both("match_steps_%s_lstm: heterogeneous env, then state shape", F, S, het, lt, i, i, (s128, s128))
    cases.append(("match_steps_fused_lstm: LSTM(64)", lambda: M.match_steps_fused_lstm(ok, lt64, i, i, (s128, s128), *tail)))
    cases.append(("match_steps_fused_lstm: state shape, then LSTM(64)", lambda: M.match_steps_fused_lstm(ok, lt64, i, i, (s256, s256), *tail)))
    cases.append(("match_steps: rne_post (MLP table, fused)", lambda: M.match_steps(rne, mt, i, i, None, *tail)))
    cases.append(("match_steps: state shape (LSTM table, step by step)", lambda: M.match_steps(ok, lt, i, i, (s128, s128), *tail, fused=False)))
    cases.append(("match_steps: LSTM(64) (fused)", lambda: M.match_steps(ok, lt64, i, i, (s128, s128), *tail)))
    F, S = M.zoo_match_steps_fused, M.zoo_match_steps_stepwise
    both("zoo_match_steps_%s: heterogeneous env", F, S, het, mt, zoo, i, i)
    both("zoo_match_steps_%s: rne_post", F, S, rne, mt, zoo, i, i)
    both("zoo_match_steps_%s: LSTM table against zoo MLP nets", F, S, ok, lt, zoo, i, i)
    both("zoo_match_steps_%s: zoo nets wider than the observation", F, S, ok, mt, wide, i, i)
    both("zoo_match_steps_%s: rne_post, then LSTM table against zoo MLP nets", F, S, rne, lt, zoo, i, i)
    both("zoo_match_steps_%s: LSTM table against zoo MLP nets, then zoo width", F, S, ok, lt, wide, i, i)
    F, S = M.zoo_lstm_match_steps_fused, M.zoo_lstm_match_steps_stepwise
    both("zoo_lstm_match_steps_%s: rne_post", F, S, rne, mt, zl, i, i, s128)
    both("zoo_lstm_match_steps_%s: LSTM table against zoo MLP nets", F, S, ok, lt, zoo, i, i, (s256, s128))
    both("zoo_lstm_match_steps_%s: zoo nets wider than the observation", F, S, ok, mt, wide_l, i, i, s128)
    both("zoo_lstm_match_steps_%s: a ZooTable", F, S, ok, mt, zoo, i, i, s128)
    both("zoo_lstm_match_steps_%s: [N][256] is not a zoo state", F, S, ok, mt, zl, i, i, s256)
    both("zoo_lstm_match_steps_%s: zoo state not contiguous", F, S, ok, mt, zl, i, i, strided[:, :128])
    both("zoo_lstm_match_steps_%s: agent 0's state of the wrong shape", F, S, ok, lt, zl, i, i, (s128, s128))
    both("zoo_lstm_match_steps_%s: zoo width, then a ZooTable", F, S, ok, mt, wide, i, i, s128)
    both("zoo_lstm_match_steps_%s: a ZooTable, then state shape", F, S, ok, mt, zoo, i, i, s256)
    both("zoo_lstm_match_steps_%s: agent 0's state, then the zoo state", F, S, ok, lt, zl, i, i, (s128, s256))
    cases.append(("zoo_lstm_match_steps_fused: LSTM(64)", lambda: M.zoo_lstm_match_steps_fused(ok, lt64, zl, i, i, (s128, s128), *tail)))
    cases.append(("zoo_lstm_match_steps_fused: zoo state, then LSTM(64)", lambda: M.zoo_lstm_match_steps_fused(ok, lt64, zl, i, i, (s128, s256), *tail)))
    F, S = M.cross_match_steps_fused, M.cross_match_steps_stepwise
    both("cross_match_steps_%s: tables swapped", F, S, ok, lt, mt, 0, i, i, s256)
    both("cross_match_steps_%s: two MLP tables", F, S, ok, mt, mt_b, 0, i, i, s256)
    both("cross_match_steps_%s: lstm_side 2", F, S, ok, mt, lt, 2, i, i, s256)
    both("cross_match_steps_%s: heterogeneous env", F, S, het, mt, lt, 1, i, i, s256)
    both("cross_match_steps_%s: MLP table of another observation space", F, S, ok, mt_small, lt, 0, i, i, s256)
    both("cross_match_steps_%s: state of the wrong shape", F, S, ok, mt, lt, 1, i, i, s128)
    both("cross_match_steps_%s: tables swapped, then lstm_side 2", F, S, ok, lt, mt, 2, i, i, s256)
    both("cross_match_steps_%s: lstm_side 2, then heterogeneous env", F, S, het, mt, lt, 2, i, i, s256)
    both("cross_match_steps_%s: rne_post, then state shape", F, S, rne, mt, lt, 0, i, i, s128)
    cases.append(("cross_match_steps_fused: LSTM(64)", lambda: M.cross_match_steps_fused(ok, mt, lt64, 0, i, i, s128, *tail)))
    cases.append(("cross_match_steps_fused: state shape, then LSTM(64)", lambda: M.cross_match_steps_fused(ok, mt, lt64, 1, i, i, s256, *tail)))
    F, S = M.lstm_zoo_match_steps_fused, M.lstm_zoo_match_steps_stepwise
    both("lstm_zoo_match_steps_%s: an MLP table", F, S, ok, mt, zoo, i, i, s256)
    both("lstm_zoo_match_steps_%s: a ZooLstmTable", F, S, ok, lt, zl, i, i, s256)
    both("lstm_zoo_match_steps_%s: heterogeneous env", F, S, het, lt, zoo, i, i, s256)
    both("lstm_zoo_match_steps_%s: zoo nets wider than the observation", F, S, ok, lt, wide, i, i, s256)
    both("lstm_zoo_match_steps_%s: state of the wrong shape", F, S, ok, lt, zoo, i, i, s128)
    both("lstm_zoo_match_steps_%s: an MLP table, then heterogeneous env", F, S, het, mt, zoo, i, i, s256)
    both("lstm_zoo_match_steps_%s: rne_post, then zoo width", F, S, rne, lt, wide, i, i, s256)
    both("lstm_zoo_match_steps_%s: zoo width, then state shape", F, S, ok, lt, wide, i, i, s128)
    cases.append(("lstm_zoo_match_steps_fused: LSTM(64)", lambda: M.lstm_zoo_match_steps_fused(ok, lt64, zoo, i, i, s128, *tail)))
    cases.append(("lstm_zoo_match_steps_fused: state shape, then LSTM(64)", lambda: M.lstm_zoo_match_steps_fused(ok, lt64, zoo, i, i, s256, *tail)))
    cases += [
        ("play_matches: heterogeneous env", lambda: M.play_matches(het, mt, [(0, 1)], 1, 4)),
        ("play_matches: rne_post (step by step)", lambda: M.play_matches(rne, mt, [(0, 1)], 1, 4, fused=False)),
        ("play_matches: row past the table", lambda: M.play_matches(ok, mt, [(0, 1), (0, 4)], 1, 4)),
        ("play_matches: negative row", lambda: M.play_matches(ok, mt, [(-1, 0)], 1, 4)),
        ("play_matches: empty row", lambda: M.play_matches(ok, mt, [(3, 0)], 1, 4)),
        ("play_matches: empty row (LSTM table)", lambda: M.play_matches(ok, lt, [(0, 2)], 1, 4)),
        ("play_matches: rounds_per_env 0", lambda: M.play_matches(ok, mt, [(0, 1)], 0, 4)),
        ("play_matches: chunk 0", lambda: M.play_matches(ok, lt, [(0, 1)], 1, 4, chunk=0)),
        ("play_matches: LSTM(64) fused", lambda: M.play_matches(ok, lt64, [(0, 1)], 1, 4)),
        ("play_matches: more envs per pair than envs (LSTM(64) step by step)", lambda: M.play_matches(ok, lt64, [(0, 1)], 1, 9, fused=False)),
        ("play_matches: rne_post, then empty row", lambda: M.play_matches(rne, mt, [(3, 0)], 1, 4)),
        ("play_matches: empty row, then chunk 0", lambda: M.play_matches(ok, mt, [(3, 0)], 1, 4, chunk=0)),
        ("play_matches: chunk 0, then LSTM(64) fused", lambda: M.play_matches(ok, lt64, [(0, 1)], 1, 4, chunk=0)),
    ]
    cases += [
        ("play_cross_matches: one MLP table twice", lambda: M.play_cross_matches(ok, mt, mt, [(0, 1)], 1, 4)),
        ("play_cross_matches: one LSTM table twice", lambda: M.play_cross_matches(ok, lt, lt, [(0, 1)], 1, 4)),
        ("play_cross_matches: two MLP tables", lambda: M.play_cross_matches(ok, mt, mt_b, [(0, 1)], 1, 4)),
        ("play_cross_matches: two LSTM tables of different widths", lambda: M.play_cross_matches(ok, lt, lt64, [(0, 1)], 1, 4)),
        ("play_cross_matches: heterogeneous env", lambda: M.play_cross_matches(het, mt, lt, [(0, 1)], 1, 4)),
        ("play_cross_matches: agent 0's table of another observation space", lambda: M.play_cross_matches(ok, mt_small, lt, [(0, 1)], 1, 4)),
        ("play_cross_matches: row 2 exists in the MLP table only", lambda: M.play_cross_matches(ok, mt, lt, [(0, 2)], 1, 4)),
        ("play_cross_matches: the same, LSTM table first", lambda: M.play_cross_matches(ok, lt, mt, [(2, 0)], 1, 4)),
        ("play_cross_matches: row 3 is empty in the MLP table", lambda: M.play_cross_matches(ok, lt, mt, [(0, 3)], 1, 4)),
        ("play_cross_matches: rounds_per_env 0", lambda: M.play_cross_matches(ok, mt, lt, [(0, 1)], 0, 4)),
        ("play_cross_matches: LSTM(64) fused", lambda: M.play_cross_matches(ok, mt, lt64, [(0, 1)], 1, 4)),
        ("play_cross_matches: LSTM(64) fused, LSTM table first", lambda: M.play_cross_matches(ok, lt64, mt, [(0, 1)], 1, 4)),
        ("play_cross_matches: two MLP tables, then heterogeneous env", lambda: M.play_cross_matches(het, mt, mt_b, [(0, 1)], 1, 4)),
        ("play_cross_matches: rne_post, then row past the table", lambda: M.play_cross_matches(rne, mt, lt, [(0, 5)], 1, 4)),
        ("play_cross_matches: empty row, then chunk 0, then LSTM(64)", lambda: M.play_cross_matches(ok, mt, lt64, [(3, 0)], 1, 4, chunk=0)),
        ("play_cross_matches: chunk 0, then LSTM(64) fused", lambda: M.play_cross_matches(ok, mt, lt64, [(0, 1)], 1, 4, chunk=0)),
    ]
    cases += [
        ("play_against_zoo: LSTM table against zoo MLP nets", lambda: M.play_against_zoo(ok, lt, zoo, [(0, 0)], 1, 4)),
        ("play_against_zoo: the same, cross_family=False", lambda: M.play_against_zoo(ok, lt, zoo, [(0, 0)], 1, 4, cross_family=False)),
        ("play_against_zoo: the same, step by step", lambda: M.play_against_zoo(ok, lt, zoo, [(0, 0)], 1, 4, fused=False)),
        ("play_against_zoo: LSTM(64) against zoo MLP nets, cross_family", lambda: M.play_against_zoo(ok, lt64, zoo, [(0, 0)], 1, 4, cross_family=True)),
        ("play_against_zoo: LSTM(64) against zoo LSTM nets", lambda: M.play_against_zoo(ok, lt64, zl, [(0, 0)], 1, 4)),
        ("play_against_zoo: heterogeneous env", lambda: M.play_against_zoo(het, mt, zoo, [(0, 0)], 1, 4)),
        ("play_against_zoo: heterogeneous env, cross_family", lambda: M.play_against_zoo(het, lt, zoo, [(0, 0)], 1, 4, cross_family=True)),
        ("play_against_zoo: zoo nets wider than the observation", lambda: M.play_against_zoo(ok, mt, wide, [(0, 0)], 1, 4)),
        ("play_against_zoo: the same, LSTM table with cross_family", lambda: M.play_against_zoo(ok, lt, wide, [(0, 0)], 1, 4, cross_family=True)),
        ("play_against_zoo: zoo row past the table", lambda: M.play_against_zoo(ok, mt, zoo, [(0, 2)], 1, 4)),
        ("play_against_zoo: empty checkpoint row", lambda: M.play_against_zoo(ok, mt, zl, [(3, 0)], 1, 4)),
        ("play_against_zoo: empty checkpoint row, LSTM table with cross_family", lambda: M.play_against_zoo(ok, lt, zoo, [(2, 0)], 1, 4, cross_family=True)),
        ("play_against_zoo: chunk 0", lambda: M.play_against_zoo(ok, mt, zoo, [(0, 0)], 1, 4, chunk=0)),
        ("play_against_zoo: rne_post, then LSTM table against zoo MLP nets", lambda: M.play_against_zoo(rne, lt, zoo, [(0, 0)], 1, 4)),
        ("play_against_zoo: LSTM table against zoo MLP nets, then zoo width", lambda: M.play_against_zoo(ok, lt, wide, [(0, 0)], 1, 4)),
        ("play_against_zoo: zoo width, then zoo row past the table", lambda: M.play_against_zoo(ok, mt, wide, [(0, 2)], 1, 4)),
        ("play_against_zoo: zoo row past the table, then rounds_per_env 0", lambda: M.play_against_zoo(ok, mt, zl, [(0, 2)], 0, 4)),
        ("play_against_zoo: chunk 0, then LSTM(64) fused, cross_family", lambda: M.play_against_zoo(ok, lt64, zoo, [(0, 0)], 1, 4, chunk=0, cross_family=True)),
        ("play_against_zoo: chunk 0, then LSTM(64) fused against zoo LSTM nets", lambda: M.play_against_zoo(ok, lt64, zl, [(0, 0)], 1, 4, chunk=0)),
    ]
    # the version drivers: what they refuse before an env exists
    import joblib

    def no_env(*a, **k):
        raise AssertionError("an env was built")
    M._make_env = no_env
    with tempfile.TemporaryDirectory() as tmp:
        def run_dir(name, plists):
            for v, pl in enumerate(plists):
                path = os.path.join(tmp, name, "checkpoints", "%.5i" % v)
                os.makedirs(os.path.dirname(path), exist_ok=True)
                joblib.dump(pl, path)
            return os.path.join(tmp, name)
        mlp = run_dir("mlp", [[rng.standard_normal(s).astype(np.float32) for s in policies.param_shapes(D, A)] for _ in range(3)])
        lstm, lstm64 = (run_dir("lstm%d" % H, [[rng.standard_normal(s).astype(np.float32) for s in policies.lstm_param_shapes(D, A, H)]
                                               for _ in range(3)]) for H in (128, 64))
        empty = run_dir("empty", [[np.zeros(1, np.float32)]])
        C = M.compare_history_versions
        cases += [
            ("compare_history_versions: MLP against LSTM", lambda: C(mlp, lstm, 4)),
            ("compare_history_versions: LSTM against MLP, cross_family=False", lambda: C(lstm, mlp, 4, cross_family=False)),
            ("compare_history_versions: mixed LSTM widths", lambda: C(lstm, lstm64, 4)),
            ("compare_history_versions: mixed LSTM widths, cross_family", lambda: C(lstm, lstm64, 4, cross_family=True)),
            ("compare_history_versions: MLP against LSTM(64) fused, cross_family", lambda: C(mlp, lstm64, 4, cross_family=True)),
            ("compare_history_versions: LSTM(64) against MLP fused, cross_family", lambda: C(lstm64, mlp, 4, cross_family=True)),
            ("compare_history_versions: MLP against LSTM(64) step by step reaches the env", lambda: C(mlp, lstm64, 4, cross_family=True, fused=False)),
            ("compare_history_versions: MLP against LSTM, cross_family, reaches the env", lambda: C(mlp, lstm, 4, cross_family=True)),
            ("compare_history_versions: LSTM(64) against itself reaches the env (refused by play_matches later)", lambda: C(lstm64, lstm64, 4)),
            ("compare_history_versions: no checkpoints", lambda: C(empty, mlp, 4)),
            ("round_robin: reaches the env", lambda: M.round_robin(lstm, 1, 4)),
            ("round_robin: interval 0", lambda: M.round_robin(lstm, 0, 4)),
            ("evaluate_history_against_zoo: reaches the env", lambda: M.evaluate_history_against_zoo(lstm, [os.path.join(tmp, "x.npy")], 4)),
            ("evaluate_history_against_zoo: no checkpoints", lambda: M.evaluate_history_against_zoo(empty, [], 4, start=5)),
        ]
        for name, call in cases:
            try:
                call()
                print("%s -> no exception" % name)
            except Exception as e:                               # noqa: BLE001 -- the type is what is printed
                print("%s -> %s: %s" % (name, type(e).__name__, str(e).replace(tmp, "<tmp>")))


def gpu_refusals():
    """The host index checks of the step-by-step paths (they sit behind the env's buffers): message text only, no launch."""
    import numpy as np
    import torch
    import test_gpu_matches_cross as X
    from robosumo_selfplay_amd import matches as M
    np.random.seed(16)
    env = X._env(ANT, 16)
    D_, A_ = X._dims(env)
    mt, lt = X._mlp_table(env), X._lstm_table(env)
    zoo, zl = _zoo_tables(env, D_, A_)
    env.reset_device()
    n = env.num_envs
    z, sc = np.zeros(n, np.int32), torch.zeros((n, 3), dtype=torch.int32, device="cuda")
    two, neg = z.copy(), z.copy()
    two[3], neg[5] = 2, -1                                       # row 2: the MLP table has it, the other tables do not
    s256, s128 = (torch.zeros((n, w), dtype=torch.float32, device="cuda") for w in (256, 128))
    three = two + (two > 0)
    for name, call in (
            ("match_steps_stepwise: idx1 past the table", lambda: M.match_steps_stepwise(env, mt, z, three, sc, 1, 1)),
            ("match_steps_stepwise: negative idx0", lambda: M.match_steps_stepwise(env, mt, neg, z, sc, 1, 1)),
            ("match_steps_stepwise_lstm: idx0 past the table", lambda: M.match_steps_stepwise_lstm(env, lt, two, z, (s256, s256.clone()), sc, 1, 1)),
            ("zoo_match_steps_stepwise: idx1 past the zoo table", lambda: M.zoo_match_steps_stepwise(env, mt, zoo, two, two, sc, 1, 1)),
            ("zoo_lstm_match_steps_stepwise: idx1 past the zoo table", lambda: M.zoo_lstm_match_steps_stepwise(env, mt, zl, z, two, s128, sc, 1, 1)),
            ("zoo_lstm_match_steps_stepwise: idx0 past the LSTM table", lambda: M.zoo_lstm_match_steps_stepwise(env, lt, zl, two, z, (s256, s128), sc, 1, 1)),
            ("cross_match_steps_stepwise: LSTM table as agent 0, idx0 past it", lambda: M.cross_match_steps_stepwise(env, mt, lt, 0, two, z, s256, sc, 1, 1)),
            ("cross_match_steps_stepwise: LSTM table as agent 1, idx1 past it", lambda: M.cross_match_steps_stepwise(env, mt, lt, 1, two, two, s256, sc, 1, 1)),
            ("lstm_zoo_match_steps_stepwise: idx1 past the zoo table", lambda: M.lstm_zoo_match_steps_stepwise(env, lt, zoo, z, two, s256, sc, 1, 1))):
        try:
            call()
            print("%s -> no exception" % name)
        except ValueError as e:
            print("%s -> %s: %s" % (name, type(e).__name__, e))
    env.close()


def main(argv):
    if "--refusals" in argv:
        refusals()
        return
    step_functions()
    drivers()
    gpu_refusals()


if __name__ == "__main__":
    main(sys.argv[1:])
