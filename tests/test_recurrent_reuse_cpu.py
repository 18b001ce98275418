"""CPU-side checks of opponent-data reuse for recurrent learners (learn(network='lstm', use_opponent_data=...)): the batch assembly
against a plain-numpy restatement, the float64 masked loss reference (tests/lstm_reuse_ref.py) against the oracle function and against
central finite differences, the refusals, and the declarations / bindings of the four new C entry points."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lstm_reuse_ref as R
from oracle import ppo_oracle as po
from robosumo_selfplay_amd import alg_ppo, build, capi, lstm_model, ppo_capi, runner, vec_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = 50.0


def _rollout(seed=0, nenv=3, T=4, D=5, A=2, H=4):
    """A fake rollout in the Runner's return layout: [2, nenv * T, ...] env-major.  Agent 1's neglogp: some entries at the threshold
    (invalid: the rule is ``<``), some above, one NaN."""
    rng = np.random.default_rng(seed)
    rows = nenv * T
    a = dict(obs=rng.normal(0, 1, (2, rows, D)).astype(np.float32), returns=rng.normal(0, 1, (2, rows)).astype(np.float32),
             masks=rng.random((2, rows)) < 0.3, actions=rng.normal(0, 1, (2, rows, A)).astype(np.float32),
             values=rng.normal(0, 1, (2, rows)).astype(np.float32), neglogpacs=rng.normal(10, 2, (2, rows)).astype(np.float32),
             rewards=rng.normal(0, 1, (2, rows)).astype(np.float32))
    a["neglogpacs"][1, [1, 6]] = THR            # exactly at the threshold: invalid
    a["neglogpacs"][1, [2, 9]] = THR + 7.0
    a["neglogpacs"][1, 4] = np.nan
    a["neglogpacs"][0, 3] = THR + 1.0           # agent 0's rows are never masked
    a["off_policy_ratio"] = rng.uniform(0, 1, rows).astype(np.float32)
    a["total_ratio"] = rng.uniform(0, 1, rows).astype(np.float32)
    a["states0"] = rng.normal(0, 1, (nenv, 2 * H)).astype(np.float32)
    a["shadow0"] = rng.normal(0, 1, (nenv, 2 * H)).astype(np.float32)
    return a, nenv, T


ORDER = ("obs", "returns", "masks", "actions", "values", "neglogpacs", "rewards", "off_policy_ratio", "total_ratio", "states0", "shadow0")


@pytest.mark.parametrize("mode", ["direct", "off_policy", "both"])
@pytest.mark.parametrize("vgap,gap", [(None, None), (5, 3), (5, 9)])
def test_assemble_recurrent_update_batch_matches_numpy(mode, vgap, gap):
    import torch
    a, nenv, T = _rollout()
    kw = dict(nenv=nenv, neglogp_threshold=THR, use_opponent_data=mode, vgap=vgap, version_gap=gap)
    want = R.recurrent_update_batch(*[a[k] for k in ORDER], **kw)
    got = alg_ppo.assemble_recurrent_update_batch(*[torch.from_numpy(a[k]) for k in ORDER], **kw)
    use_opp = not (vgap is not None and gap > vgap)
    assert got["nseq"] == want["nseq"] == (2 * nenv if use_opp else nenv)
    for k in ("obs", "returns", "masks", "actions", "values", "neglogpacs", "rewards", "states", "valid", "weights", "usable_index"):
        g = got[k].numpy()
        assert g.shape == want[k].shape and np.array_equal(g, want[k], equal_nan=g.dtype.kind == "f"), k
    assert got["useful_ratio"] == want["useful_ratio"] == 7.0 / 12.0
    rows = nenv * T
    # sequence order and start states: agent 0's sequences first, each with its own state; agent 1's follow from the shadow state
    assert np.array_equal(got["obs"][:rows].numpy(), a["obs"][0]) and np.array_equal(got["states"][:nenv].numpy(), a["states0"])
    assert (got["valid"][:rows] == 1).all() and (got["weights"][:rows] == 1).all()
    if use_opp:
        assert np.array_equal(got["obs"][rows:].numpy(), a["obs"][1]) and np.array_equal(got["states"][nenv:].numpy(), a["shadow0"])
        assert np.array_equal(got["masks"][rows:].numpy(), a["masks"][1])
        v1 = got["valid"][rows:].numpy()
        assert np.array_equal(np.nonzero(v1 == 0)[0], [1, 2, 4, 6, 9])                    # at the threshold, above it, NaN
        w1 = got["weights"][rows:].numpy()
        src = {"direct": np.ones(rows, np.float32), "off_policy": a["off_policy_ratio"], "both": a["total_ratio"]}[mode]
        assert np.array_equal(w1, np.where(v1 == 1, src, np.float32(0)))
    else:
        assert got["obs"].shape[0] == rows


def test_assemble_recurrent_update_batch_refuses_an_unknown_mode():
    import torch
    a, nenv, T = _rollout()
    with pytest.raises(ValueError):
        alg_ppo.assemble_recurrent_update_batch(*[torch.from_numpy(a[k]) for k in ORDER], nenv=nenv, neglogp_threshold=THR,
                                                use_opponent_data="sideways")


# ---- the float64 masked reference ------------------------------------------------------------------------------------------------
def _case(seed=0, T=5, n=4, D=6, A=3, H=8):
    rng = np.random.default_rng(seed)
    params = [rng.normal(0, 0.4, s) for s in [(D, 4 * H), (H, 4 * H), (4 * H,), (H, A), (A,), (1, A), (H, 1), (1,)]]
    params[5] = rng.normal(-0.3, 0.1, (1, A))
    obs = rng.normal(0, 1, (T, n, D))
    masks = (rng.random((T, n)) < 0.25).astype(np.float64)
    actions = rng.normal(0, 0.7, (T, n, A))
    advs = rng.normal(0, 1, (T, n))
    returns = rng.normal(0, 1, (T, n))
    S0 = rng.normal(0, 0.5, (n, 2 * H))
    w = rng.uniform(0.5, 1.5, (T, n))
    old = np.zeros((T, n))
    state = S0.copy()
    f32 = lambda x: x.astype(np.float32)
    for t in range(T):
        hh, state = po.lstm_step_baselines(f32(params[0]), f32(params[1]), f32(params[2]), f32(obs[t]), f32(state), f32(masks[t]))
        old[t] = po.neglogp(hh @ params[3] + params[4], params[5], actions[t])
    old = old + rng.normal(0, 0.25, (T, n))          # ratios straddle the clip range
    return params, obs, masks, actions, advs, returns, old, w, S0, rng


def test_masked_reference_with_every_row_valid_is_the_oracle():
    params, obs, masks, actions, advs, returns, old, w, S0, rng = _case()
    T, n = masks.shape
    want = po.lstm_ppo_loss_and_grads(params, obs, masks, actions, advs, returns, old, w, S0, 0.2, 0.01, 0.5)
    got = R.masked_loss_and_grads(params, obs, masks, actions, advs, returns, old, w, np.ones((T, n)), S0, 0.2, 0.01, 0.5)
    assert got[4] == T * n
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3])
    for a, b in zip(got[2], want[2]):
        assert np.array_equal(a, b)


def test_masked_reference_matches_finite_differences():
    """Step and tolerance of tests/test_lstm_oracle.py.  Sequence 2 has no valid row; the invalid rows hold NaN in every per-row
    input, which must reach nothing."""
    params, obs, masks, actions, advs, returns, old, w, S0, rng = _case()
    T, n = masks.shape
    valid = (rng.random((T, n)) < 0.6).astype(np.float64)
    valid[:, 2] = 0.0
    valid[0, 0], valid[1, 0] = 1.0, 0.0
    bad = valid == 0
    advs, returns, old, w = (np.where(bad, np.nan, x) for x in (advs, returns, old, w))
    f = lambda p: R.masked_loss_and_grads(p, obs, masks, actions, advs, returns, old, w, valid, S0, 0.2, 0.01, 0.5)
    loss, stats, grads, _, cnt = f(params)
    assert cnt == int(valid.sum()) and 0 < cnt < T * n
    assert np.isfinite(loss) and np.isfinite(stats).all() and 0.0 < stats[4] < 1.0
    assert all(np.isfinite(g).all() for g in grads)
    eps = 1e-6
    for k, (p, g) in enumerate(zip(params, grads)):
        flat = p.ravel()
        for j in rng.choice(flat.size, size=min(6, flat.size), replace=False):
            orig = flat[j]
            flat[j] = orig + eps; lp = f(params)[0]
            flat[j] = orig - eps; lm = f(params)[0]
            flat[j] = orig
            fd = (lp - lm) / (2 * eps)
            assert abs(fd - np.ravel(g)[j]) < 1e-6 * (1 + abs(fd)), (k, j, fd, np.ravel(g)[j])
    # no valid row at all (ent_coef 0): zero loss, zero gradient
    none = R.masked_loss_and_grads(params, obs, masks, actions, advs, returns, old, w, np.zeros((T, n)), S0, 0.2, 0.0, 0.5)
    assert none[4] == 0 and none[0] == 0.0 and all(not g.any() for g in none[2])


def test_masked_advantage_normalisation_reference():
    rng = np.random.default_rng(3)
    r, v = rng.normal(0, 1, 40).astype(np.float32), rng.normal(0, 1, 40).astype(np.float32)
    ones = R.masked_normalize_advantages(r, v, np.ones(40))
    assert np.allclose(ones, po.normalize_advantages(r, v), rtol=1e-5, atol=1e-6)
    valid = rng.random(40) < 0.5
    got = R.masked_normalize_advantages(r, v, valid)
    assert (got[~valid] == 0).all() and np.allclose(got[valid], po.normalize_advantages(r[valid], v[valid]), rtol=1e-5, atol=1e-6)
    assert not R.masked_normalize_advantages(r, v, np.zeros(40)).any()


# ---- refusals, before anything touches a GPU ------------------------------------------------------------------------------------
def test_recurrent_reuse_refusals():
    alg_ppo.check_recurrent_reuse("latest", None)                     # the supported case passes
    alg_ppo.check_recurrent_reuse("ours", None, device_mode=True)
    with pytest.raises(NotImplementedError, match="fix"):
        alg_ppo.check_recurrent_reuse("fix", None)
    with pytest.raises(NotImplementedError, match="single GPU"):
        alg_ppo.check_recurrent_reuse("latest", object())
    with pytest.raises(NotImplementedError, match="device-mode"):
        alg_ppo.check_recurrent_reuse("latest", None, device_mode=False)


class _NoEnv(object):          # learn() reads these before it builds a model; a refusal comes before any of it reaches a device
    num_envs = 4

    class _Sp(object):
        shape = (121,)
    observation_space = [_Sp(), _Sp()]

    class _Ac(object):
        shape = (8,)
    action_space = [_Ac(), _Ac()]


@pytest.mark.parametrize("kw,exc,msg", [(dict(opponent_mode="fix"), NotImplementedError, "opponent_mode='fix'"),
                                        (dict(use_opponent_data="sideways"), ValueError, None)])
def test_learn_refuses_before_the_first_rollout(kw, exc, msg):
    args = dict(network="lstm", env=_NoEnv(), total_timesteps=64, nagent=2, nsteps=4, nminibatches=2, use_opponent_data="direct",
                opponent_mode="latest", verbose=False)
    args.update(kw)
    with pytest.raises(exc, match=msg):          # the message of check_recurrent_reuse, not the blanket refusal it replaced
        alg_ppo.learn(**args)


# ---- declarations and bindings ---------------------------------------------------------------------------------------------------
NEW_PPO = ("ppo_adv_moments_masked_ws", "ppo_adv_normalize_masked", "ppo_lstm_head_grad_masked")


def test_headers_declare_the_new_entry_points():
    with open(os.path.join(ROOT, "include", "sumo_ppo.h")) as f:
        hp = f.read()
    for n in NEW_PPO:
        m = re.search(r"\bint %s\(([^;]*)\);" % n, hp)
        assert m and "const float* valid" in " ".join(m.group(1).split()), n
    args = " ".join(re.search(r"\bint ppo_lstm_head_grad_masked\(([^;]*)\);", hp).group(1).split())
    assert "const double* count_dev" in args and "inv_count" not in args
    with open(os.path.join(ROOT, "include", "sumo_hip.h")) as f:
        hh = f.read()
    m = re.search(r"\bint sumo_rollout_steps_lstm_reuse\(([^;]*)\);", hh)
    assert m and " ".join(m.group(1).split()).startswith("sumo_handle_t h, const sumo_rollout_lstm_reuse* r, float* actions_dev")
    assert re.search(r"typedef struct sumo_rollout_lstm_reuse \{[^}]*float\* state2;[^}]*\} sumo_rollout_lstm_reuse;", hh)


def test_bindings_list_the_new_entry_points():
    for n in NEW_PPO:
        assert n in ppo_capi.EXPORTS, n
    assert "sumo_rollout_steps_lstm_reuse" in capi.EXPORTS
    assert callable(getattr(capi.Engine, "rollout_steps_lstm_reuse", None))
    assert callable(getattr(vec_env.SumoVecEnv, "rollout_steps_lstm_reuse_group", None))
    la = runner.rollout_launch("lstm", "self", None, True)      # what the Runner launches under ``reuse_opponent``
    assert (la.entry, la.struct) == ("rollout_steps_lstm_reuse_group", "RolloutLstmReuse")
    assert "reuse" in runner.RolloutMode._fields
    for name in ("rollout_mode", "fused_steps", "_steps_fused_lstm"):
        assert callable(getattr(runner.Runner, name, None)), name
    assert callable(getattr(lstm_model.LstmPPOModel, "score_value_advance", None))
    build.build_all()
    L = C.CDLL(build.lib_path("libsumo_ppo.so"))
    for n in NEW_PPO:
        assert hasattr(L, n), n
    assert hasattr(C.CDLL(build.lib_path("libsumo_hip.so")), "sumo_rollout_steps_lstm_reuse")


def test_reuse_launch_struct_mirror_matches_the_header(tmp_path):
    """capi.RolloutLstmReuse lists the fields flat; the header nests sumo_rollout_lstm and appends state2: same layout."""
    names = [f[0] for f in capi.RolloutLstmReuse._fields_]
    assert names[:-1] == [f[0] for f in capi.RolloutLstm._fields_] and names[-1] == "state2"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sumo_hip.h"', 'int main(void) {',
             '  printf("%zu %zu %zu %zu\\n", sizeof(sumo_rollout_lstm_reuse), offsetof(sumo_rollout_lstm_reuse, state2), '
             'offsetof(sumo_rollout_lstm_reuse, ro), sizeof(sumo_rollout_lstm));', '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    size, off2, off0, base = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert (C.sizeof(capi.RolloutLstmReuse), capi.RolloutLstmReuse.state2.offset) == (size, off2)
    assert off0 == 0 and off2 == base == C.sizeof(capi.RolloutLstm)
