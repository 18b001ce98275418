"""ppo_selection_scores / policy_selector.FusedSelector on the GPU: every candidate of the 'ours' opponent selector scored in one
launch, against the per-candidate path it replaces (``PolicyWithValue.action_probability`` + ``alg_ppo.selection_probs``)."""
import os

import numpy as np
import pytest

from conftest import has_gpu

pytestmark = pytest.mark.gpu
if has_gpu():
    import torch
    from oracle import ppo_oracle
    from robosumo_selfplay_amd import policies, ppo_capi
    from robosumo_selfplay_amd.model import PPOModel
    from robosumo_selfplay_amd.policy_selector import FusedSelector, selection_probs_from_scores
    from robosumo_selfplay_amd.vec_env import SumoVecEnv
    DEV = torch.device("cuda", 0)

A = 8
TABLE_ROWS = 40
# non-monotone subsets of the 40 table rows, each with a repeated row
CAND_ROWS = {1: [17], 5: [31, 4, 22, 4, 9],
             32: [39, 0, 13, 27, 5, 33, 21, 8, 36, 2, 19, 30, 11, 25, 7, 38, 16, 1, 29, 13, 23, 35, 6, 18, 32, 10, 26, 3, 37, 15, 24, 12]}
_CASES = {}


def _spec(D):
    return policies.PolicySpec(D, A, value_network="copy", activation="relu")


def _neglogp(spec, vec, obs, act):
    """What the per-candidate path computes: ``action_probability`` of one parameter vector (a ppo_forward launch)."""
    pol = policies.PolicyWithValue(spec, torch.from_numpy(np.ascontiguousarray(vec, np.float32)).to(DEV), DEV)
    return pol.action_probability(obs, given_action=act)


def _case(D, n):
    """Reference net, a filled 40-row table (rows perturbed from the reference by 1e-3 .. 1e-1), data, and the reference neglogps
    [1 + 40][n] from the per-candidate path -- computed once per (D, n) and left unchanged."""
    if (D, n) not in _CASES:
        rng = np.random.RandomState(100 * D + n)
        spec = _spec(D)
        ref = policies.flatten_params(policies.init_param_list(D, A, rng=rng))
        eps = np.logspace(-3, -1, TABLE_ROWS)
        rows = [(ref + eps[k] * rng.standard_normal(ref.size)).astype(np.float32) for k in range(TABLE_ROWS)]
        sel = FusedSelector(spec, DEV, TABLE_ROWS)
        assert not sel.staging and sel.capacity == TABLE_ROWS
        for k, v in enumerate(rows):
            sel.table.set(k, v)
        obs = torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32)).to(DEV)
        act = torch.from_numpy((0.5 * rng.standard_normal((n, A))).astype(np.float32)).to(DEV)
        want = torch.stack([_neglogp(spec, v, obs, act) for v in [ref] + rows])
        _CASES[(D, n)] = dict(spec=spec, ref=torch.from_numpy(ref).to(DEV), ref_np=ref, rows=rows, sel=sel, obs=obs, act=act, want=want)
    return _CASES[(D, n)]


def _expected_sums(nl, keep=None):
    """float64 sums and counts of |nap / ap - 1| (float32 per row, non-finite rows masked) from neglogps nl [1 + k][n]."""
    with np.errstate(all="ignore"):
        r = np.abs(nl[1:] / nl[0] - np.float32(1.0))
    assert r.dtype == np.float32
    ok = np.isfinite(r)
    if keep is not None:
        ok &= keep[None, :]
    return np.where(ok, r, 0).astype(np.float64).sum(axis=1), ok.sum(axis=1).astype(np.int32)


def _bits(x):
    return x.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32)


@pytest.mark.parametrize("D,n,max_blocks", [(121, 1, 0), (121, 53, 0), (121, 16 * 9 + 3, 1), (121, 16 * 9 + 3, 2),
                                            (37, 1, 0), (37, 53, 0), (37, 16 * 9 + 3, 1), (37, 16 * 9 + 3, 2)])
def test_scores_match_the_per_candidate_path(D, n, max_blocks):
    c = _case(D, n)
    sel = c["sel"]
    for ncand, rows in CAND_ROWS.items():
        dbg = torch.full((ncand + 1, n), -1.0, dtype=torch.float32, device=DEV)
        scores = sel.scores(c["ref"], rows, c["obs"], c["act"], max_blocks=max_blocks, neglogp_dbg=dbg)
        # per-row parity: the same tile code as ppo_forward, compared as bit patterns
        want = c["want"][[0] + [r + 1 for r in rows]]
        assert np.array_equal(_bits(dbg), _bits(want)), (ncand, "neglogp differs from action_probability")
        # sums: the same float32 terms, only the float64 summation order may differ (n * 2^-53 << 1e-9)
        nl = dbg.cpu().numpy()
        assert np.isfinite(nl).all()
        esum, ecnt = _expected_sums(nl)
        gsum, gcnt = sel.score_sum[:ncand].cpu().numpy(), sel.finite_count[:ncand].cpu().numpy()
        print("D %d n %d ncand %d blocks %d: max rel sum err %.3g" % (D, n, ncand, max_blocks, np.max(np.abs(gsum - esum) / esum)))
        assert np.array_equal(gcnt, ecnt) and (ecnt == n).all()
        np.testing.assert_allclose(gsum, esum, rtol=1e-9, atol=0)
        np.testing.assert_allclose(scores, esum / ecnt, rtol=1e-9, atol=0)
        np.testing.assert_allclose(selection_probs_from_scores(scores), ppo_oracle.opponent_selection_probs(nl[0], nl[1:]), rtol=0, atol=1e-6)


def test_non_finite_rows_are_left_out():
    D, n = 121, 53
    c = _case(D, n)
    spec, obs, act = c["spec"], c["obs"], c["act"]
    sel = FusedSelector(spec, DEV, 3)
    sharp = c["rows"][7].copy()
    P = sharp.size
    sharp[P - 1 - policies.HIDDEN - A:P - 1 - policies.HIDDEN] = -60.0          # pi/logstd: the neglogp overflows to inf on every row
    for k, v in enumerate((c["rows"][3], sharp, c["rows"][12])):
        sel.table.set(k, v)
    dbg = torch.empty((4, n), dtype=torch.float32, device=DEV)
    scores = sel.scores(c["ref"], [0, 1, 2], obs, act, neglogp_dbg=dbg)
    nl = dbg.cpu().numpy()
    assert np.isinf(nl[2]).all()
    cnt = sel.finite_count[:3].cpu().numpy()
    assert list(cnt) == [n, 0, n] and scores[1] == 0.0
    both = sel.score_sum[:3].cpu().numpy()
    alone = sel.scores(c["ref"], [0, 2], obs, act)                               # the other candidates are unaffected
    assert np.array_equal(sel.score_sum[:2].cpu().numpy(), both[[0, 2]]) and np.array_equal(alone, scores[[0, 2]])
    # one observation row holds a NaN: that row is left out for every candidate, the other rows' terms are unchanged
    bad = 20
    obs_nan = obs.clone()
    obs_nan[bad, 5] = float("nan")
    sel.scores(c["ref"], [0, 1, 2], obs_nan, act)
    cnt = sel.finite_count[:3].cpu().numpy()
    gsum = sel.score_sum[:3].cpu().numpy()
    keep = np.arange(n) != bad
    esum, ecnt = _expected_sums(nl, keep)
    print("NaN row: counts", cnt, "expected", ecnt, "sums", gsum, "expected", esum)
    assert list(cnt) == [n - 1, 0, n - 1] and np.array_equal(cnt, ecnt)
    np.testing.assert_allclose(gsum[[0, 2]], esum[[0, 2]], rtol=1e-9, atol=0)
    assert gsum[1] == 0.0


def test_candidates_equal_to_the_reference_give_uniform():
    c = _case(121, 53)
    sel = FusedSelector(c["spec"], DEV, 5)
    for k in range(5):
        sel.table.set(k, c["ref_np"])
    scores = sel.scores(c["ref"], [0, 1, 2, 3, 4], c["obs"], c["act"])
    assert scores.dtype == np.float64 and (scores == 0.0).all()
    assert (sel.finite_count[:5].cpu().numpy() == 53).all()
    assert np.array_equal(selection_probs_from_scores(scores), np.full(5, 0.2))


def test_deterministic_across_launches_and_grids():
    c = _case(121, 16 * 9 + 3)
    sel, rows = c["sel"], CAND_ROWS[32]
    sums = {}
    for mb in (1, 2, 0):
        sel.launch(c["ref"], rows, c["obs"], c["act"], max_blocks=mb)
        first = sel.score_sum.clone()
        sel.launch(c["ref"], rows, c["obs"], c["act"], max_blocks=mb)
        assert np.array_equal(_bits(first.view(torch.float32)), _bits(sel.score_sum.view(torch.float32))), mb
        sums[mb] = first.cpu().numpy()
    np.testing.assert_allclose(sums[1], sums[2], rtol=1e-12, atol=0)
    np.testing.assert_allclose(sums[1], sums[0], rtol=1e-12, atol=0)


@pytest.mark.parametrize("ncand", [0, 33])
def test_argument_errors_launch_nothing(ncand):
    c = _case(121, 53)
    sel = c["sel"]
    out_s = torch.full((40,), -7.0, dtype=torch.float64, device=DEV)
    out_c = torch.full((40,), -7, dtype=torch.int32, device=DEV)
    rows = torch.zeros(40, dtype=torch.int32, device=DEV)
    with pytest.raises(ppo_capi.PpoHipError, match="ncand"):
        ppo_capi.chk(ppo_capi.lib().ppo_selection_scores(
            c["ref"].data_ptr(), sel.table.params.data_ptr(), sel.table.params.stride(0), rows.data_ptr(), ncand, c["obs"].data_ptr(), 53,
            c["obs"].stride(0), 121, A, c["act"].data_ptr(), out_s.data_ptr(), out_c.data_ptr(), None, 0, sel.workspace.data_ptr(), None))
    torch.cuda.synchronize()
    assert (out_s == -7.0).all() and (out_c == -7).all()
    with pytest.raises(ValueError, match="candidates"):
        sel.scores(c["ref"], list(range(ncand)), c["obs"], c["act"])


def test_fused_selector_rows_from_models_and_files(tmp_path):
    c = _case(121, 53)
    spec, obs, act = c["spec"], c["obs"], c["act"]
    np.random.seed(4)
    model = PPOModel(policy=spec, trainable=False)
    paths = []
    for k in (3, 20, 33):
        model.params.copy_(torch.from_numpy(c["rows"][k]))
        paths.append(os.path.join(str(tmp_path), "%.5i" % len(paths)))
        model.save(paths[-1])
    # note_saved (device to device) == set from the saved file
    a, b = FusedSelector(spec, DEV, 3), FusedSelector(spec, DEV, 3)
    assert a.note_saved(2, model, paths[2]) and list(a.filled) == [False, False, True]
    b.table.set(2, paths[2])
    sa, sb = a.scores(c["ref"], [2], obs, act), b.scores(c["ref"], [2], obs, act)
    assert np.array_equal(sa.view(np.uint64), sb.view(np.uint64)) and sa[0] > 0
    assert not a.note_saved(3, model, paths[2])                      # past the table's end: left to ensure()
    with pytest.raises(ValueError, match="not filled"):
        a.scores(c["ref"], [0, 2], obs, act)
    # ensure fills only the missing rows
    seen = []
    orig = a.table.set
    a.table.set = lambda k, src, label=None: (seen.append(k), orig(k, src, label))[1]
    assert a.ensure(paths, [0, 1, 2]) == 2 and seen == [0, 1] and a.filled.all()
    assert a.ensure(paths, [2, 0]) == 0 and seen == [0, 1]
    hist = a.scores(c["ref"], [2, 0, 1], obs, act)
    np.testing.assert_array_equal(hist, c["sel"].scores(c["ref"], [33, 3, 20], obs, act))
    # the 32-row staging mode (forced by a tiny table budget) gives the same scores
    s = FusedSelector(spec, DEV, 3, table_mb=0.01)
    assert s.staging and s.capacity == 32 and not s.note_saved(0, model, paths[0])
    with pytest.raises(ValueError, match="staging"):
        s.scores(c["ref"], [2, 0, 1], obs, act)
    assert s.ensure(paths, [2, 0, 1]) == 3
    np.testing.assert_array_equal(s.scores(c["ref"], [2, 0, 1], obs, act), hist)


def test_learn_with_fused_selector_matches_the_per_candidate_selector(tmp_path, monkeypatch):
    """Two short runs from the same seed, the selector per candidate and fused.  At update 2 -- the first selection, both runs still
    in the same state -- the probability vectors agree; the fused run goes on to choose an opponent in every update."""
    from robosumo_selfplay_amd import alg_ppo
    probs = {False: [], True: []}
    orig_probs, orig_scores = alg_ppo.selection_probs, FusedSelector.scores

    def spy_probs(ap, naps):
        out = orig_probs(ap, naps)
        probs[False].append(np.array(out))
        return out

    def spy_scores(self, *a, **kw):
        out = orig_scores(self, *a, **kw)
        probs[True].append(selection_probs_from_scores(out))
        return out
    monkeypatch.setattr(alg_ppo, "selection_probs", spy_probs)
    monkeypatch.setattr(FusedSelector, "scores", spy_scores)
    hist = {}
    for fused in (False, True):
        env = SumoVecEnv("RoboSumo-Ant-vs-Ant-v0", num_envs=32, seed=1)
        model = alg_ppo.learn(network="mlp", env=env, seed=1, total_timesteps=32 * 8 * 4, nagent=2, log_dir=os.path.join(str(tmp_path), str(fused)),
                              verbose=False, nsteps=8, nminibatches=2, noptepochs=1, opponent_mode="ours", value_network="copy", num_hidden=64,
                              activation="relu", fused_selector=fused)
        hist[fused] = model.history
        env.close()
    assert len(probs[False]) == 3 and len(probs[True]) == 3          # updates 2, 3, 4
    print("update 2 probabilities: per candidate", probs[False][0], "fused", probs[True][0])
    assert probs[True][0].shape == (2,) and np.isfinite(probs[True][0]).all()
    np.testing.assert_allclose(probs[True][0], probs[False][0], rtol=0, atol=1e-6)
    versions = hist[True]["opponent_versions"]
    assert len(versions) == 4
    for update, chosen in enumerate(versions, start=1):
        assert len(chosen) == 1 and all(0 <= v < update for v in chosen)
    assert len(hist[True]["lossvals"]) == 4 and all(np.isfinite(l).all() for l in hist[True]["lossvals"])
