"""Host side of the fused 'ours' opponent selector: the normalisation tail, what ``learn(fused_selector=True)`` refuses before it
touches the env or the device, the command-line flag, and the static code-object check of the rebuilt PPO library."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import ppo_oracle
from robosumo_selfplay_amd import alg_ppo, build, codegen_check, ppo_capi
from robosumo_selfplay_amd.policy_selector import selection_probs_from_scores


def test_selection_probs_from_scores_normalises_like_the_oracle():
    rng = np.random.default_rng(0)
    ap = rng.uniform(5.0, 15.0, 200)                     # float64 throughout: only the normalisation is compared here
    naps = ap[None, :] * (1.0 + rng.normal(0.0, [[0.01], [0.1], [0.3], [0.03]], (4, 200)))
    scores = np.array([np.abs(nap / ap - 1.0).mean() for nap in naps])
    got = selection_probs_from_scores(scores)
    np.testing.assert_allclose(got, ppo_oracle.opponent_selection_probs(ap, naps), rtol=1e-12)
    assert got.sum() == pytest.approx(1.0, abs=1e-12)
    np.testing.assert_allclose(selection_probs_from_scores([1.0, 3.0]), [0.25, 0.75], rtol=1e-15)


@pytest.mark.parametrize("scores", [[0.0, 0.0, 0.0], [np.nan, 1.0, 2.0], [np.inf, 1.0, 2.0], [1.0, -1.0, 0.0], [0.0]])
def test_selection_probs_from_scores_falls_back_to_uniform(scores):
    got = selection_probs_from_scores(scores)
    assert np.array_equal(got, np.full(len(scores), 1.0 / len(scores)))


def test_selection_probs_keeps_its_results():
    """``alg_ppo.selection_probs`` now ends in the shared tail: same probabilities as before, the uniform fall-back included."""
    import torch
    ap = torch.tensor([10.0, 8.0, 0.0, 12.0])
    naps = [torch.tensor([11.0, 8.0, 1.0, 12.0]), torch.tensor([10.0, 10.0, 0.0, 9.0])]
    want = np.array([np.mean([0.1, 0.0, 0.0]), np.mean([0.0, 0.25, 0.25])])        # row 2 (ap == 0) is inf / NaN: left out
    np.testing.assert_allclose(alg_ppo.selection_probs(ap, naps), want / want.sum(), rtol=1e-6)
    assert np.array_equal(alg_ppo.selection_probs(ap, [ap, ap]), [0.5, 0.5])


@pytest.mark.parametrize("kw,match", [(dict(network="lstm"), "lstm"), (dict(opponent_mode="random"), "ours"),
                                      (dict(opponent_mode="fix"), "ours"), (dict(model_fn=lambda **kw: None), "params")])
def test_learn_refuses_fused_selector_before_touching_the_env(kw, match):
    args = dict(network="mlp", env=None, total_timesteps=10, fused_selector=True)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        alg_ppo.learn(**args)


def test_run_parser_accepts_fused_selector():
    sys.path.insert(0, ROOT)
    import run
    args, unknown = run.build_parser().parse_known_args(["--env", "RoboSumo-Ant-vs-Ant-v0", "--fused_selector", "--nsteps=128"])
    assert args.fused_selector is True and unknown == ["--nsteps=128"]
    assert run.build_parser().parse_known_args([])[0].fused_selector is False


def test_run_parser_accepts_selector_table_mb():
    sys.path.insert(0, ROOT)
    import run
    assert run.build_parser().parse_known_args(["--fused_selector", "--selector_table_mb", "64"])[0].selector_table_mb == 64.0
    assert run.build_parser().parse_known_args(["--fused_selector"])[0].selector_table_mb is None      # learn()'s default of 1024 holds


def test_binding_declares_the_selector_entry_points():
    assert {"ppo_selection_scores", "ppo_selection_scores_workspace_bytes"} <= set(ppo_capi.EXPORTS)
    build.build_all()
    L = ppo_capi.lib()
    # 1024 slots x 32 candidates x (float64 sum + int32 count) + the arrival counter's 16 bytes
    assert L.ppo_selection_scores_workspace_bytes() == 1024 * 32 * 12 + 16


def test_codegen_check_passes_on_the_rebuilt_library():
    build.build_all()
    lib = build.lib_path("libsumo_ppo.so")
    assert os.path.exists(lib)
    assert codegen_check.scan_library(lib) == {}
