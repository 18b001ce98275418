#!/usr/bin/env python3
"""Time of the 'ours' opponent selector per update (alg_ppo.learn, opponent_mode='ours'): --rows opponent samples (default 4096 envs
x 128 steps), --candidates saved checkpoints plus the reference opponent, MLP(64,64) on Ant-vs-Ant's 121 / 8 dimensions.

Three ways to the same probabilities, each timed as the median of --runs runs after --warmup runs, with a device synchronisation on
both sides of every run (wall clock, everything included: file reads, copies, launches, the host read-back):

  per_candidate   what learn() does without fused_selector: per candidate ``model.load`` (joblib read + host-to-device copy),
                  ``action_probability`` (one ppo_forward launch over the whole batch), then ``alg_ppo.selection_probs``
  fused_history   ``FusedSelector`` whose table holds the run's checkpoints: ``ensure`` (nothing to read) + one launch + one copy
  fused_staging   ``FusedSelector`` with the 32-row staging table: the sampled files are read again every update, then one launch

Prints ONE JSON line; the largest difference between the three probability vectors is part of it.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def timed(fn, warmup, runs, sync):
    out = None
    for _ in range(warmup):
        out = fn()
    ts = []
    for _ in range(runs):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return out, 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts)), 1e3 * float(np.max(ts))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096 * 128)
    ap.add_argument("--candidates", type=int, default=30)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    if not (1 <= args.candidates <= 32 and args.rows >= 1 and args.runs >= 10 and args.warmup >= 1):
        raise SystemExit("--candidates 1..32, --rows >= 1, --runs >= 10, --warmup >= 1")
    import torch
    from robosumo_selfplay_amd import alg_ppo, policies
    from robosumo_selfplay_amd.model import PPOModel
    from robosumo_selfplay_amd.policy_selector import FusedSelector, selection_probs_from_scores
    D, A, K = 121, 8, args.candidates
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    spec = policies.PolicySpec(D, A, value_network="copy", activation="relu")
    np.random.seed(args.seed)
    ref = PPOModel(policy=spec, trainable=False)
    util = PPOModel(policy=spec, trainable=False)
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    obs = torch.randn((args.rows, D), generator=gen, device=dev, dtype=torch.float32)
    act = 0.5 * torch.randn((args.rows, A), generator=gen, device=dev, dtype=torch.float32)
    rows = list(range(K))
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for k in range(K):           # the run's history: the reference drifting away, as successive checkpoints do
            util.params.copy_(ref.params + 1e-3 * (k + 1) * torch.randn(ref.params.shape, generator=gen, device=dev))
            paths.append(os.path.join(d, "%.5i" % k))
            util.save(paths[-1])

        def per_candidate():
            ap_ = ref.act_model.action_probability(obs, given_action=act)
            naps = []
            for i in rows:
                util.load(paths[i])
                naps.append(util.act_model.action_probability(obs, given_action=act))
            return alg_ppo.selection_probs(ap_, naps)

        hist = FusedSelector(spec, dev, K)
        for k in range(K):
            util.load(paths[k])
            hist.note_saved(k, util, paths[k])
        stag = FusedSelector(spec, dev, K, table_mb=0.01)
        assert not hist.staging and stag.staging

        def fused(sel):
            def run():
                sel.ensure(paths, rows)
                return selection_probs_from_scores(sel.scores(ref.params, rows, obs, act))
            return run

        res = dict(per_candidate=timed(per_candidate, args.warmup, args.runs, sync), fused_history=timed(fused(hist), args.warmup, args.runs, sync),
                   fused_staging=timed(fused(stag), args.warmup, args.runs, sync))
    base = res["per_candidate"][0]
    out = dict(metric="selector_ms_per_update", rows=args.rows, candidates=K, runs=args.runs, warmup=args.warmup, ob_dim=D, ac_dim=A,
               device=torch.cuda.get_device_name(0))
    for name, (p, med, lo, hi) in res.items():
        out[name + "_ms"] = dict(median=med, min=lo, max=hi)
        out[name + "_max_prob_diff"] = float(np.max(np.abs(p - base)))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
