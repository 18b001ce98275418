#!/usr/bin/env python3
"""Time of a rollout of an MLP learner on a mixed match-up (robosumo_selfplay_amd/mixed.py ``MixedRunner.run``): the one-launch step
(``fused=True``, ``ppo_mixed_step``) against its definition (``fused=False``: ``ppo_forward``, the step-by-step seat launches and the
torch copies of record and action buffer).

RoboSumo-Ant-vs-Bug-v0, --num_env (default 4096) envs, T = --nsteps (default 32), a seat of one zoo MLP and one zoo LSTM bug net
(tests/golden/zoo_v3_params.npz).  Two runners on two env sets of equal seeds in ONE process; after a warm-up rollout of each the two
ALTERNATE, --runs (default 12, at least 10) rollouts each, a host clock around ``run`` ending in a device synchronise: median, min,
max and env-steps/s.  Then the step's policy part alone, ``mixed_step`` with a full record on the first runner's env between device
events, --step_runs calls of each alternating, in microseconds -- once with the league's round-robin deal (on the step-by-step path
every tile is a run of its own: a launch and a copy each) and once with the two nets in two contiguous blocks (two runs).  Both runners' final buffers are compared (bit-identity is the
acceptance criterion; the speed has no threshold).  Writes ONE JSON object to --out and prints it.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ENV_ID = "RoboSumo-Ant-vs-Bug-v0"


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return dict(median=float(np.median(xs)), min=float(xs.min()), max=float(xs.max()), n=int(xs.size))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_env", type=int, default=4096)
    ap.add_argument("--nsteps", type=int, default=32)
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--step_runs", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_mixed_rollout_bench.json"))
    args = ap.parse_args(argv)
    if args.num_env < 32 or args.num_env % 16 or args.runs < 10 or args.nsteps < 1 or args.step_runs < 1:
        raise SystemExit("--num_env a multiple of 16, at least 32 (a tile for each net), --runs >= 10, --nsteps and --step_runs >= 1")
    import torch
    from robosumo_selfplay_amd import mixed, policies, zoo_pairs
    from robosumo_selfplay_amd.model import PPOModel
    from robosumo_selfplay_amd.vec_env import SumoVecEnv
    if not torch.cuda.is_available():
        raise SystemExit("mixed_rollout_bench needs a HIP device: nothing is measured without one")
    N, T = args.num_env, args.nsteps
    with np.load(os.path.join(ROOT, "tests", "golden", "zoo_v3_params.npz"), allow_pickle=False) as z:
        nets = [z["bug-mlp-v3"].copy(), z["bug-lstm-v3"].copy()]
    runners = {}
    for fused in (True, False):
        env = SumoVecEnv(ENV_ID, num_envs=N, seed=0)
        spec = policies.PolicySpec(env.model.obs_dims[0], env.model.act_dims[0], value_network="copy", activation="relu")
        np.random.seed(0)
        model = PPOModel(policy=spec, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, trainable=False)
        model.act_model.seed(1)
        runners[fused] = mixed.MixedRunner(env, model, zoo_pairs.seat_for(env, 1, nets), T, 0.995, 0.95, 500, fused=fused, seat_seed=2)
    dev = runners[True].device
    out = dict(metric="mixed_rollout_s", env_id=ENV_ID, num_env=N, nsteps=T, runs=args.runs, seat=["mlp", "lstm"],
               device=torch.cuda.get_device_name(0), timing="host clock around MixedRunner.run ending in a device synchronise; the two "
               "alternate after one warm-up rollout each")
    try:
        times = {True: [], False: []}
        for k in range(args.runs + 1):                          # round 0 is the warm-up of each
            for fused in (True, False):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                runners[fused].run(k + 1)
                torch.cuda.synchronize(dev)
                if k:
                    times[fused].append(time.perf_counter() - t0)
        same = all(torch.equal(runners[True].last_buffers[k], runners[False].last_buffers[k]) for k in runners[True].last_buffers)
        same = bool(same and torch.equal(runners[True].state, runners[False].state)
                    and torch.equal(runners[True].env.obs_dev, runners[False].env.obs_dev))
        out["bit_identical_after_%d_rollouts" % (args.runs + 1)] = same
        for fused, name in ((True, "fused"), (False, "definition")):
            s = stats(times[fused])
            s["env_steps_per_s"] = N * T / s["median"]
            out[name] = s
        out["rollout_speedup_of_medians"] = out["definition"]["median"] / out["fused"]["median"]
        # the policy part of one step alone, between device events
        r = runners[True]
        B = r.last_buffers
        rec = dict(obs=B["obs"][0], act=B["act"][0], nlp=B["nlp"][0], val=B["val"][0], done=B["done"][0])
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        # ... with the league's deal (round robin: every tile is a run of its own on the step-by-step path) and with the two nets in two
        # contiguous blocks (two runs), which separates the kernel from the number of launches
        blocks = torch.sort(r.tile_entry).values.contiguous()
        out["policy_step_us"] = dict(timing="device events around mixed_step with a full record, %d calls each, alternating" % args.step_runs)
        for deal, te in (("round_robin", r.tile_entry), ("two_blocks", blocks)):
            runs1 = zoo_pairs.seat_runs(te)
            us = {True: [], False: []}
            for k in range(args.step_runs + 3):
                for fused in (True, False):
                    ev[0].record()
                    mixed.mixed_step(r.env, r.learner_seat, r.zoo_seat, te, r.state, B["noise0"][0], B["noise1"][0], None, rec, fused,
                                     r.status, None, runs1)
                    ev[1].record()
                    torch.cuda.synchronize(dev)
                    if k >= 3:
                        us[fused].append(ev[0].elapsed_time(ev[1]) * 1e3)
            out["policy_step_us"][deal] = dict(seat_runs=len(runs1), fused=stats(us[True]), definition=stats(us[False]))
    finally:
        for r in runners.values():
            r.env.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
