#!/usr/bin/env python3
"""Time of a co-training rollout on a mixed match-up (robosumo_selfplay_amd/co_train.py ``PairRunner.run``): the one-launch step
(``fused=True``, ``ppo_mixed_pair_step``) against its definition (``fused=False``: per side two ``ppo_forward`` launches -- the live
half and the frozen half -- and the torch copies of record and action buffer).

RoboSumo-Ant-vs-Bug-v0, --num_env (default 4096) envs, T = --nsteps (default 32).  Two runners on two env sets of equal seeds in ONE
process; after a warm-up rollout of each the two ALTERNATE, --runs (default 12, at least 10) rollouts each, a host clock around
``run`` ending in a device synchronise: median, min, max and env-steps/s.  Then the step's policy part alone, ``pair_step`` with full
records on the first runner's env between device events, --step_runs calls of each alternating, in microseconds.  Both runners'
final buffers are compared (bit-identity is the acceptance criterion; the speed has no threshold).  Writes ONE JSON object to --out
and prints it.

--engine_fused adds a third contender that alternates with the two in the same process: ``PairRunner(engine_fused=True)``, the rollout's
steps inside the engine's fused launch (``sumo_rollout_steps_pair``).  Its buffers are compared where it writes them: the shared ones,
each side's record over its own half of the envs, and the env's observations.  --env_id times another mixed match-up.
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
    ap.add_argument("--engine_fused", action="store_true", help="add the engine's fused launch as a third contender")
    ap.add_argument("--env_id", default=ENV_ID)
    ap.add_argument("--out", default=None, help="default: profiles/r27_co_train_bench.json, with --engine_fused profiles/r28_pair_fused_bench.json")
    args = ap.parse_args(argv)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "r28_pair_fused_bench.json" if args.engine_fused else "r27_co_train_bench.json")
    env_id = args.env_id
    if args.num_env < 32 or args.num_env % 32 or args.runs < 10 or args.nsteps < 1 or args.step_runs < 1:
        raise SystemExit("--num_env a multiple of 32, --runs >= 10, --nsteps and --step_runs >= 1")
    import torch
    from robosumo_selfplay_amd import co_train, mixed, policies
    from robosumo_selfplay_amd.model import PPOModel
    from robosumo_selfplay_amd.vec_env import SumoVecEnv
    if not torch.cuda.is_available():
        raise SystemExit("co_train_bench needs a HIP device: nothing is measured without one")
    N, T = args.num_env, args.nsteps
    runners = {}
    contenders = (True, False) + (("engine",) if args.engine_fused else ())      # fused step, definition, the engine's fused launch
    names = {True: "fused", False: "definition", "engine": "engine_fused"}
    for fused in contenders:
        env = SumoVecEnv(env_id, num_envs=N, seed=0)
        np.random.seed(0)
        models = []
        for s in range(2):
            spec = policies.PolicySpec(env.model.obs_dims[s], env.model.act_dims[s], value_network="copy", activation="relu")
            models.append(PPOModel(policy=spec, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, trainable=False))
            models[s].act_model.seed(1 + s)
        runners[fused] = co_train.PairRunner(env, models, T, 0.995, 0.95, 500, fused=fused is not False, engine_fused=fused == "engine")
        rng = np.random.default_rng(3)                          # frozen rows that differ from the live ones
        for s in range(2):
            runners[fused].set_frozen(s, (models[s].params.cpu().numpy() * (1.0 + 0.05 * rng.standard_normal(models[s].P))).astype(np.float32))
    dev = runners[True].device
    out = dict(metric="co_train_rollout_s", env_id=env_id, num_env=N, nsteps=T, runs=args.runs, device=torch.cuda.get_device_name(0),
               timing="host clock around PairRunner.run ending in a device synchronise; the contenders alternate after one warm-up rollout each")
    try:
        times = {c: [] for c in contenders}
        for k in range(args.runs + 1):                          # round 0 is the warm-up of each
            for fused in contenders:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                runners[fused].run(k + 1)
                torch.cuda.synchronize(dev)
                if k:
                    times[fused].append(time.perf_counter() - t0)
        bf, bd = runners[True].last_buffers, runners[False].last_buffers
        same = all(torch.equal(bf[k], bd[k]) for k in bf if k != "side")
        same = same and all(torch.equal(bf["side"][s][k], bd["side"][s][k]) for s in range(2) for k in bf["side"][s])
        same = bool(same and torch.equal(runners[True].env.obs_dev, runners[False].env.obs_dev))
        out["bit_identical_after_%d_rollouts" % (args.runs + 1)] = same
        for fused in contenders:
            s = stats(times[fused])
            s["env_steps_per_s"] = N * T / s["median"]
            out[names[fused]] = s
        if args.engine_fused:
            be, re_ = runners["engine"].last_buffers, runners["engine"]
            same = all(torch.equal(bf[k], be[k]) for k in bf if k != "side")
            for s in range(2):
                own = co_train.own_envs(N, s)
                same = same and all(torch.equal(bf["side"][s][k][:, own], be["side"][s][k][:, own]) for k in bf["side"][s])
            same = bool(same and torch.equal(runners[True].env.obs_dev, re_.env.obs_dev) and torch.equal(runners[True].env.done_dev, re_.env.done_dev))
            out["engine_fused_bit_identical_after_%d_rollouts" % (args.runs + 1)] = same
            out["engine_fused_speedup_of_medians_over_fused"] = out["fused"]["median"] / out["engine_fused"]["median"]
            out["engine_fused_median_below_fused_min"] = bool(out["engine_fused"]["median"] < out["fused"]["min"])
        out["rollout_speedup_of_medians"] = out["definition"]["median"] / out["fused"]["median"]
        # the policy part of one step alone, between device events
        r = runners[True]
        records = tuple({k: b[k][0] for k in mixed.RECORD_KEYS} for b in bf["side"])
        noise = tuple(b["noise"][0] for b in bf["side"])
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        us = {True: [], False: []}
        for k in range(args.step_runs + 3):
            for fused in (True, False):
                ev[0].record()
                co_train.pair_step(r.env, r.seats, r.tile_rows, noise, records, fused, r.status, r._runs)
                ev[1].record()
                torch.cuda.synchronize(dev)
                if k >= 3:
                    us[fused].append(ev[0].elapsed_time(ev[1]) * 1e3)
        out["policy_step_us"] = dict(timing="device events around pair_step with full records, %d calls each, alternating" % args.step_runs,
                                     fused=stats(us[True]), definition=stats(us[False]))
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
