#!/usr/bin/env python3
"""Throughput of the A2C learner (alg_ac.learn, --algo ac): Ant-vs-Ant, --envs envs, nsteps 5, reference defaults otherwise.

Runs --warmup + --updates updates of ``learn`` itself in this one process (bounded, no retries) and prints ONE JSON line:
updates/s and env-steps/s over the timed updates (wall clock, everything included: opponent selection, rollout, optimiser step,
checkpoint writes), and the per-update medians of the parts learn() times -- opponent selection (select_ms), the fused rollout
launch + V-trace + episode harvest (rollout_ms), batch assembly + the optimiser step (update_ms) -- plus what is left (host_ms).
An env-step is one step of one env (both agents).
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robosumo_selfplay_amd import hostcfg  # noqa: E402

hostcfg.apply()
import numpy as np  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="RoboSumo-Ant-vs-Ant-v0")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--nsteps", type=int, default=5)
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--opponent_mode", default="latest", choices=["ours", "latest", "random"])
    ap.add_argument("--save_interval", type=int, default=3000)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    if args.updates < 1 or args.warmup < 1 or args.updates + args.warmup > 100000:
        raise SystemExit("--updates / --warmup out of range")
    import torch
    from robosumo_selfplay_amd import alg_ac, defaults
    from robosumo_selfplay_amd.vec_env import make_vec_env
    env = make_vec_env(args.env, args.envs, args.seed, device=0, groups=1)
    kw = defaults.get_default_params(args.env, "ac")
    kw.update(nsteps=args.nsteps, save_interval=args.save_interval)
    stamps = []
    nup = args.warmup + args.updates
    with tempfile.TemporaryDirectory() as d:
        model = alg_ac.learn(network="mlp", env=env, seed=args.seed, total_timesteps=args.envs * args.nsteps * nup, nagent=2, log_dir=d,
                             verbose=False, opponent_mode=args.opponent_mode, update_fn=lambda u: stamps.append(time.perf_counter()), **kw)
    env.close()
    h = model.history
    W = args.warmup
    wall = stamps[-1] - stamps[W - 1]
    med = lambda k: 1e3 * float(np.median(h[k][W:]))
    per_update_ms = 1e3 * wall / args.updates
    out = dict(metric="a2c_updates_per_s", env=args.env, envs=args.envs, nsteps=args.nsteps, updates=args.updates, warmup=W,
               opponent_mode=args.opponent_mode, updates_per_s=args.updates / wall,
               env_steps_per_s=args.updates * args.envs * args.nsteps / wall, ms_per_update=per_update_ms,
               select_ms=med("select_s"), rollout_ms=med("rollout_s"), update_ms=med("update_s"),
               host_ms=per_update_ms - med("select_s") - med("rollout_s") - med("update_s"),
               rollout_aborts=int(sum(h["env_rollout_aborts"])), losses_finite=bool(all(np.isfinite(l).all() for l in h["lossvals"])),
               device=torch.cuda.get_device_name(0))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
