#!/usr/bin/env python3
"""Time of one seat's actions of one step in zoo-vs-zoo play (robosumo_selfplay_amd/zoo_pairs.py ``seat_act``): the one-launch seat
kernel (``fused=True``, ``ppo_zoo_seat_act``) against its step-by-step definition (``fused=False``: one ``ppo_forward_filtered`` /
``ppo_lstm_step`` launch per run of tiles that share a net, plus the mask conversion and the copies into the action buffer).

Agent 1 of --num_env (default 4096) RoboSumo-Spider-vs-Spider-v0 envs after a reset, stochastic actions; the seat holds 1, 2 and 6
nets, MLP and LSTM mixed, dealt over the envs in contiguous blocks as ``play_zoo_pairs`` deals them.  The nets are the spider
vectors of tests/golden/zoo_v3_params.npz and scaled copies of them (the time does not depend on the weights), or --zoo DIR's
spider files.  Each case: --warmup calls, then --runs calls timed one by one with device events; median, min and max in
microseconds.  Writes ONE JSON object to --out and prints it.
"""
import argparse
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

CASES = (("1_mlp", ("mlp",)), ("1_lstm", ("lstm",)), ("2_mixed", ("mlp", "lstm")), ("6_mixed", ("mlp", "lstm", "mlp", "lstm", "mlp", "lstm")))


def nets_of(kinds, zoo):
    if zoo:
        files = {k: sorted(glob.glob(os.path.join(zoo, "spider", k, "agent-params-v*.npy"))) for k in ("mlp", "lstm")}
        seen = {"mlp": 0, "lstm": 0}
        out = []
        for k in kinds:
            out.append(np.load(files[k][seen[k] % len(files[k])], allow_pickle=False))
            seen[k] += 1
        return out
    with np.load(os.path.join(ROOT, "tests", "golden", "zoo_v3_params.npz"), allow_pickle=False) as z:
        base = {k: z["spider-%s-v3" % k].copy() for k in ("mlp", "lstm")}
    return [(base[k] * np.float32(1.0 - 0.01 * j)).astype(np.float32) for j, k in enumerate(kinds)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_env", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--zoo", default=None, help="the policy zoo's assets directory (default: the test fixture's spider nets)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_zoo_pair_bench.json"))
    args = ap.parse_args(argv)
    if args.num_env < 96 or args.num_env % 16 or args.runs < 1 or args.warmup < 1:
        raise SystemExit("--num_env a multiple of 16, at least 96 (a tile for each of six nets), --runs and --warmup >= 1")
    import torch
    from robosumo_selfplay_amd import zoo_pairs
    from robosumo_selfplay_amd.vec_env import SumoVecEnv
    N, side = args.num_env, 1
    env = SumoVecEnv("RoboSumo-Spider-vs-Spider-v0", num_envs=N, seed=0, adjust_z=zoo_pairs.EVAL_ADJUST_Z)
    out = dict(metric="zoo_seat_act_us", env_id=env.spec.id, num_env=N, side=side, runs=args.runs, warmup=args.warmup,
               nets="zoo files" if args.zoo else "fixture spider nets and scaled copies", device=torch.cuda.get_device_name(0), cases={})
    try:
        env.reset_device()
        gen = torch.Generator(device=env.device).manual_seed(0)
        for name, kinds in CASES:
            seat = zoo_pairs.seat_for(env, side, nets_of(kinds, args.zoo))
            env_net = np.repeat(np.arange(N // 16) * len(kinds) // (N // 16), 16)      # contiguous blocks of whole tiles, near equal
            tiles_h = seat.tile_entries(env_net)
            tiles, runs = torch.from_numpy(tiles_h).to(env.device), zoo_pairs.seat_runs(tiles_h)
            noise = torch.randn((N, seat.ac_dim), generator=gen, device=env.device)
            res = {}
            for label, fused in (("fused", True), ("stepwise", False)):
                state = seat.new_state(N)
                call = lambda: zoo_pairs.seat_act(seat, env, side, tiles, state, noise, fused=fused, runs=runs)
                for _ in range(args.warmup):
                    call()
                ts = []
                for _ in range(args.runs):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    call()
                    e1.record()
                    e1.synchronize()
                    ts.append(1e3 * e0.elapsed_time(e1))
                res[label] = dict(median=float(np.median(ts)), min=float(np.min(ts)), max=float(np.max(ts)))
            res["launches_stepwise"] = len(runs)
            res["speedup_median"] = res["stepwise"]["median"] / res["fused"]["median"]
            out["cases"][name] = res
    finally:
        env.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
