#!/usr/bin/env python3
"""Throughput of checkpoint-vs-checkpoint matches: the fused match launch (sumo_match_steps) against the step-by-step path
(ppo_forward for both sides of every match-up -- PPOModel.step's kernel -- plus step_device), same match-ups, same noise.

    python tools/match_bench.py --num_env 4096 --pairs 16 --steps 256 --chunk 64
    python tools/match_bench.py --network lstm     # LSTM(128) checkpoints: sumo_match_steps_lstm against ppo_lstm_step per side
    python tools/match_bench.py --opponent zoo --repeats 3   # MLP checkpoints against policy-zoo MLP nets: sumo_match_steps_zoo
                                                   # against ppo_forward + ppo_forward_filtered per step, repeats interleaved
    python tools/match_bench.py --opponent zoo_lstm [--network lstm]   # checkpoints against policy-zoo LSTM nets:
                                                   # sumo_match_steps_zoo_lstm / sumo_match_steps_lstm_zoo_lstm against ppo_forward
                                                   # (or ppo_lstm_step) + ppo_lstm_step per step
    python tools/match_bench.py --network cross [--lstm_side 1]   # MLP(64,64) against LSTM(128) checkpoints, the LSTM table as agent
                                                   # --lstm_side: sumo_match_steps_cross against ppo_forward + ppo_lstm_step per step
    python tools/match_bench.py --network lstm --opponent zoo     # LSTM(128) checkpoints against policy-zoo MLP nets:
                                                   # sumo_match_steps_lstm_zoo against ppo_lstm_step + ppo_forward_filtered per step

Prints one JSON line: env-steps/s and finished matches per second of both paths (stochastic play, Ant-vs-Ant by default)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _zoo_flat(policy_zoo, D, A, rng):
    """A synthetic policy-zoo MLP vector: unit-count filter sums, O(1) weights."""
    import numpy as np
    sh = policy_zoo.zoo_mlp_shapes(D, A)
    parts = []
    for k in policy_zoo._ZOO_MLP_ORDER:
        s = sh[k]
        v = {"count": 1000.0, "sum": 1000.0 * rng.normal(0, 0.5, s), "sumsq": 1000.0 * (0.25 + rng.uniform(0.0, 2.0, s))}.get(k.split("/")[-1])
        if v is None:
            v = rng.normal(-1.0, 0.3, s) if k == "logstd" else rng.normal(0, 1.0 / max(1.0, float(s[0])) ** 0.5 if k.endswith("/w") else 0.1, s)
        parts.append(np.asarray(v, np.float32).ravel())
    return np.concatenate(parts)


def _zoo_lstm_flat(policy_zoo, D, A, rng):
    """A synthetic policy-zoo LSTM vector: unit-count filter sums, O(1) weights."""
    import numpy as np
    sh = policy_zoo.zoo_lstm_shapes(D, A)
    parts = []
    for k in policy_zoo._ZOO_LSTM_ORDER:
        s = sh[k]
        v = {"count": 1000.0, "sum": 1000.0 * rng.normal(0, 0.5, s), "sumsq": 1000.0 * (0.25 + rng.uniform(0.0, 2.0, s))}.get(k.split("/")[-1])
        if v is None:
            v = rng.normal(-1.0, 0.3, s) if k == "logstd" else rng.normal(0, 1.0 / max(1.0, float(s[0])) ** 0.5 if len(s) == 2 else 0.1, s)
        parts.append(np.asarray(v, np.float32).ravel())
    return np.concatenate(parts)


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="RoboSumo-Ant-vs-Ant-v0")
    ap.add_argument("--num_env", type=int, default=4096)
    ap.add_argument("--pairs", type=int, default=16, help="match-ups; each gets a contiguous block of num_env / pairs envs")
    ap.add_argument("--steps", type=int, default=256, help="timed env steps per path")
    ap.add_argument("--chunk", type=int, default=64, help="steps per fused launch (and per counter read on both paths)")
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--skip_stepwise", action="store_true")
    ap.add_argument("--network", choices=("mlp", "lstm", "cross"), default="mlp", help="MLP(64,64) or LSTM(128) snapshots, or an MLP "
                    "table against an LSTM(128) table (cross)")
    ap.add_argument("--lstm_side", type=int, choices=(0, 1), default=0, help="--network cross: the agent the LSTM table plays")
    ap.add_argument("--opponent", choices=("checkpoint", "zoo", "zoo_lstm"), default="checkpoint", help="agent 1: checkpoints of the same "
                    "table, synthetic policy-zoo MLP nets (one per pair) in a ZooTable, or synthetic policy-zoo LSTM nets in a ZooLstmTable")
    ap.add_argument("--repeats", type=int, default=1, help="timed runs per path, interleaved fused / step by step; the JSON line then "
                    "carries every run and the spread (max - min) of each path")
    args = ap.parse_args(argv)
    if args.network == "cross" and args.opponent != "checkpoint":
        raise SystemExit("--network cross plays checkpoints against checkpoints")
    import numpy as np
    import torch
    from robosumo_selfplay_amd import matches, policies
    from robosumo_selfplay_amd.vec_env import SumoVecEnv
    N, K = args.num_env, args.chunk
    env = SumoVecEnv(args.env, num_envs=N, seed=0, adjust_z=-0.5)
    D, A = env.observation_space[0].shape[0], env.action_space[0].shape[0]
    nsnap = 2 * args.pairs
    rng = np.random.default_rng(0)
    table = ltable = None
    if args.network in ("lstm", "cross"):
        from robosumo_selfplay_amd.lstm_model import LstmSpec
        ltable = matches.LstmSnapshotTable(LstmSpec(D, A, 128), nsnap, env.device)
        for j in range(nsnap):
            ltable.set(j, [p + 0.1 * rng.standard_normal(p.shape).astype(np.float32)
                           for p in policies.init_lstm_param_list(D, A, 128, np.random.RandomState(j))])
    if args.network in ("mlp", "cross"):
        table = matches.SnapshotTable(policies.PolicySpec(D, A, value_network="copy", activation="relu"), nsnap, env.device)
        for j in range(nsnap):
            table.set(j, policies.flatten_params([p + 0.1 * rng.standard_normal(p.shape).astype(np.float32)
                                                  for p in policies.init_param_list(D, A)]))
    mlp_table = table
    if args.network == "lstm":
        table = ltable
    epp = N // args.pairs
    zoo_table = None
    if args.opponent == "zoo":
        from robosumo_selfplay_amd import policy_zoo
        zoo_table = policy_zoo.ZooTable([_zoo_flat(policy_zoo, D - 1, A, rng) for _ in range(args.pairs)], A, env.device)
    elif args.opponent == "zoo_lstm":
        from robosumo_selfplay_amd import policy_zoo
        zoo_table = policy_zoo.ZooLstmTable([_zoo_lstm_flat(policy_zoo, D - 1, A, rng) for _ in range(args.pairs)], A, env.device)
    idx0_h, idx1_h, _ = matches.env_assignment([(2 * p, p if zoo_table is not None else 2 * p + 1) for p in range(args.pairs)],
                                               list(range(args.pairs)), epp, N)
    idx0, idx1 = torch.from_numpy(idx0_h).cuda(), torch.from_numpy(idx1_h).cuda()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    noise = tuple(torch.randn((K, N, A), generator=gen, device="cuda") for _ in range(2))
    out = dict(env=args.env, network=args.network, opponent=args.opponent, num_env=N, pairs=args.pairs, chunk=K)
    if args.network == "cross":
        out["lstm_side"] = args.lstm_side
    quota = 1 << 30
    if args.network == "cross":
        tables = (ltable, mlp_table) if args.lstm_side == 0 else (mlp_table, ltable)
    else:
        tables = (table, zoo_table if zoo_table is not None else table)
    pairing = matches.match_pairing(*tables)
    states = tuple(None if s.width is None else torch.zeros((N, s.width), dtype=torch.float32, device="cuda") for s in pairing.seats)

    def launch(fused, score):
        i0, i1 = (idx0, idx1) if fused else (idx0_h, idx1_h)
        matches.pairing_steps(env, pairing, states, i0, i1, score, quota, K, noise, fused)

    def run(fused, steps):
        score = torch.zeros((N, 3), dtype=torch.int32, device="cuda")
        env._needs_seed = True
        env.reset_device()
        for st in states:
            if st is not None:
                st.zero_()
        for _ in range(-(-args.warmup // K)):
            launch(fused, score)
        score.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        while n < steps:
            launch(fused, score)
            score.sum().item()                    # the per-launch counter read of play_matches
            n += K
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return n * N / dt, int(score.sum().item()) / dt

    runs = {True: [], False: []}
    for _ in range(max(1, args.repeats)):              # interleaved: drift of the machine hits both paths alike
        for fused in (True,) if args.skip_stepwise else (True, False):
            runs[fused].append(run(fused, args.steps))
    for fused, name in ((True, "fused"), (False, "stepwise")):
        if runs[fused]:
            eps = sorted(r[0] for r in runs[fused])
            out[name + "_env_steps_per_s"], out[name + "_matches_per_s"] = eps[len(eps) // 2], sorted(r[1] for r in runs[fused])[len(eps) // 2]
            if args.repeats > 1:
                out[name + "_runs"], out[name + "_spread"] = [r[0] for r in runs[fused]], eps[-1] - eps[0]
    if runs[False]:
        out["speedup"] = out["fused_env_steps_per_s"] / out["stepwise_env_steps_per_s"]
    env.close()
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main(sys.argv[1:])
