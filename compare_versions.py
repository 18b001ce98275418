#!/usr/bin/env python3
"""CLI counterpart of the reference's compare_history_version.py: play saved checkpoints of two runs against each other on the GPU
(version i of P1 as agent 0 against version i of P2 as agent 1) and print / save P1's win rate per version -- or, with
--round_robin, every selected version of one run against every other (win / draw / loss matrix).

    python compare_versions.py --p1 results/ours/RoboSumo-Ant-vs-Ant-v0-0 --p2 results/random/RoboSumo-Ant-vs-Ant-v0-0 --trials 100
    python compare_versions.py --path results/RoboSumo-Ant-vs-Ant-v0-0 --round_robin --interval 10 --trials 100

Play is stochastic (model.step samples, as in the reference script) unless --deterministic is given; every agent reports its
height with adjust_z = -0.5 (compare_history_version.py:73-74).  MLP(64,64) and LSTM runs (learn(network='lstm')) are both
accepted: the network is read from the checkpoints and recorded in the JSON output; both runs must use the same one, unless
--cross_family is given: then an MLP(64,64) run and an LSTM run play each other, P1 as agent 0.

    python compare_versions.py --p1 results/mlp/RoboSumo-Ant-vs-Ant-v0-0 --p2 results/lstm/RoboSumo-Ant-vs-Ant-v0-0 --cross_family
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def parse_args(argv):
    ap = argparse.ArgumentParser(description="Play checkpoints of self-play runs against each other (fused match launch).")
    ap.add_argument("--p1", help="run directory (holding checkpoints/) of player 1 (agent 0)")
    ap.add_argument("--p2", help="run directory of player 2 (agent 1)")
    ap.add_argument("--path", help="run directory for --round_robin")
    ap.add_argument("--round_robin", action="store_true", help="every selected version of --path against every other")
    ap.add_argument("--trials", type=int, default=10, help="games per version pair (compare_history_version.py --trials)")
    ap.add_argument("--num_env", type=int, default=256)
    ap.add_argument("--interval", type=int, default=1, help="round robin: every interval-th version")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--deterministic", action="store_true", help="act with the policy means instead of sampling")
    ap.add_argument("--adjust_z", type=float, default=-0.5, help="Agent._adjust_z of every agent (compare_history_version.py:73-74)")
    ap.add_argument("--env", default="RoboSumo-Ant-vs-Ant-v0")
    ap.add_argument("--chunk", type=int, default=64, help="env steps per fused launch")
    ap.add_argument("--cross_family", action="store_true", help="paired mode: let an MLP(64,64) run play an LSTM run (refused otherwise)")
    ap.add_argument("--out", help="JSON output path (default: next to the run)")
    args = ap.parse_args(argv)
    if args.round_robin:
        if not args.path or args.p1 or args.p2:
            ap.error("--round_robin takes --path (and no --p1 / --p2)")
    elif not (args.p1 and args.p2) or args.path:
        ap.error("give --p1 and --p2 (paired mode) or --path with --round_robin")
    if args.trials < 1 or args.num_env < 1 or args.interval < 1 or args.chunk < 1:
        ap.error("--trials, --num_env, --interval and --chunk must be >= 1")
    return args


def main(argv):
    args = parse_args(argv)
    from robosumo_selfplay_amd import matches
    kw = dict(num_env=args.num_env, deterministic=args.deterministic, seed=args.seed, adjust_z=args.adjust_z, env_id=args.env,
              chunk=args.chunk)
    if args.round_robin:
        r = matches.round_robin(args.path, args.interval, args.trials, **kw)
        V = len(r["versions"])
        for i in range(V):
            for j in range(V):
                if i != j:
                    print("-----%s vs %s win: %.2f, draw: %.2f, lose: %.2f-----" % (r["versions"][i], r["versions"][j], r["win"][i, j],
                                                                                  r["draw"][i, j], r["loss"][i, j]))
        rec = dict(mode="round_robin", path=args.path, trials=args.trials, deterministic=args.deterministic, network=r["network"],
                   nlstm=r["nlstm"], versions=r["versions"],
                   win=[[None if i == j else float(r["win"][i, j]) for j in range(V)] for i in range(V)],
                   draw=[[None if i == j else float(r["draw"][i, j]) for j in range(V)] for i in range(V)],
                   loss=[[None if i == j else float(r["loss"][i, j]) for j in range(V)] for i in range(V)])
        out = args.out or os.path.join(args.path, "round_robin.json")
    else:
        from robosumo_selfplay_amd import mjcf
        m = mjcf.load_model(args.env)
        if m.obs_dims[0] != m.obs_dims[1] or m.act_dims[0] != m.act_dims[1]:      # the two sides of a co-trained run (run.py --co_train)
            from robosumo_selfplay_amd import co_train
            if args.cross_family:
                raise SystemExit("--cross_family is about LSTM runs; mixed match-ups compare MLP(64,64) runs")
            r = co_train.compare_history_versions(args.p1, args.p2, args.trials, interval=args.interval, **kw)
        else:
            r = matches.compare_history_versions(args.p1, args.p2, args.trials, cross_family=args.cross_family, **kw)
        for (a, b), w, res in zip(r["versions"], r["win_rate"], r["results"]):
            print("-----P1 %s vs P2 %s: P1 win rate %.2f (%d wins, %d losses, %d draws)-----" % (a, b, w, res["wins"], res["losses"],
                                                                                             res["draws"]))
        rec = dict(mode="paired", p1=args.p1, p2=args.p2, trials=args.trials, deterministic=args.deterministic,
                   network=r["network"], nlstm=r["nlstm"], versions=[list(v) for v in r["versions"]], win_rate=r["win_rate"],
                   results=r["results"], cross_family=args.cross_family)
        if "networks" in r:
            rec["networks"] = r["networks"]
        out = args.out or os.path.join(args.p1, "compare_versions_vs_%s.json" % os.path.basename(os.path.normpath(args.p2)))
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote %s" % out)
    return rec


if __name__ == "__main__":
    main(sys.argv[1:])
