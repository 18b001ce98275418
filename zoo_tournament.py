#!/usr/bin/env python3
"""Policy-zoo nets against each other on any of the nine match-ups: counterpart of the reference's robosumo/demos/play.py,
played on the GPU and counted instead of watched.

    python zoo_tournament.py --zoo robosumo/policy_zoo/assets --env RoboSumo-Ant-vs-Bug-v0 --policy-names mlp lstm --param-versions 1 2
    python zoo_tournament.py --zoo robosumo/policy_zoo/assets --env RoboSumo-Bug-vs-Spider-v0 --all --max_episodes 64 --out result.json

The nets are found as the demo finds them: the species are the 2nd and 4th dash-separated fields of the env id, agent a's file is
<zoo>/<species>/<mlp|lstm>/agent-params-v<version>.npy.  --all plays every net found for agent 0's species against every net
found for agent 1's as a round robin.  One line per pair: agent 0 wins, agent 1 wins, draws.  A pair plays whole tiles of 16
envs, so --max_episodes is rounded up to a multiple of 16.  --record DIR stores the joint positions of the first batch as
DIR/traj.npz, which `play.py --replay DIR/traj.npz --out DIR` renders.
"""
import argparse
import glob
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FAMILIES = ("mlp", "lstm")


def species_of(env_id):
    """The two agents' species, as the demo reads them from the env id."""
    f = str(env_id).split("-")
    if len(f) < 5:
        raise ValueError("%r is not a RoboSumo-<A>-vs-<B>-v0 env id" % (env_id,))
    return f[1].lower(), f[3].lower()


def zoo_paths(env_id, policy_names, param_versions, zoo_dir):
    """The demo's path rule: [<zoo>/<species>/<name>/agent-params-v<version>.npy for agent 0, the same for agent 1]."""
    if len(policy_names) != 2 or len(param_versions) != 2:
        raise ValueError("--policy-names and --param-versions take two values each")
    for p in policy_names:
        if p not in FAMILIES:
            raise ValueError("policy names are 'mlp' / 'lstm', got %r" % (p,))
    return [os.path.join(str(zoo_dir), a, p, "agent-params-v%d.npy" % int(v))
            for a, p, v in zip(species_of(env_id), policy_names, param_versions)]


def all_paths(env_id, zoo_dir):
    """([files of agent 0's species], [files of agent 1's]): every agent-params-v*.npy of either family, MLP first, by version."""
    version = lambda f: int(re.search(r"agent-params-v(\d+)\.npy$", f).group(1))
    out = []
    for a in species_of(env_id):
        files = []
        for p in FAMILIES:
            files += sorted(glob.glob(os.path.join(str(zoo_dir), a, p, "agent-params-v[0-9]*.npy")), key=version)
        if not files:
            raise ValueError("no agent-params-v*.npy under %s" % os.path.join(str(zoo_dir), a))
        out.append(files)
    return out


def parse_args(argv):
    ap = argparse.ArgumentParser(description="Play policy-zoo nets against each other on the GPU.")
    ap.add_argument("--env", default="RoboSumo-Ant-vs-Ant-v0")
    ap.add_argument("--policy-names", nargs=2, choices=FAMILIES, default=["mlp", "mlp"], metavar=("A", "B"))
    ap.add_argument("--param-versions", nargs=2, type=int, default=[1, 1], metavar=("U", "V"))
    ap.add_argument("--max_episodes", type=int, default=20, help="games per pair (rounded up to a multiple of 16)")
    ap.add_argument("--zoo", required=True, help="the policy zoo's assets directory")
    ap.add_argument("--all", action="store_true", help="round robin of every net found for each agent's species")
    ap.add_argument("--num_env", type=int, default=256)
    ap.add_argument("--deterministic", action="store_true", help="act with the policy means (the demo samples)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--stepwise", action="store_true", help="the step-by-step definition instead of the one-launch seat kernel")
    ap.add_argument("--record", metavar="DIR", help="store the first batch's joint positions as DIR/traj.npz")
    ap.add_argument("--out", metavar="result.json")
    args = ap.parse_args(argv)
    if args.max_episodes < 1 or args.num_env < 16 or args.num_env % 16:
        ap.error("--max_episodes must be >= 1 and --num_env a multiple of 16")
    return args


def main(argv):
    args = parse_args(argv)
    from robosumo_selfplay_amd import zoo_pairs
    if args.all:
        files0, files1 = all_paths(args.env, args.zoo)
    else:
        files0, files1 = [[f] for f in zoo_paths(args.env, args.policy_names, args.param_versions, args.zoo)]
    trials = -(-args.max_episodes // 16) * 16
    if trials != args.max_episodes:
        print("playing %d games per pair (whole tiles of 16 envs; asked for %d)" % (trials, args.max_episodes))
    r = zoo_pairs.tournament(args.env, files0, files1, trials, num_env=args.num_env, deterministic=args.deterministic, seed=args.seed,
                             fused=not args.stepwise, record=args.record)
    print("%s: %d games per pair; agent 0 wins, agent 1 wins, draws" % (r["env_id"], r["trials"]))
    for i, a in enumerate(r["labels0"]):
        for j, b in enumerate(r["labels1"]):
            w, l, d = (int(x) for x in r["counts"][i, j])
            print("%s  vs  %s: %d %d %d" % (a, b, w, l, d))
    result = dict(r, counts=r["counts"].tolist())
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    return result


if __name__ == "__main__":
    main(sys.argv[1:])
