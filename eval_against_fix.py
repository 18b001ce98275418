#!/usr/bin/env python3
"""CLI counterpart of the reference's eval_robosumo_against_fix.py (:121-262): play saved checkpoints of a run against a
fixed policy-zoo opponent (MLP or LSTM net) on the GPU and print / save win, draw and lose rates per checkpoint.

    python eval_against_fix.py --path results/RoboSumo-Ant-vs-Ant-v0-0 --opponent_path <zoo>/ant/mlp/agent-params-v3.npy \\
        --num_env 256 --rounds 512 --interval 10
    python eval_against_fix.py --path results/RoboSumo-Ant-vs-Ant-v0-0 --opponent_path <zoo v1>.npy --opponent_path <zoo v3>.npy \
        --fused --trials 512 --interval 10      (all checkpoints x opponents batched over the envs, one fused launch per 64 steps;
                                                 MLP and LSTM opponent files may be mixed: each family plays in launches of its own;
                                                 an LSTM run plays zoo MLP files with --cross_family)
    python eval_against_fix.py --path results/RoboSumo-Ant-vs-Bug-v0-0 --env RoboSumo-Ant-vs-Bug-v0 --fused --trials 512 \
        --opponent_path <zoo>/bug/mlp/agent-params-v3.npy --opponent_path <zoo>/bug/lstm/agent-params-v3.npy
                                                (a run on a mixed match-up: mixed.evaluate_history_against_zoo, --trials a multiple of 16)
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--path", required=True, help="run directory holding checkpoints/NNNNN (run.py --log_path/<env>-<suffix>)")
    ap.add_argument("--opponent_path", required=True, action="append",
                    help="policy-zoo .npy (robosumo/robosumo/policy_zoo/assets/<agent>/{mlp,lstm}/...); with --fused it may be given several times")
    ap.add_argument("--env", default="RoboSumo-Ant-vs-Ant-v0")
    ap.add_argument("--num_env", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=500)
    ap.add_argument("--start", type=int, default=0)
    ap.add_argument("--interval", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--stochastic", action="store_true")
    ap.add_argument("--adjust_z", type=float, default=-0.5, help="Agent._adjust_z of every agent; the reference's evaluator sets -0.5 "
                    "(eval_robosumo_against_fix.py:108-115): the zoo nets were trained with the tatami surface at z = 0")
    ap.add_argument("--cfrc_mode", default="zero", choices=["zero", "rne_post"])
    ap.add_argument("--fused", action="store_true", help="play every selected checkpoint against every opponent in fused match launches "
                    "(matches.evaluate_history_against_zoo): zoo MLP and LSTM opponents, exactly --trials games per checkpoint and opponent")
    ap.add_argument("--trials", type=int, default=None, help="games per checkpoint and opponent with --fused (default: --rounds)")
    ap.add_argument("--cross_family", action="store_true", help="with --fused: let an LSTM run play zoo MLP files too (refused otherwise)")
    args = ap.parse_args(argv)
    import numpy as np
    if args.fused:
        return main_fused(args)
    if len(args.opponent_path) != 1:
        raise SystemExit("several --opponent_path need --fused")
    args.opponent_path = args.opponent_path[0]
    from robosumo_selfplay_amd import policy_zoo
    from robosumo_selfplay_amd.model import PPOModel
    from robosumo_selfplay_amd.policies import build_policy
    from robosumo_selfplay_amd.vec_env import make_vec_env
    env = make_vec_env(args.env, args.num_env, args.seed, adjust_z=args.adjust_z, cfrc_mode=args.cfrc_mode)   # eval_robosumo_against_fix.py:108-115
    policy = build_policy(env, "mlp", value_network="copy", num_hidden=64, activation="relu")
    model = PPOModel(policy=policy, ob_space=env.observation_space[0], ac_space=env.action_space[0], trainable=False,
                     model_scope="model_0")
    opp = policy_zoo.load_zoo_policy(args.opponent_path, env.action_space[1].shape[0])
    ckdir = os.path.join(args.path, "checkpoints")
    ids = sorted(int(f) for f in os.listdir(ckdir) if f.isdigit())
    table = []
    for cid in ids:
        if cid < args.start or (cid - args.start) % args.interval:
            continue
        model.load(os.path.join(ckdir, "%.5i" % cid))
        r = policy_zoo.evaluate_against(model, opp, env, args.rounds, deterministic=not args.stochastic)
        table.append([cid, r["win"], r["draw"], r["lose"]])
        print("-----Episode %d win: %.2f, draw: %.2f, lose: %.2f (%d rounds, %d steps)-----" % (cid, r["win"], r["draw"], r["lose"],
                                                                                           r["rounds"], r["steps"]))
    with open(os.path.join(args.path, "eval_against_fix.json"), "w") as f:
        json.dump(table, f)
    env.close()
    return np.array(table)


def main_fused(args):
    import numpy as np
    from robosumo_selfplay_amd import matches
    if args.cfrc_mode != "zero":
        raise SystemExit("--fused runs on the fused match launch, which refuses --cfrc_mode rne_post")
    trials = args.trials if args.trials is not None else args.rounds
    from robosumo_selfplay_amd import mjcf
    scene = mjcf.load_model(args.env)
    if scene.obs_dims[0] != scene.obs_dims[1] or scene.act_dims[0] != scene.act_dims[1]:
        # a mixed match-up: the learner's seat against a zoo seat on the per-step env launch (--trials a multiple of 16)
        from robosumo_selfplay_amd import mixed
        if args.cross_family:
            raise SystemExit("--cross_family is about LSTM runs; mixed match-ups evaluate MLP(64,64) runs")
        r = mixed.evaluate_history_against_zoo(args.path, args.opponent_path, trials, start=args.start, interval=args.interval,
                                               num_env=args.num_env, deterministic=not args.stochastic, fused=True, seed=args.seed,
                                               adjust_z=args.adjust_z, env_id=args.env)
    else:
        r = matches.evaluate_history_against_zoo(args.path, args.opponent_path, trials, start=args.start, interval=args.interval,
                                                 num_env=args.num_env, deterministic=not args.stochastic, fused=True, seed=args.seed,
                                                 adjust_z=args.adjust_z, env_id=args.env, cross_family=args.cross_family)
    table = []
    for cid in r["checkpoints"]:
        row = [cid]
        for k in range(len(r["opponents"])):       # one (win, draw, lose) triple per opponent, in --opponent_path order
            x = r["results"][(cid, k)]
            row += [x["win"], x["draw"], x["lose"]]
            print("-----Episode %d win: %.2f, draw: %.2f, lose: %.2f (%d rounds, %d steps)-----" % (cid, x["win"], x["draw"], x["lose"],
                                                                                               x["rounds"], x["env_steps"]))
        table.append(row)
    with open(os.path.join(args.path, "eval_against_fix.json"), "w") as f:
        json.dump(table, f)
    with open(os.path.join(args.path, "eval_against_fix_networks.json"), "w") as f:   # which families met (the table above is rates only)
        json.dump(dict(cross_family=args.cross_family, networks=[dict(network=r["network"], nlstm=r["nlstm"]), r["opponent_networks"]],
                       checkpoints=r["checkpoints"], opponents=r["opponents"]), f, indent=1)
    return np.array(table)


if __name__ == "__main__":
    main(sys.argv[1:])
