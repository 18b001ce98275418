#!/usr/bin/env python3
"""Throughput of the rollout launches of learn(opponent_mode='fix') against a policy-zoo net, next to plain self-play: K rollout steps
per launch through the Runner's own drivers (noise draws included), the fused launch against the step-by-step launches.

    python tools/fix_rollout_bench.py --opponent zoo_lstm   # sumo_rollout_steps_zoo_lstm against ppo_forward + ppo_lstm_step per step
    python tools/fix_rollout_bench.py --opponent zoo        # sumo_rollout_steps_zoo against ppo_forward + ppo_forward_filtered
    python tools/fix_rollout_bench.py --opponent self       # sumo_rollout_steps (MLP self-play) against ppo_selfplay_forward
    python tools/fix_rollout_bench.py --network lstm --opponent zoo        # sumo_rollout_steps_lstm_zoo: an LSTM(128) learner
    python tools/fix_rollout_bench.py --network lstm --opponent zoo_lstm   # sumo_rollout_steps_lstm_zoo_lstm
    python tools/fix_rollout_bench.py --opponent league --league-mlp 3 --league-lstm 3   # sumo_rollout_steps_zoo_league against the
                                                                   # step-by-step league path (--network lstm: sumo_rollout_steps_lstm_zoo_league;
                                                                   # one of the two counts 0: that family's launch with its index array filled)

Every repeat times `launches` windows of K steps on each path, fused and step by step interleaved, after `warmup` windows; the envs
keep running from window to window.  Prints one JSON line: env-steps/s per repeat and the median of both paths."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="RoboSumo-Ant-vs-Ant-v0")
    ap.add_argument("--num_env", type=int, default=4096)
    ap.add_argument("--K", type=int, default=20, help="rollout steps per launch (the rollout buffer's length)")
    ap.add_argument("--launches", type=int, default=10, help="timed K-step windows per repeat and path")
    ap.add_argument("--warmup", type=int, default=5, help="untimed K-step windows per path")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--opponent", choices=("self", "zoo", "zoo_lstm", "league"), default="zoo_lstm")
    ap.add_argument("--league-mlp", default="0", help="--opponent league: its zoo MLP members, a count of synthetic nets or a comma-separated list of .npy files")
    ap.add_argument("--league-lstm", default="0", help="--opponent league: its zoo LSTM members, likewise")
    ap.add_argument("--network", choices=("mlp", "lstm"), default="mlp", help="the learner: MLP(64,64) nets or an LSTM(128) (LstmPPOModel; "
                    "--opponent zoo / zoo_lstm)")
    ap.add_argument("--skip_stepwise", action="store_true")
    args = ap.parse_args(argv)
    if args.network == "lstm" and args.opponent == "self":
        ap.error("--network lstm measures the fix-mode launches: --opponent zoo, zoo_lstm or league (tools/lstm_bench.py times recurrent self-play)")
    import numpy as np
    import torch
    from tools.match_bench import _zoo_flat, _zoo_lstm_flat
    from robosumo_selfplay_amd import lstm_model, policies, policy_zoo
    from robosumo_selfplay_amd.model import PPOModel
    from robosumo_selfplay_amd.runner import Runner
    from robosumo_selfplay_amd.vec_env import SumoVecEnv

    def runner():
        env = SumoVecEnv(args.env, num_envs=args.num_env, seed=3)
        D, A = env.observation_space[0].shape[0], env.action_space[0].shape[0]
        if args.network == "lstm":
            spec = lstm_model.LstmSpec(D, A, 128)
            models = [lstm_model.LstmPPOModel(policy=spec, nbatch_act=args.num_env, nsteps=args.K, trainable=False) for _ in range(2)]
        else:
            spec = policies.PolicySpec(D, A, value_network="copy", activation="relu")
            models = [PPOModel(policy=spec, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, trainable=False) for _ in range(2)]
        rng = np.random.default_rng(1)
        fixed = None
        if args.opponent == "zoo":
            fixed = policy_zoo.FixedOpponentModel(policy_zoo.ZooMLPPolicy(_zoo_flat(policy_zoo, D - 1, A, rng), A))
        elif args.opponent == "zoo_lstm":
            fixed = policy_zoo.FixedOpponentModel(policy_zoo.ZooLSTMPolicy(_zoo_lstm_flat(policy_zoo, D - 1, A, rng), A))
        elif args.opponent == "league":
            def members(arg, synth, load_kind):
                if arg.isdigit():
                    return [policy_zoo.load_zoo_policy_from_flat(synth(policy_zoo, D - 1, A, rng), A, kind=load_kind) for _ in range(int(arg))]
                return [policy_zoo.load_zoo_policy(f, A, kind=load_kind) for f in arg.split(",")]
            nets = members(args.league_mlp, _zoo_flat, "mlp") + members(args.league_lstm, _zoo_lstm_flat, "lstm")
            fixed = policy_zoo.FixedOpponentModel(policy_zoo.ZooLeague(nets, args.num_env, env.device))
        if fixed is not None and args.network == "mlp":
            models[1] = fixed
        for k, m in enumerate(models):
            m.act_model.seed(100 + k)
        r = Runner(env=env, models=models, nsteps=args.K, nagent=2, gamma=0.995, lam=0.95, rho_bar=1.0, c_bar=1.0)
        if fixed is not None and args.network == "lstm":      # as learn() does: the Runner is built on two recurrent models first
            fixed.act_model.seed(101)
            r.models[1] = fixed
        r.fused_fix_opponent = True
        return r

    def window(r, B, fused):
        if fused:
            r.fused_steps()(B, 0, args.K, 0.5)
        else:
            for s in range(args.K):
                r._step_device(B, s, 0.5)

    paths = [True] if args.skip_stepwise else [True, False]
    rs = {f: runner() for f in paths}
    for f, r in rs.items():
        r.fused_rollout = f
        assert (r.fused_steps() is not None) == f, "the fused launch does not apply"
    Bs = {f: r._alloc_device(args.K) for f, r in rs.items()}
    rates = {f: [] for f in paths}
    for rep in range(args.repeats + 1):                      # repeat 0 is the warm-up
        for f in paths:
            n = args.warmup if rep == 0 else args.launches
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                window(rs[f], Bs[f], f)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep:
                rates[f].append(args.num_env * args.K * n / dt)
    for f, r in rs.items():
        if f:
            for E in r.env.engines:
                E.rollout_status()
        assert r.env.stats()["rollout_aborts"] == 0
    out = dict(network=args.network, opponent=args.opponent, env=args.env, num_env=args.num_env, K=args.K, launches=args.launches, repeats=args.repeats)
    if args.opponent == "league":
        out.update(league_mlp=args.league_mlp, league_lstm=args.league_lstm)
    for f in paths:
        name = "fused" if f else "stepwise"
        out[name + "_env_steps_per_s"] = [round(x) for x in rates[f]]
        out[name + "_median"] = round(float(np.median(rates[f])))
    print(json.dumps(out))
    for r in rs.values():
        r.env.close()
    return out


if __name__ == "__main__":
    main(sys.argv[1:])
