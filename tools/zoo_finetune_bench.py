#!/usr/bin/env python3
"""What fine-tuning a policy-zoo MLP net costs and whether it learns (one GPU; no threshold, these are first measurements).

    python tools/zoo_finetune_bench.py --part timing --out profiles/zoo_finetune.json     # rollout_s / update_s per update, three learners
    python tools/zoo_finetune_bench.py --part kernel --out profiles/zoo_finetune.json     # ppo_grad_act (tanh) against ppo_grad per call
    python tools/zoo_finetune_bench.py --part learn  --out profiles/zoo_finetune.json     # a fine-tuning run, then 512 games against the source

``timing``: Ant-vs-Ant, 4096 envs x 128 steps, the reference's PPO defaults otherwise; the zoo learner (step-by-step rollouts), the relu
learner on the same step-by-step path (SUMO_FUSED_ROLLOUT=0) and the relu learner on the fused path; the first update (graph capture,
allocations) is left out of the medians.  ``kernel``: one minibatch of 16 384 rows, both entries between device events, alternating, the
median of 30.  ``learn``: ant-mlp-v3 against the frozen ant-mlp-v3 (opponent_mode='fix') for ``--updates`` updates of 1024 x 128, then
the last checkpoint against its source through zoo_pairs.tournament, 256 games on each seat.  Each part merges its result into ``--out``.
The zoo vectors are those of tests/golden/zoo_v3_params.npz."""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

ANT = "RoboSumo-Ant-vs-Ant-v0"


def zoo_file(tmp, name="ant-mlp-v3"):
    with np.load(os.path.join(ROOT, "tests", "golden", "zoo_v3_params.npz"), allow_pickle=False) as z:
        path = os.path.join(tmp, name + ".npy")
        np.save(path, z[name])
    return path


def med(xs):
    return float(statistics.median(xs))


def part_timing(args, tmp):
    from robosumo_selfplay_amd import alg_ppo, defaults
    from robosumo_selfplay_amd.vec_env import make_vec_env
    src = zoo_file(tmp)
    out = {}
    cases = [("zoo_mlp", "0", dict(network="zoo_mlp", zoo_init=src, opponent_mode="latest")),
             ("relu_stepwise", "0", dict(network="mlp", opponent_mode="latest")),
             ("relu_fused", "1", dict(network="mlp", opponent_mode="latest"))]
    for name, fused, kw in cases:
        os.environ["SUMO_FUSED_ROLLOUT"] = fused            # the Runner reads it when it is built
        cfg = defaults.get_default_params(ANT, "ppo")
        cfg.update(nsteps=args.nsteps)
        if kw["network"] == "zoo_mlp":
            for k in ("value_network", "num_hidden", "num_layers", "activation"):
                cfg.pop(k, None)
        cfg.update(kw)
        env = make_vec_env(ANT, args.num_env, 1, groups=2 if fused == "0" else 1)
        try:
            model = alg_ppo.learn(env=env, seed=1, total_timesteps=args.num_env * args.nsteps * args.timing_updates, nagent=2,
                                  log_dir=os.path.join(tmp, name), verbose=False, save_interval=1, **cfg)
        finally:
            env.close()
        h = model.history
        out[name] = dict(updates=args.timing_updates, rollout_s=h["rollout_s"], update_s=h["update_s"],
                         rollout_s_median=med(h["rollout_s"][1:]), update_s_median=med(h["update_s"][1:]),
                         nminibatches=cfg["nminibatches"], noptepochs=cfg["noptepochs"])
        print(name, "rollout %.3f s  update %.3f s" % (out[name]["rollout_s_median"], out[name]["update_s_median"]), flush=True)
    os.environ.pop("SUMO_FUSED_ROLLOUT", None)
    return dict(env=ANT, num_env=args.num_env, nsteps=args.nsteps, cases=out)


def part_kernel(args, tmp):
    import torch
    from robosumo_selfplay_amd import ppo_capi
    L, dev = ppo_capi.lib(), torch.device("cuda:0")
    ob, ac, n, NB = 120, 8, 16384, 4096 * 128
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)
    P = L.ppo_param_count(ob, ac)
    params = 0.1 * rn(P)
    obs, act = rn(NB, ob + 1).clamp_(-5, 5), rn(NB, ac)
    ret, adv, old, w = rn(NB), rn(n), rn(NB) + 11.0, torch.ones(NB, device=dev)
    idx = torch.randperm(NB, device=dev, generator=g)[:n].to(torch.int32)
    grads, stats, lr = torch.zeros(P, device=dev), torch.zeros(8, dtype=torch.float64, device=dev), torch.zeros(n, device=dev)
    ws = torch.zeros(L.ppo_grad_workspace_bytes(ob, ac), dtype=torch.uint8, device=dev)
    head = (params.data_ptr(), obs.data_ptr(), ob + 1, ob, ac, act.data_ptr(), adv.data_ptr(), ret.data_ptr(), old.data_ptr(), w.data_ptr(),
            idx.data_ptr(), n, 1.0 / n, 0.2, 0.0, 0.5)
    tail = (grads.data_ptr(), stats.data_ptr(), lr.data_ptr(), ws.data_ptr(), None)
    calls = dict(ppo_grad=lambda: L.ppo_grad(*head, *tail), ppo_grad_act_tanh=lambda: L.ppo_grad_act(*head, ppo_capi.GRAD_TANH, 2.0, 0.5, *tail))
    times = {k: [] for k in calls}
    for rep in range(5 + 30):                                # five warm-up rounds, then 30 alternating
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ppo_capi.chk(fn())
            e1.record()
            e1.synchronize()
            if rep >= 5:
                times[k].append(e0.elapsed_time(e1) * 1e3)
    out = dict(rows=n, ob_dim=ob, ac_dim=ac, unit="us per call (gradient kernel + slab reduction)", calls=30)
    for k, v in times.items():
        out[k] = dict(median=med(v), min=min(v), max=max(v))
        print(k, "median %.1f us  min %.1f  max %.1f" % (med(v), min(v), max(v)), flush=True)
    return out


def part_learn(args, tmp):
    from robosumo_selfplay_amd import alg_ppo, defaults, zoo_pairs
    from robosumo_selfplay_amd.vec_env import make_vec_env
    src = zoo_file(tmp)
    cfg = defaults.get_default_params(ANT, "ppo")
    for k in ("value_network", "num_hidden", "num_layers", "activation"):
        cfg.pop(k, None)
    cfg.update(nsteps=128, lr=args.lr, network="zoo_mlp", zoo_init=src, opponent_mode="fix", fix_opponent_path=src)
    log = os.path.join(tmp, "learn")
    env = make_vec_env(ANT, 1024, 1, groups=2, adjust_z=-0.5)            # the zoo nets' own setting (policy_zoo.EVAL_ADJUST_Z)
    try:
        model = alg_ppo.learn(env=env, seed=1, total_timesteps=1024 * 128 * args.updates, nagent=2, log_dir=log, verbose=True, log_interval=5,
                              **cfg)
    finally:
        env.close()
    h = model.history
    last = os.path.join(log, "checkpoints", "%.5i" % args.updates)
    games = {}
    for seat, (f0, f1) in (("tuned_on_seat0", ([last], [src])), ("tuned_on_seat1", ([src], [last]))):
        r = zoo_pairs.tournament(ANT, f0, f1, 256, num_env=256, seed=7)
        games[seat] = [int(x) for x in r["counts"][0, 0]]            # agent 0 wins, agent 1 wins, draws
    wins, losses = games["tuned_on_seat0"][0] + games["tuned_on_seat1"][1], games["tuned_on_seat0"][1] + games["tuned_on_seat1"][0]
    draws = games["tuned_on_seat0"][2] + games["tuned_on_seat1"][2]
    print("fine-tuned vs source over 512 games: %d wins, %d losses, %d draws" % (wins, losses, draws), flush=True)
    return dict(env=ANT, source="ant-mlp-v3", opponent="ant-mlp-v3 (fix)", num_env=1024, nsteps=128, updates=args.updates, lr=args.lr,
                nminibatches=cfg["nminibatches"], noptepochs=cfg["noptepochs"], adjust_z=-0.5,
                lossvals=[[float(x) for x in l] for l in h["lossvals"]], rollout_s=h["rollout_s"], update_s=h["update_s"],
                games=games, tuned_wins=wins, tuned_losses=losses, draws=draws)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", required=True, choices=["timing", "kernel", "learn"])
    ap.add_argument("--out", required=True)
    ap.add_argument("--num_env", type=int, default=4096)
    ap.add_argument("--nsteps", type=int, default=128)
    ap.add_argument("--timing_updates", type=int, default=4)
    ap.add_argument("--updates", type=int, default=40, help="learn: updates of 1024 x 128")
    ap.add_argument("--lr", type=float, default=1e-4, help="learn: step size (the reference's 1e-3 starts nets from scratch)")
    args = ap.parse_args()
    import torch
    with tempfile.TemporaryDirectory(prefix="zoo_finetune_") as tmp:
        res = dict(timing=part_timing, kernel=part_kernel, learn=part_learn)[args.part](args, tmp)
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc.update(tool="tools/zoo_finetune_bench.py", device=torch.cuda.get_device_name(0), torch=torch.__version__)
    doc[args.part] = res
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
