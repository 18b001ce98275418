#!/usr/bin/env python3
"""CLI counterpart of the reference's run.py (run.py:211-251) for the hot path:
    python run.py --env RoboSumo-Ant-vs-Ant-v0 --num_env 4096 --num_timesteps 2097152 --nsteps=128
    python run.py --env RoboSumo-Ant-vs-Ant-v0 --algo ac --num_env 1024 --num_timesteps 512000      (A2C learner, one GPU)
    python run.py --env RoboSumo-Ant-vs-Ant-v0 --num_env 1024 --nsteps=128 --eval_interval 5 --eval_opponent 00000 \\
        --eval_opponent <zoo>/ant/mlp/agent-params-v1.npy      (play the live learner against fixed opponents every 5 updates)
    python run.py --co_train --env RoboSumo-Ant-vs-Bug-v0 --num_env 4096 --nsteps=128      (two species against each other, co_train.learn)
    python run.py --co_train --fused_rollout --env RoboSumo-Ant-vs-Bug-v0 --num_env 4096 --nsteps=128      (its rollouts in the fused launch)
    python run.py --env RoboSumo-Ant-vs-Ant-v0 --num_env 4096 --nsteps=128 --resume_interval 10 --resume      (write a resume state every
        10 updates; started again after a kill, the same command continues the run bit for bit)
The run directory gets the reference's run files (log.txt, progress.csv, 0.0.monitor.csv, its pickles; ``--no_run_log``: none).
Unknown ``--key=value`` flags are forwarded to ``learn`` like the reference does (run.py:29-63), but parsed with
``ast.literal_eval`` instead of ``eval``.  Under ``torchrun`` every rank takes an equal shard of ``--num_env``.
"""
import argparse
import ast
import os
import pickle
import shutil
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def parse_unknown(args):
    out = {}
    for a in args:
        if not a.startswith("--") or "=" not in a:
            raise SystemExit("cannot parse extra argument %r (expected --key=value)" % a)
        k, v = a[2:].split("=", 1)
        try:
            v = ast.literal_eval(v)
        except (ValueError, SyntaxError):
            pass
        if k == "fix_opponent_path" and k in out:      # given several times: a league of policy-zoo nets (one occurrence: a single net)
            out[k] = (out[k] if isinstance(out[k], list) else [out[k]]) + [v]
        else:
            out[k] = v
    return out


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="RoboSumo-Ant-vs-Ant-v0")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--num_timesteps", type=float, default=1e8)
    ap.add_argument("--network", default="mlp", help="mlp (relu 64-64, the default), lstm, or zoo_mlp: fine-tune the policy-zoo MLP net given by "
                    "--zoo_init (--algo ppo; the checkpoints are zoo files)")
    ap.add_argument("--zoo_init", default=None, help="--network zoo_mlp: the policy-zoo MLP .npy file to start from")
    ap.add_argument("--num_env", type=int, default=1)
    ap.add_argument("--algo", default="ppo", help="ppo (PPO2, alg_ppo.learn) or ac (A2C, alg_ac.learn); the reference's td3 is not ported")
    ap.add_argument("--log_path", default="results")
    ap.add_argument("--suffix", default="0")
    ap.add_argument("--env_groups", type=int, default=0, help="env groups per GPU (vec_env.SumoVecEnv): 0 = 1 when the whole rollout is one fused "
                    "launch that balances the envs itself (MLP policies, LSTM policies with nlstm 128), 2 for step-by-step launches on two streams")
    ap.add_argument("--cfrc_mode", default="zero", choices=["zero", "rne_post"], help="contact-force observation entries: zero = the reference's "
                    "behaviour (MuJoCo 2.1 without force sensors), rne_post = as mj_rnePostConstraint would fill them (second launch per step)")
    ap.add_argument("--adjust_z", type=float, default=0.0, help="Agent._adjust_z (agents.py:33): offset of the torso height the agents report "
                    "(observations, lose test).  0 = the reference's training setting (its run.py:76-77 leaves the -0.5 commented out); its "
                    "evaluation / play scripts use -0.5, which is what the policy-zoo nets expect")
    ap.add_argument("--fused_fix_opponent", action="store_true", help="opponent_mode=fix: play the policy-zoo net (MLP or LSTM file) inside the fused "
                    "rollout launch (sumo_rollout_steps_zoo / sumo_rollout_steps_zoo_lstm; --network lstm: sumo_rollout_steps_lstm_zoo / sumo_rollout_steps_lstm_zoo_lstm).  Opt-in: the action noise is drawn per rollout buffer instead of per step, "
                    "so the same seed gives another, equally valid random stream")
    ap.add_argument("--fused_selector", action="store_true", help="opponent_mode=ours with MLP policies: keep the run's checkpoints in a device table "
                    "and score the selector's candidates in one launch per update (policy_selector.FusedSelector) instead of one file read and one "
                    "forward launch per candidate.  Opt-in; --algo ppo only")
    ap.add_argument("--selector_table_mb", type=float, default=None, help="--fused_selector: device memory the checkpoint table may take, in MiB "
                    "(default 1024).  A run whose checkpoints fit gets one row per checkpoint, allocated before the first update; a longer run, "
                    "or a smaller value here, gets the 32-row staging table (3 MiB on Ant) refilled from the sampled files each update")
    ap.add_argument("--no_run_log", action="store_true", help="do not write the run's files (log.txt, progress.csv, 0.0.monitor.csv, history.json, "
                    "the reference's pickles; robosumo_selfplay_amd/runlog.py).  They are written by default, as the reference's run.py always "
                    "configures its logger on the run directory")
    ap.add_argument("--eval_interval", type=int, default=0, help="evaluate the live learner against the --eval_opponent list every so many "
                    "updates (and at the first and the last), inside the training process (robosumo_selfplay_amd/train_eval.py); 0 = never")
    ap.add_argument("--eval_opponent", action="append", default=None, help="an evaluation opponent, repeatable: a policy-zoo .npy file (MLP or "
                    "LSTM), 00000 (the run's own first checkpoint) or a checkpoint path of the learner's family")
    ap.add_argument("--eval_trials", type=int, default=None, help="games per evaluation and opponent (default 64)")
    ap.add_argument("--eval_num_env", type=int, default=None, help="envs of the evaluation env (default 64)")
    ap.add_argument("--eval_stochastic", action="store_true", help="sample the evaluated actions (default: the mode, as the reference's evaluator)")
    ap.add_argument("--eval_cross_family", action="store_true", help="let an LSTM learner play zoo MLP files in its evaluation (refused otherwise)")
    ap.add_argument("--co_train", action="store_true", help="a MIXED match-up (RoboSumo-Ant-vs-Bug-v0, ...): train one MLP learner per side against "
                    "the other side's checkpoints (co_train.learn; --opponent_mode=latest, the default here, or =random).  The run directory "
                    "gets agent0/ and agent1/, each a run directory of its own")
    ap.add_argument("--fused_rollout", action="store_true", help="--co_train: run each rollout's steps inside the engine's fused launch "
                    "(sumo_rollout_steps_pair: both seats act in the wave that owns the env) instead of three launches per step.  Opt-in; "
                    "the same checkpoints bit for bit; not with --cfrc_mode rne_post")
    ap.add_argument("--resume_interval", type=int, default=0, help="write the run's whole state (learner, optimiser, generators, Runner, envs) "
                    "into <run dir>/resume/state.pt after every K-th update and after the last (robosumo_selfplay_amd/resume.py); 0 = never")
    ap.add_argument("--resume", action="store_true", help="continue the run in the run directory from its resume state, bit for bit; the "
                    "directory is kept.  Without a state file the run starts from update 1, so a job script can always pass it")
    return ap


def check_resume(args, world):
    """What --resume / --resume_interval refuse, before an env is built: each combination with its own message."""
    if not (args.resume or args.resume_interval):
        return
    if args.resume_interval < 0:
        raise SystemExit("--resume_interval is a number of updates, 0 or more")
    if args.algo != "ppo":
        raise SystemExit("--resume / --resume_interval belong to --algo ppo: the %s learner keeps no resume state" % args.algo)
    if args.co_train:
        raise SystemExit("--resume / --resume_interval are not available with --co_train (co_train.learn keeps no resume state)")
    if world > 1:
        raise SystemExit("--resume / --resume_interval run on a single GPU: launch without torchrun / with WORLD_SIZE=1")
    sides = args.env.replace("RoboSumo-", "").rsplit("-v", 1)[0].split("-vs-")
    if len(sides) == 2 and sides[0] != sides[1]:
        raise SystemExit("--resume / --resume_interval are not available on a mixed match-up (%s): only homogeneous scenes are resumed" % args.env)


def check_zoo_mlp(args, extra, world):
    """What --network zoo_mlp / --zoo_init refuse, before an env is built: each combination with its own message."""
    if args.network != "zoo_mlp":
        if args.zoo_init is not None:
            raise SystemExit("--zoo_init belongs to --network zoo_mlp")
        return
    if args.zoo_init is None:
        raise SystemExit("--network zoo_mlp needs --zoo_init <policy-zoo MLP .npy file>")
    if args.algo != "ppo":
        raise SystemExit("--network zoo_mlp belongs to --algo ppo: the %s learner does not take it" % args.algo)
    if args.co_train:
        raise SystemExit("--network zoo_mlp is not available with --co_train (both seats hold MLP(64,64) policies)")
    if extra.get("opponent_mode", "ours") == "ours":
        raise SystemExit("--network zoo_mlp: --opponent_mode=ours (the default) is not available; give --opponent_mode=latest, random or fix")
    if int(extra.get("opponent_pool", 1)) > 1:
        raise SystemExit("--network zoo_mlp: --opponent_pool is not available")
    if args.fused_selector:
        raise SystemExit("--network zoo_mlp: --fused_selector serves opponent_mode=ours, which this learner does not run")
    if args.fused_fix_opponent:
        raise SystemExit("--network zoo_mlp: --fused_fix_opponent is not available, the zoo-architecture learner plays step by step")
    if args.eval_interval or args.eval_opponent:
        raise SystemExit("--network zoo_mlp: --eval_interval / --eval_opponent are not available; the checkpoints are zoo files, play them "
                         "with zoo_tournament.py")
    if args.resume or args.resume_interval:
        raise SystemExit("--network zoo_mlp: --resume / --resume_interval are not available")
    if world > 1:
        raise SystemExit("--network zoo_mlp runs on a single GPU: launch without torchrun / with WORLD_SIZE=1")
    sides = args.env.replace("RoboSumo-", "").rsplit("-v", 1)[0].split("-vs-")
    if len(sides) == 2 and sides[0] != sides[1]:
        raise SystemExit("--network zoo_mlp is not available on a mixed match-up (%s): homogeneous scenes only" % args.env)


def check_co_train(args, extra, world):
    """What --co_train refuses, before an env is built: each combination with its own message."""
    if args.algo != "ppo":
        raise SystemExit("--co_train trains two PPO learners: --algo %s is not available with it" % args.algo)
    if args.network != "mlp":
        raise SystemExit("--co_train: both seats hold MLP(64,64) policies, --network %s is not available" % args.network)
    mode = extra.get("opponent_mode", "latest")
    if mode == "fix":
        raise SystemExit("--co_train with --opponent_mode=fix: a learner against policy-zoo nets is a plain run (leave --co_train out)")
    if mode == "ours":
        raise SystemExit("--co_train with --opponent_mode=ours: the selector would have to score another species' samples; use latest or random")
    if extra.get("use_opponent_data") is not None:
        raise SystemExit("--co_train: --use_opponent_data is not available, a learner cannot score another species' action")
    if int(extra.get("opponent_pool", 1)) > 1:
        raise SystemExit("--co_train: --opponent_pool is not available, each side keeps one frozen checkpoint")
    if args.fused_selector:
        raise SystemExit("--co_train: --fused_selector serves opponent_mode=ours, which co-training cannot run")
    if args.eval_interval or args.eval_opponent:
        raise SystemExit("--co_train: evaluation while training (--eval_interval / --eval_opponent) is out of scope; evaluate agent0/ and "
                         "agent1/ afterwards with eval_against_fix.py --fused and compare_versions.py")
    if world > 1:
        raise SystemExit("--co_train runs on a single GPU: launch it without torchrun / with WORLD_SIZE=1")
    if args.fused_rollout and args.cfrc_mode != "zero":
        raise SystemExit("--co_train --fused_rollout: not with --cfrc_mode %s, whose observations a second launch per step completes (leave "
                         "--fused_rollout out)" % args.cfrc_mode)


def co_train_main(args, extra):
    """--co_train: ``co_train.learn`` on a mixed env, the run directory prepared as ``main`` prepares it."""
    from robosumo_selfplay_amd import co_train, defaults, dist as sdist
    check_co_train(args, extra, sdist.env_rank_world()[2])
    from robosumo_selfplay_amd.vec_env import make_vec_env
    kw = defaults.get_default_params(args.env, "ppo")
    for k in ("rho_bar", "c_bar"):          # the importance clips of opponent-data reuse: no such samples here
        kw.pop(k)
    kw.update(extra)
    kw.setdefault("opponent_mode", "latest")
    if args.fused_rollout:
        kw["fused_rollout"] = True
    log_path = os.path.join(args.log_path, "%s-%s" % (args.env, args.suffix))
    # the step-by-step env launches run on two streams by default; a fused launch balances its envs itself
    groups = max(1, args.env_groups or (1 if args.fused_rollout else 2))
    env = make_vec_env(args.env, args.num_env, args.seed, device=0, groups=groups if args.num_env % (16 * groups) == 0 else 1,
                       cfrc_mode=args.cfrc_mode, adjust_z=args.adjust_z)
    try:
        co_train.check_learn(env, network=args.network, opponent_mode=kw["opponent_mode"], nsteps=kw["nsteps"], nminibatches=kw["nminibatches"],
                             fused_rollout=args.fused_rollout)
        shutil.rmtree(log_path, ignore_errors=True)
        os.makedirs(log_path, exist_ok=True)
        with open(os.path.join(log_path, "config.pkl"), "wb") as f:
            pickle.dump(dict(vars(args), **kw), f)
        return co_train.learn(network=args.network, env=env, seed=args.seed, total_timesteps=int(args.num_timesteps), log_dir=log_path, **kw)
    finally:
        env.close()


def eval_kwargs(args):
    """The ``learn`` keywords of the run-log and evaluation flags; the evaluation ones only where they were given."""
    kw = dict(run_log=not args.no_run_log)
    if args.eval_interval:
        kw["eval_interval"] = args.eval_interval
    if args.eval_opponent:
        kw["eval_opponents"] = list(args.eval_opponent)
    for k in ("eval_trials", "eval_num_env"):
        if getattr(args, k) is not None:
            kw[k] = getattr(args, k)
    if args.eval_stochastic:
        kw["eval_deterministic"] = False
    if args.eval_cross_family:
        kw["eval_cross_family"] = True
    return kw


def main(argv):
    args, unknown = build_parser().parse_known_args(argv)
    extra = parse_unknown(unknown)
    if args.network == "zoo_mlp" or args.zoo_init is not None:
        from robosumo_selfplay_amd import dist as sdist
        check_zoo_mlp(args, extra, sdist.env_rank_world()[2])
    if args.resume or args.resume_interval:
        from robosumo_selfplay_amd import dist as sdist
        check_resume(args, sdist.env_rank_world()[2])
    if args.co_train:
        return co_train_main(args, extra)
    if args.fused_rollout:
        raise SystemExit("--fused_rollout belongs to --co_train (a homogeneous match-up's rollouts run in the fused launch by default)")
    from robosumo_selfplay_amd import alg_ac, alg_ppo, defaults, dist as sdist
    from robosumo_selfplay_amd.vec_env import make_vec_env
    learn = {"ppo": alg_ppo.learn, "ac": alg_ac.learn}.get(args.algo)
    kw = defaults.get_default_params(args.env, args.algo)       # (td3 / unknown algorithms stop here)
    kw.update(extra)
    kw.update(eval_kwargs(args))
    if args.fused_fix_opponent:
        kw["fused_fix_opponent"] = True
    if args.fused_selector:
        if args.algo != "ppo":
            raise SystemExit("--fused_selector belongs to --algo ppo (the A2C learner's 'ours' mode scores no candidates)")
        kw["fused_selector"] = True
    if args.selector_table_mb is not None:
        if not args.fused_selector or not args.selector_table_mb > 0:
            raise SystemExit("--selector_table_mb is a positive size in MiB and belongs to --fused_selector")
        kw["selector_table_mb"] = args.selector_table_mb
    if args.algo == "ac":             # the A2C learner's scope, checked before anything touches the GPU
        if sdist.env_rank_world()[2] > 1:
            raise SystemExit("--algo ac runs on a single GPU: launch it without torchrun / with WORLD_SIZE=1")
        alg_ac.check_config(args.network, kw.get("use_opponent_data"), None)
    comm = sdist.init_process_group()
    rank, local_rank, world = sdist.env_rank_world()
    log_path = os.path.join(args.log_path, "%s-%s" % (args.env, args.suffix))
    resuming = False
    if args.resume or args.resume_interval:
        from robosumo_selfplay_amd import resume as resume_state
        kw.update(resume=args.resume, resume_interval=args.resume_interval)
        resuming = args.resume and os.path.exists(resume_state.state_path(log_path))
    if rank == 0:
        if not resuming:                                                   # a run that continues keeps its directory
            shutil.rmtree(log_path, ignore_errors=True)                    # run.py:233-234
        os.makedirs(log_path, exist_ok=True)
    start, per = sdist.shard_envs(args.num_env, rank, world)
    if args.env_groups <= 0:
        stepwise = (os.environ.get("SUMO_FUSED_ROLLOUT", "1") == "0" or args.cfrc_mode != "zero" or args.network == "zoo_mlp"
                    or (args.network == "lstm" and int(extra.get("nlstm", 128)) != 128))
        args.env_groups = 2 if stepwise else 1
    groups = args.env_groups if per % max(1, args.env_groups) == 0 else 1
    import torch
    local_rank = local_rank % max(1, torch.cuda.device_count())        # gloo rehearsal of N ranks on fewer GPUs
    env = make_vec_env(args.env, per, args.seed + start, device=local_rank, groups=groups, cfrc_mode=args.cfrc_mode, adjust_z=args.adjust_z)  # run.py:144: env i gets seed + i
    if args.network in ("lstm", "zoo_mlp"):   # the RoboSumo defaults describe the MLP (defaults.py:8-26); recurrent nets share the latent, a zoo file fixes its own architecture
        for k in ("value_network", "num_hidden", "num_layers", "activation"):
            kw.pop(k, None)
    if args.network == "zoo_mlp":
        kw["zoo_init"] = args.zoo_init
    if rank == 0:
        with open(os.path.join(log_path, "config.pkl"), "wb") as f:        # run.py:176-177
            pickle.dump(dict(vars(args), **kw), f)
    model = learn(network=args.network, env=env, seed=args.seed, total_timesteps=int(args.num_timesteps) // world,
                  nagent=len(env.agents), log_dir=log_path, comm=comm, **kw)
    env.close()
    return model


if __name__ == "__main__":
    main(sys.argv[1:])
