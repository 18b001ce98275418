"""A2C self-play driver: counterpart of the reference's ``alg_ac.learn`` (alg_ac.py:25-341).

Per update: opponent selection from the checkpoint directory, one rollout of ``nsteps`` steps (``runner.run(update)``: the fused
``sumo_rollout_steps`` launch with MLP policies), optional reuse of the opponent's samples, then ONE optimiser step of
``ActorCriticModel`` on the whole batch (no minibatches, no epochs: nbatch_train = nbatch, alg_ac.py:110-111).  Rollout buffers
stay in HBM.  Not reproduced: TF summaries, matplotlib histograms; the reference's ``eval_env`` runner is replaced by the
evaluation of train_eval.py (``eval_interval`` / ``eval_opponents``).

Decisions on the reference's A2C path (DESIGN.md section 8 gives the reasons):
  1. ``rho_bar`` / ``c_bar``, which alg_ac.py:153 forgets to hand to its Runner (TypeError), are ``learn`` keywords with PPO's RoboSumo
     defaults, 10.0 / 1.0.  They enter only agent 1's V-trace returns, i.e. they matter only with opponent-data reuse.
  2. ``use_opponent_data``: None and ``'direct'`` (weights 1); ``'off_policy'`` / ``'both'`` read ratios of commented-out code
     (alg_ac.py:285-290, NameError) and raise NotImplementedError.
  3. ``opponent_mode='ours'`` has no selection block in alg_ac.py:200-213: the opponent stays checkpoint 00000 for the whole run.
     That is what the reference trains against and is kept; the log line reports version 0.
The stages that are the same for both learners come from ``alg_ppo`` ("The learners: one loop, named stages").
Single GPU, MLP policies only (``comm`` / ``network='lstm'`` raise NotImplementedError)."""
import os
import os.path as osp
import time
from collections import deque

import numpy as np

from .alg_ppo import (assemble_update_batch, assign_league, check_opponent_pool, choose_opponents, collect_rollout, constfn,
                      install_fixed_opponent, install_opponents, report_update, save_checkpoint)

NEGLOGP_THRESHOLD = 50.0      # alg_ac.py:241-243, hard-coded there


def check_config(network, use_opponent_data, comm):
    """The scope of this learner, checked before anything touches the GPU."""
    if network == "lstm":
        raise NotImplementedError("the A2C learner (--algo ac) supports MLP policies only; recurrent (lstm) policies train with --algo ppo")
    if network == "zoo_mlp":
        raise NotImplementedError("the A2C learner (--algo ac) does not take network='zoo_mlp': policy-zoo nets are fine-tuned with --algo ppo")
    if use_opponent_data in ("off_policy", "both"):
        raise NotImplementedError("use_opponent_data=%r: the reference's A2C computes these importance ratios in commented-out code "
                                  "(alg_ac.py:285-290) and fails with NameError; supported here: None and 'direct'" % (use_opponent_data,))
    if use_opponent_data not in (None, "direct"):
        raise ValueError("use_opponent_data %r" % (use_opponent_data,))
    if comm is not None:
        raise NotImplementedError("the A2C learner (--algo ac) runs on a single GPU (no comm)")


def learn(*, network, env, total_timesteps, opponent_mode="ours", use_opponent_data=None, eval_env=None, seed=None, nsteps=2048,
          ent_coef=0.0, lr=3e-4, vf_coef=0.5, max_grad_norm=0.5, gamma=0.99, lam=0.95, log_interval=10, save_interval=1,
          load_path=None, model_fn=None, update_fn=None, init_fn=None, mpi_rank_weight=1, comm=None, nagent=1, anneal_bound=500,
          fix_opponent_path=None, rho_bar=10.0, c_bar=1.0, log_dir=None, verbose=True, opponent_pool=1, fused_fix_opponent=False,
          run_log=False, eval_interval=0, eval_opponents=None, eval_trials=64, eval_num_env=64, eval_deterministic=True, eval_seed=0,
          eval_cross_family=False, **network_kwargs):
    """``run_log`` and the ``eval_*`` arguments as in ``alg_ppo.learn``: the run's files (runlog.py) and the evaluation of the live
    learner against fixed opponents (train_eval.py), on ``eval_env`` or an env of its own; off by default."""
    check_config(network, use_opponent_data, comm)
    if opponent_mode not in ("ours", "random", "latest", "fix"):
        raise ValueError("opponent_mode %r" % (opponent_mode,))
    from . import train_eval
    eval_plan = train_eval.plan_for(env, network, network_kwargs, eval_env=eval_env, eval_interval=eval_interval, eval_opponents=eval_opponents,
                                    eval_trials=eval_trials, eval_num_env=eval_num_env, eval_cross_family=eval_cross_family)
    import torch
    from .a2c_model import ActorCriticModel
    from .policies import build_policy
    from .runner import Runner
    if seed is not None:                                                # set_global_seeds (misc_util.py:48-62)
        np.random.seed(seed)
        torch.manual_seed(seed)
    lr = constfn(lr) if isinstance(lr, float) else lr
    total_timesteps = int(total_timesteps)
    policy = build_policy(env, network, **network_kwargs)
    nenvs = env.num_envs
    ob_space, ac_space = env.observation_space[0], env.action_space[0]
    nbatch = nenvs * nsteps
    model_fn = model_fn or ActorCriticModel
    dev = getattr(env, "device", torch.device("cuda", 0))
    mk = lambda scope, trainable: model_fn(policy=policy, ob_space=ob_space, ac_space=ac_space, nbatch_act=nenvs, nbatch_train=nbatch,
                                           nsteps=nsteps, ent_coef=ent_coef, vf_coef=vf_coef, max_grad_norm=max_grad_norm,
                                           trainable=trainable, model_scope=scope, device=dev.index or 0)
    model = mk("model_0", True)
    models = [model] + [mk("model_%d" % i, False) for i in range(1, nagent)]
    log_dir = log_dir or os.environ.get("OPENAI_LOGDIR") or "/tmp/robosumo_selfplay_amd"
    checkdir = osp.join(log_dir, "checkpoints")
    save_checkpoint(model, checkdir, "00000")                            # alg_ac.py:117-118
    if load_path is not None:
        for m in models:
            m.load(load_path)
    for i, m in enumerate(models):
        m.act_model.seed((seed or 0) * 1000 + 17 * i)
    runner = Runner(env=env, models=models, nsteps=nsteps, nagent=nagent, gamma=gamma, lam=lam, rho_bar=rho_bar, c_bar=c_bar,
                    anneal_bound=anneal_bound)
    runner.fused_fix_opponent = bool(fused_fix_opponent)     # opt-in, as in alg_ppo: the fix-mode zoo net inside the fused launch
    # opponent_pool = K > 1 (extension, as in alg_ppo): K snapshots resident in HBM, one per env tile, drawn by the selection law of
    # opponent_mode; K = 1 is the reference's single opponent for all envs
    pool = None
    if int(opponent_pool) > 1:
        check_opponent_pool(opponent_mode, runner, fused=True)
        from .opponent_pool import OpponentPool
        pool = runner.opponent_pool = OpponentPool(policy, int(opponent_pool), nenvs, dev)
    epinfobuf = deque(maxlen=100)
    if init_fn is not None:
        init_fn()
    tfirststart = time.perf_counter()
    history = dict(opponent_versions=[], useful_ratio=[], lossvals=[], fps=[], select_s=[], rollout_s=[], update_s=[],
                   env_diverged=[], env_dropped_contacts=[], env_rollout_aborts=[],     # per update, from the engine's counters
                   league_scores=[], league_tiles=[])       # fix mode with a list of files: per update and member (alg_ppo.league_note)
    env_stats = env.stats() if hasattr(env, "stats") else None
    nupdates = total_timesteps // nbatch
    report = train_eval.Report(run_log=run_log, plan=eval_plan, log_dir=log_dir, env=env, model=model, history=history, eval_env=eval_env,
                               deterministic=eval_deterministic, seed=eval_seed, first_checkpoint=osp.join(checkdir, "00000"),
                               log_interval=log_interval, verbose=verbose, opponent_mode=opponent_mode)
    tail = dict(nupdates=nupdates, nsteps=nsteps, nbatch=nbatch, env=env, runner=runner, history=history, model=model, report=report,
                epinfobuf=epinfobuf, update_fn=update_fn, log_interval=log_interval, verbose=verbose, save_interval=save_interval,
                checkdir=checkdir)
    loaded = None        # the checkpoint(s) the opponent holds: re-read from disk only when the selection changes
    league = None        # fix mode with a list of files: the policy_zoo.ZooLeague on agent 1
    for update in range(1, nupdates + 1):
        tstart = time.perf_counter()
        frac = 1.0 - (update - 1.0) / nupdates
        lrnow = lr(frac)
        # ---- opponent selection (alg_ac.py:172-213)
        if opponent_mode == "fix":
            if update == 1:
                install_fixed_opponent(runner, fix_opponent_path, ac_space.shape[0], dev, (seed or 0) * 1000 + 17)
            league = assign_league(runner, update)
            history["opponent_versions"].append([])
        else:
            if update == 1 or opponent_mode == "ours":                   # 'ours': v0 for the whole run (decision 3 above)
                paths, choices = [osp.join(checkdir, "00000")], [0]
            else:
                paths = sorted(osp.join(checkdir, f) for f in os.listdir(checkdir))
                # 'random' over the checkpoints there are (alg_ac.py:203-205), 'latest' as in alg_ppo (:206-208)
                choices = choose_opponents(opponent_mode, len(paths), len(paths), pool.capacity if pool is not None else 1)
            sel = tuple(paths[c] for c in choices)
            if sel != loaded:
                install_opponents(runner.models[1], pool, sel)
                loaded = sel
            history["opponent_versions"].append([int(osp.basename(p)) for p in sel])
        tsel = time.perf_counter()
        # ---- rollout, timed from the end of the selection
        ro, t_roll = collect_rollout(runner, update, dev, tsel)
        # ---- batch: the learner's rows, plus the opponent's usable rows under 'direct' (alg_ac.py:241-262)
        if use_opponent_data is None:
            b_obs, b_ret, b_act, b_val = ro.obs[0], ro.returns[0], ro.actions[0], ro.values[0]
            weights = torch.ones(nbatch, dtype=torch.float32, device=dev)
            history["useful_ratio"].append(None)
        else:
            ub = assemble_update_batch(*ro[:7], None, None, nbatch=nbatch, neglogp_threshold=NEGLOGP_THRESHOLD, use_opponent_data=use_opponent_data)
            b_obs, b_ret, b_act, b_val, weights = ub["obs"], ub["returns"], ub["actions"], ub["values"], ub["weights"]
            history["useful_ratio"].append(ub["useful_ratio"])
        epinfobuf.extend(ro.epinfos[-epinfobuf.maxlen:])
        # ---- one optimiser step on the whole batch (alg_ac.py:273-276)
        out3 = model.train_device(lrnow, b_obs.contiguous(), b_ret.contiguous(), b_act.contiguous(), b_val.contiguous(), weights)
        lossvals = out3.cpu().numpy().astype(np.float64)                # (waits for the step)
        tnow = time.perf_counter()
        history["lossvals"].append(lossvals); history["fps"].append(nbatch / (tnow - tstart))
        history["select_s"].append(tsel - tstart)                      # opponent selection (checkpoint reads)
        history["rollout_s"].append(t_roll); history["update_s"].append(tnow - tsel - t_roll)
        # ---- report (alg_ppo.report_update): counters, run log, evaluation, the printed line, checkpoint (alg_ac.py:333-339)
        opp = history["opponent_versions"][-1]
        middle = "opponent %s  fps %.0f  rollout %.2fms  update %.2fms" % (opp[0] if opp else "fix", history["fps"][-1], 1e3 * t_roll,
                                                                           1e3 * history["update_s"][-1])
        env_stats = report_update(update, middle, dict(values=b_val, returns=b_ret), lossvals, ro.epinfos, env_stats, tnow - tfirststart,
                                  league=league, **tail)
    report.close()
    model.history = history
    model.time_elapsed = time.perf_counter() - tfirststart
    return model
