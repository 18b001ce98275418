"""Evaluation of the live learner inside ``learn()`` (alg_ppo / alg_ac).

In self-play ``eprewmean`` says nothing about strength: the reference measures it in a separate pass over the checkpoints
(eval_robosumo_against_fix.py, compare_history_version.py).  Here the learner's parameters go device to device into row 0 of a
snapshot table and play, as agent 0, ``eval_trials`` games against every evaluation opponent through the drivers of the offline
evaluator (``matches.play_against_zoo`` for policy-zoo files, ``matches.play_matches`` for checkpoints), with its settings:
``adjust_z = EVAL_ADJUST_Z``, the same batching, seeding and quota -- so an evaluation at update u returns exactly what the
offline call returns on checkpoint u.

:func:`plan_evaluation` is the pure part: it reads the opponents' files, refuses everything unsupported with the message the
offline path gives, and names the driver of every opponent; it needs no GPU.  :class:`Evaluator` owns the device side: its env,
its tables and (inside the drivers) its ``torch.Generator``.  It constructs no model and draws from no global random stream, and
the training env is never touched.
"""
import os
import time
import types

import numpy as np

from . import matches, policy_zoo

FIRST_CHECKPOINT = "00000"        # the evaluation opponent that names the run's own first checkpoint


def _ckpt_shape(network, ob_dim, ac_dim, nlstm):
    """What ``matches.match_pairing`` and the checks read of a snapshot table, without the device table."""
    return types.SimpleNamespace(recurrent=network == "lstm", spec=types.SimpleNamespace(ob_dim=ob_dim, ac_dim=ac_dim, nlstm=nlstm))


def _zoo_shape(kind, nparams, ac_dim):
    """The same of a zoo table holding one net of ``nparams`` entries (both families' counts are affine in ``ob_dim``)."""
    count = policy_zoo.zoo_lstm_param_count if kind == "lstm" else policy_zoo.zoo_mlp_param_count
    ob_dim = (int(nparams) - count(0, ac_dim)) // (count(1, ac_dim) - count(0, ac_dim))
    return types.SimpleNamespace(recurrent=kind == "lstm", hidden=policy_zoo.HIDDEN, ob_dim=ob_dim, ac_dim=ac_dim)


def plan_evaluation(*, network, ob_dim, ac_dim, nlstm=128, cfrc_mode="zero", eval_interval=0, eval_opponents=None, eval_trials=64,
                    eval_num_env=64, eval_cross_family=False):
    """The checks of an in-training evaluation, before the first rollout and without a GPU.  Returns None when evaluation is off
    (``eval_interval == 0`` and no opponents), else the plan::

        dict(interval, trials, num_env, envs_per_pair, rounds_per_env, cross_family,
             opponents=[dict(name, source='zoo' | 'first' | 'checkpoint', family='mlp' | 'lstm', driver='play_against_zoo' |
                             'play_matches', entry=<the pairing's launch>, fused=bool, data=<vector | None>), ...],
             groups=[dict(driver, family, fused, positions=[indices into opponents], pairs=[(0, row), ...]), ...])

    ``eval_opponents[k]``: a policy-zoo ``.npy`` file (family read from its length), ``'00000'`` (the run's own first checkpoint,
    written by ``learn()`` itself) or a checkpoint path of the learner's family.  An opponent plays fused where its pairing's
    fused launch holds the learner (every pairing but an LSTM learner of another width than 128, which plays step by step).
    The groups are the launches of the offline evaluator: zoo MLP files, zoo LSTM files (``plan_mixed_zoo_evaluation``), then the
    checkpoints, which share the learner's table (rows 1..)."""
    given = eval_opponents is not None and len(eval_opponents) > 0
    if not eval_interval and not given:
        return None
    if isinstance(eval_opponents, (str, os.PathLike)):
        raise ValueError("eval_opponents is a list of opponents (a single one: [%r])" % (eval_opponents,))
    if not eval_interval:
        raise ValueError("eval_opponents given with eval_interval=0: set eval_interval >= 1 to evaluate against them")
    if not given:
        raise ValueError("eval_interval=%r without eval_opponents: name at least one opponent (a policy-zoo .npy, '00000' or a "
                         "checkpoint path)" % (eval_interval,))
    for name, v in (("eval_interval", eval_interval), ("eval_trials", eval_trials), ("eval_num_env", eval_num_env)):
        if int(v) != v or int(v) < 1:
            raise ValueError("%s must be an integer >= 1 (got %r)" % (name, v))
    if network not in ("mlp", "lstm"):
        raise ValueError("evaluation plays MLP(64,64) and LSTM learners (network 'mlp' | 'lstm'), not %r" % (network,))
    matches._check_cfrc_mode(cfrc_mode)
    nlstm = int(nlstm) if network == "lstm" else None
    learner = _ckpt_shape(network, ob_dim, ac_dim, nlstm)
    vector_of = matches.lstm_snapshot_vector if network == "lstm" else matches.snapshot_vector
    epp, rpe = matches.split_trials(eval_trials, eval_num_env)
    opponents = []
    for src in eval_opponents:
        name = str(src)
        if name == FIRST_CHECKPOINT:
            opp = dict(name=name, source="first", family=network, data=None)
        elif name.endswith(".npy"):
            flat = np.load(os.path.expanduser(name), allow_pickle=False)
            kind = policy_zoo.zoo_file_kind(flat.size, ac_dim)          # a net of another species fits neither family, or ...
            zoo = _zoo_shape(kind, flat.size, ac_dim)
            if not eval_cross_family:
                matches._check_zoo_family(learner, zoo)
            matches._check_zoo_dims(learner, zoo)                       # ... reads more observation columns than the env has
            opp = dict(name=name, source="zoo", family=kind, data=flat)
        else:
            # the offline tables' own refusals: another family, another LSTM width, another observation / action space
            opp = dict(name=name, source="checkpoint", family=network, data=vector_of(learner.spec, name))
        other = learner if opp["source"] != "zoo" else zoo
        pairing = matches.match_pairing(learner, other)
        opp.update(driver="play_against_zoo" if opp["source"] == "zoo" else "play_matches", entry="sumo_" + pairing.entry,
                   fused=pairing.nlstm in (None, 128))
        opponents.append(opp)
    groups = []
    zoo_pos = [k for k, o in enumerate(opponents) if o["source"] == "zoo"]
    for grp in matches.plan_mixed_zoo_evaluation(1, [opponents[k]["family"] for k in zoo_pos], eval_trials, eval_num_env) if zoo_pos else ():
        pos = [zoo_pos[i] for i in grp["opponents"]]
        groups.append(dict(driver="play_against_zoo", family=grp["kind"], fused=opponents[pos[0]]["fused"], positions=pos,
                           pairs=grp["plan"]["pairs"]))
    ck_pos = [k for k, o in enumerate(opponents) if o["source"] != "zoo"]
    if ck_pos:
        groups.append(dict(driver="play_matches", family=network, fused=opponents[ck_pos[0]]["fused"], positions=ck_pos,
                           pairs=[(0, 1 + i) for i in range(len(ck_pos))]))
    return dict(interval=int(eval_interval), trials=int(eval_trials), num_env=int(eval_num_env), envs_per_pair=epp, rounds_per_env=rpe,
                cross_family=bool(eval_cross_family), network=network, nlstm=nlstm, opponents=opponents, groups=groups)


def plan_for(env, network, network_kwargs, eval_env=None, **kw):
    """:func:`plan_evaluation` for ``learn()``'s arguments: dimensions and ``cfrc_mode`` of the training env, the env count of
    ``eval_env`` where one is given.  None when evaluation is off (then ``env`` is not looked at)."""
    if not kw.get("eval_interval") and not kw.get("eval_opponents"):
        return None
    if eval_env is not None:
        if eval_env is env:
            raise ValueError("eval_env is the training env: evaluation resets and reseeds its env, give it one of its own")
        kw["eval_num_env"] = eval_env.num_envs
    return plan_evaluation(network=network, ob_dim=env.observation_space[0].shape[0], ac_dim=env.action_space[0].shape[0],
                           nlstm=network_kwargs.get("nlstm", 128), cfrc_mode=getattr(env, "cfrc_mode", "zero"), **kw)


def due(plan, update, nupdates):
    """Evaluate at every ``interval``-th update, at update 1 and at the last one."""
    return plan is not None and (update % plan["interval"] == 0 or update == 1 or update == nupdates)


class Evaluator(object):
    """The device side of a plan: the env (``eval_env``, or ``num_env`` envs of the training env's id with ``cfrc_mode='zero'``,
    built here and closed by :meth:`close`), the learner's table -- row 0 receives the live parameters at every evaluation, rows
    1.. hold the checkpoint opponents -- and one zoo table per zoo family.  Everything is loaded here, once, before the first
    rollout; ``first_checkpoint`` is the path of the run's ``00000``."""

    def __init__(self, plan, model, train_env, first_checkpoint, eval_env=None, deterministic=True, seed=0):
        if not (hasattr(model, "params") and hasattr(model, "spec")):
            raise ValueError("evaluation needs a model with a flat ``params`` vector (PPOModel, LstmPPOModel, ActorCriticModel), not a "
                             "custom model_fn")
        self.plan, self.model = plan, model
        self.deterministic, self.seed = bool(deterministic), int(seed)
        self.own_env = eval_env is None
        if self.own_env:
            from .vec_env import SumoVecEnv
            eval_env = SumoVecEnv(train_env.spec.id, num_envs=plan["num_env"], seed=self.seed, device=train_env.device.index or 0,
                                  model=train_env.model, cfrc_mode="zero")
        self.env = eval_env
        try:
            ck = [plan["opponents"][k] for g in plan["groups"] if g["driver"] == "play_matches" for k in g["positions"]]
            Table = matches.LstmSnapshotTable if plan["network"] == "lstm" else matches.SnapshotTable
            self.table = Table(model.spec, 1 + len(ck), self.env.device)
            matches._check_env(self.env, self.table)
            if self.table.params.shape[1] != model.params.numel():
                raise ValueError("the model's parameter vector (%d) is not the table's policy (%d)" % (model.params.numel(), self.table.P))
            self.table.filled[0], self.table.labels[0] = True, "learner"
            for i, o in enumerate(ck):
                self.table.set(1 + i, first_checkpoint if o["source"] == "first" else o["data"], label=o["name"])
            self.zoo_tables = {}
            for g in plan["groups"]:
                if g["driver"] == "play_against_zoo":
                    Zoo = policy_zoo.ZooLstmTable if g["family"] == "lstm" else policy_zoo.ZooTable
                    self.zoo_tables[g["family"]] = Zoo([plan["opponents"][k]["data"] for k in g["positions"]], model.spec.ac_dim, self.env.device)
        except Exception:
            self.close()
            raise

    def names(self):
        return [o["name"] for o in self.plan["opponents"]]

    def evaluate(self, update, timesteps):
        """Play the plan with the learner's parameters of now.  Returns ``dict(update, timesteps, seconds, results=[dict(opponent,
        network, win, draw, lose, rounds, env_steps), ...])``, one result per opponent in the caller's order."""
        import torch
        plan, env = self.plan, self.env
        t0 = time.perf_counter()
        self.table.params[0].copy_(self.model.params.detach().reshape(-1))          # device to device
        results = [None] * len(plan["opponents"])
        kw = dict(deterministic=self.deterministic, seed=self.seed, adjust_z=matches.EVAL_ADJUST_Z)
        for g in plan["groups"]:
            if g["driver"] == "play_against_zoo":
                res = matches.play_against_zoo(env, self.table, self.zoo_tables[g["family"]], g["pairs"], plan["rounds_per_env"],
                                               plan["envs_per_pair"], fused=g["fused"], cross_family=plan["cross_family"], **kw)
            else:
                res = matches.play_matches(env, self.table, g["pairs"], plan["rounds_per_env"], plan["envs_per_pair"], fused=g["fused"], **kw)
            for k, r in zip(g["positions"], res):
                results[k] = result_entry(plan["opponents"][k], r)
        torch.cuda.synchronize(env.device)
        return dict(update=int(update), timesteps=int(timesteps), seconds=time.perf_counter() - t0, results=results)

    def close(self):
        if self.own_env and self.env is not None:
            self.env.close()
        self.env = None


class Report(object):
    """What rank 0 of ``learn()`` does beside training, behind two calls per update: :meth:`update` (evaluate where due, flush the
    rollout's episodes) and :meth:`log` (one row of the run log).  ``run_log`` False and ``plan`` None: both do nothing."""

    def __init__(self, *, run_log, plan, log_dir, env, model, history, first_checkpoint, eval_env=None, deterministic=True, seed=0,
                 log_interval=10, verbose=False, opponent_mode=None, resume_log=None):
        """``resume_log``: the :meth:`log_state` of an interrupted run, whose files are continued instead of truncated (resume.py)."""
        from . import runlog
        self.model, self.hist, self.plan, self.log_interval, self.verbose = model, history, plan, log_interval, verbose
        self.opponent_mode = opponent_mode
        self.evaluator = self.files = self.entry = None
        if plan is not None:
            self.evaluator = Evaluator(plan, model, env, first_checkpoint, eval_env, deterministic, seed)
            history["eval"] = []
        if run_log:
            names = self.evaluator.names() if self.evaluator is not None else []
            self.files = runlog.RunLog(log_dir, env.spec.id, header=dict(eval_opponents=names), resume=resume_log)
            self.extra = dict(eval_opponents=names, loss_names=list(model.loss_names))

    def log_state(self):
        """The run log's position (``RunLog.state``) for the resume state; None without a run log."""
        return self.files.state() if self.files is not None else None

    def resumed(self):
        """After the restored ``history`` is in place: the files that are rewritten from it hold it again."""
        if self.files is not None:
            self.files.history(self.hist, **self.extra)
            if "early_stop_info" in self.hist:
                self.files.early_stop_info(self.hist["early_stop_info"])
            if self.evaluator is not None and self.hist.get("eval"):
                self.files.evaluation(self.hist["eval"])

    def update(self, update, nupdates, timesteps, epinfos):
        """After an update's optimiser steps (and outside its timing): evaluate if due -- the entry goes to ``history['eval']`` --
        and append the rollout's episodes and the reference's pickles to the run's files (``early_stop_info.pkl`` every update,
        ``ratio_summary.pkl`` on its schedule: ``opponent_mode='random'``, update 1 and every 100th).  Returns whether a row of the
        run log is due: at ``update % log_interval == 0 or update == 1`` as the reference, and at every evaluated update, so that
        no evaluation is missing from progress.csv."""
        self.entry = None
        if due(self.plan, update, nupdates):
            self.entry = self.evaluator.evaluate(update, timesteps)
            self.hist["eval"].append(self.entry)
            if self.verbose:
                print("update %d  evaluation %.2fs  %s" % (update, self.entry["seconds"], "  ".join(
                    "[%d] win %.2f draw %.2f lose %.2f" % (k, r["win"], r["draw"], r["lose"]) for k, r in enumerate(self.entry["results"]))),
                    flush=True)
        if self.files is None:
            return False
        self.files.episodes(epinfos)
        if "early_stop_info" in self.hist:
            self.files.early_stop_info(self.hist["early_stop_info"])
        if self.opponent_mode == "random" and "total_ratio_clip_frac" in self.hist and (update % 100 == 0 or update == 1):
            self.files.ratio_summary(self.hist)
        return update % self.log_interval == 0 or update == 1 or self.entry is not None

    def log(self, *, update, league, lossvals, **kw):
        """One row of log.txt / progress.csv, ``history.json`` and, where an evaluation was made, the evaluation files."""
        from . import runlog
        self.files.row(runlog.training_row(update=update, loss_names=self.model.loss_names, lossvals=lossvals, history=self.hist,
                                           league_scores=self.hist["league_scores"][-1] if league is not None else None,
                                           eval_entry=self.entry, **kw))
        self.files.history(self.hist, **self.extra)
        if self.entry is not None:
            self.files.evaluation(self.hist["eval"])

    def close(self):
        if self.files is not None:
            self.files.history(self.hist, **self.extra)
        if self.evaluator is not None:
            self.evaluator.close()


def result_entry(opponent, r):
    """One opponent's entry from a play driver's dict: rates over the games played (``matches.merge_zoo_results``)."""
    n = float(r["rounds"])
    return dict(opponent=opponent["name"], network=opponent["family"], win=r["wins"] / n, draw=r["draws"] / n, lose=r["losses"] / n,
                rounds=r["rounds"], env_steps=r["env_steps"])
