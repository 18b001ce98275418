"""PPO2 self-play driver: counterpart of the reference's ``alg_ppo.learn`` (alg_ppo.py:25-513), non-recurrent branch.

Same keyword surface and per-update sequence -- opponent selection from the checkpoint directory (the checkpoint dir IS
the opponent pool, alg_ppo.py:217-244), ``runner.run(update)``, IS-ratio hygiene (:258-280), optional opponent-data reuse
(:325-344), ``noptepochs x nminibatches`` shuffled minibatch steps with KL early stop (:355-398), checkpoint every update
(:459-464) -- but rollout buffers stay in HBM and each minibatch is a row-index gather inside the gradient kernel.
``learn`` is a driver over one module-level function per stage ("The learners: one loop, named stages").
Not reproduced: matplotlib histograms per update (:292-318), TF summaries.
Multi-GPU: every rank runs this with its own env shard; ``comm`` (torch.distributed group) makes PPOModel all-reduce the
advantage moments and the fused gradient buffer.
"""
import os
import os.path as osp
import time
from collections import deque, namedtuple
from functools import partial

import numpy as np

from . import dist as sdist
from . import resume as resume_state
from . import train_eval
from .model import PPOModel
from .policies import build_policy, init_param_list
from .policy_selector import selection_probs_from_scores
from .runner import Runner


def constfn(val):
    def f(_):
        return val
    return f


def safemean(xs):
    return np.nan if len(xs) == 0 else np.mean(xs)


def explained_variance(ypred, y):
    """baselines/baselines/common/math_util.py:25-38"""
    vary = np.var(y)
    return np.nan if vary == 0 else 1 - np.var(y - ypred) / vary


def clean_ratio(r, clip_ratio):
    """alg_ppo.py:258-280 (one of its three identical blocks) on a device tensor: NaN -> clip_ratio, the mean and the
    fraction above the clip taken BEFORE clipping, then clamp to [0, clip_ratio].  Returns (cleaned, mean, clip_frac)."""
    import torch
    r = torch.where(torch.isnan(r), torch.full_like(r, clip_ratio), r)
    return r.clamp(0.0, clip_ratio), float(r.mean().item()), float((r > clip_ratio).float().mean().item())


def assemble_update_batch(obs, returns, masks, actions, values, neglogpacs, rewards, off_policy_ratio, total_ratio, *, nbatch,
                          neglogp_threshold, use_opponent_data, vgap=None, version_gap=None):
    """alg_ppo.py:286-344 on device tensors: the opponent samples whose learner-neglogp is below the threshold
    (``usable_index``), agent 0's rollout alone or followed by agent 1's usable rows, and the importance weights of
    ``direct`` / ``off_policy`` / ``both``.  The ratios are the CLEANED ones.  Returns a dict of the minibatch
    source arrays plus ``weights``, ``usable_index`` and ``useful_ratio`` (tests/test_update_glue.py checks it against a numpy
    restatement of the cited lines)."""
    import torch
    dev = returns.device
    usable = torch.nonzero(neglogpacs[1] < neglogp_threshold).flatten()
    names = ("obs", "returns", "masks", "actions", "values", "neglogpacs", "rewards")
    arrs = (obs, returns, masks, actions, values, neglogpacs, rewards)
    use_opp = use_opponent_data is not None and not (vgap is not None and version_gap is not None and version_gap > vgap)
    if not use_opp:                                                      # alg_ppo.py:325-330
        out = {k: x[0] for k, x in zip(names, arrs)}
    else:                                                                # :331-335
        out = {k: torch.cat([x[0], x[1][usable]], dim=0) for k, x in zip(names, arrs)}
    ones = torch.ones(nbatch, dtype=torch.float32, device=dev)
    if use_opponent_data is None:                                        # :337-344, keyed on the mode alone like the reference
        weights = ones
    elif use_opponent_data == "direct":
        weights = torch.ones(out["obs"].shape[0], dtype=torch.float32, device=dev)
    elif use_opponent_data == "off_policy":
        weights = torch.cat([ones, off_policy_ratio[usable]])
    elif use_opponent_data == "both":
        weights = torch.cat([ones, total_ratio[usable]])
    else:
        raise ValueError("use_opponent_data %r" % (use_opponent_data,))
    out.update(weights=weights, usable_index=usable, useful_ratio=float(usable.numel()) / float(neglogpacs[1].numel()))
    return out


def assemble_recurrent_update_batch(obs, returns, masks, actions, values, neglogpacs, rewards, off_policy_ratio, total_ratio, states0,
                                    shadow_state0, *, nenv, neglogp_threshold, use_opponent_data, vgap=None, version_gap=None):
    """``assemble_update_batch`` for a recurrent learner (pure torch, any device).  A row cannot be cut out of a sequence, so the batch
    is made of whole SEQUENCES -- agent 0's ``nenv`` first, then (when the ``vgap`` rule of the MLP path allows reuse) agent 1's
    ``nenv`` -- and agent 1's unusable rows (learner neglogp at or above the threshold, NaN included) stay in the recurrence and leave
    the loss: ``valid`` is 0 there, and so is the weight.  Every array is env-major ([nseq * nsteps, ...], ``sf01`` order); a
    sequence starts from its own state (``states0`` | ``shadow_state0``: the learner's state along agent 1's stream), runs on its
    own masks and carries its own old neglogp, values and returns.  ``weights`` on valid agent-1 rows: 1 (``direct``), the CLEANED
    ``off_policy_ratio`` (``off_policy``) or ``total_ratio`` (``both``).  Returns the dict of ``assemble_update_batch`` plus
    ``states``, ``valid`` and ``nseq``."""
    import torch
    if use_opponent_data not in ("direct", "off_policy", "both"):
        raise ValueError("use_opponent_data %r" % (use_opponent_data,))
    dev = returns.device
    usable_mask = neglogpacs[1] < neglogp_threshold
    usable = torch.nonzero(usable_mask).flatten()
    names = ("obs", "returns", "masks", "actions", "values", "neglogpacs", "rewards")
    arrs = (obs, returns, masks, actions, values, neglogpacs, rewards)
    use_opp = not (vgap is not None and version_gap is not None and version_gap > vgap)
    rows0 = returns[0].shape[0]
    ones = torch.ones(rows0, dtype=torch.float32, device=dev)
    if not use_opp:
        out = {k: x[0] for k, x in zip(names, arrs)}
        out.update(states=states0, valid=ones, weights=ones.clone(), nseq=int(nenv))
    else:
        out = {k: torch.cat([x[0], x[1]], dim=0) for k, x in zip(names, arrs)}
        v1 = usable_mask.to(torch.float32)
        if use_opponent_data == "direct":
            w1 = v1.clone()
        else:
            ratio = (off_policy_ratio if use_opponent_data == "off_policy" else total_ratio).to(torch.float32)
            w1 = torch.where(usable_mask, ratio, torch.zeros_like(ratio))
        out.update(states=torch.cat([states0, shadow_state0], dim=0), valid=torch.cat([ones, v1]), weights=torch.cat([ones, w1]),
                   nseq=2 * int(nenv))
    out.update(usable_index=usable, useful_ratio=float(usable.numel()) / float(neglogpacs[1].numel()))
    return out


def check_recurrent_reuse(opponent_mode, comm, device_mode=True):
    """What opponent-data reuse refuses for a recurrent learner, checked before the first rollout (``device_mode``: the Runner's)."""
    if opponent_mode == "fix":
        raise NotImplementedError("recurrent policies: opponent-data reuse needs a self-play opponent (the learner carries a shadow state "
                                  "along agent 1's stream); opponent_mode='fix' (policy-zoo nets, leagues) is not supported with it")
    if comm is not None:
        raise NotImplementedError("recurrent policies: opponent-data reuse runs on a single GPU (no comm)")
    if not device_mode:
        raise NotImplementedError("recurrent policies: opponent-data reuse needs a device-mode Runner (SumoVecEnv and LstmPPOModel)")


def selection_probs(action_prob, new_action_probs):
    """alg_ppo.py:237-242: mean |new/old - 1| of the candidates' ``action_probability`` outputs on the last rollout's opponent
    samples, normalised to sampling probabilities (uniform when every candidate equals the current opponent)."""
    import torch

    def score(nap):
        r = nap / action_prob - 1.0
        r = r[torch.isfinite(r)]           # a probability that underflowed to 0 in float32 (sharp late-training policies) gives inf / NaN here;
        return float(r.abs().mean().item()) if r.numel() else 0.0      # the reference would pass NaN to np.random.choice and stop -- those samples are left out
    return selection_probs_from_scores(np.array([score(nap) for nap in new_action_probs]))


def install_fixed_opponent(runner, fix_opponent_path, ac_dim, dev, seed):
    """``opponent_mode='fix'`` (alg_ppo.py:194-206, alg_ac.py:175-189): a policy-zoo net (MLP or LSTM: the file's length selects
    the family) plays agent 1 for the whole run.  A list or tuple of files is a LEAGUE (``policy_zoo.ZooLeague``): every 16-env
    tile faces one of them, re-dealt per update by :func:`assign_league`; its one noise generator is seeded as the single net's."""
    from .policy_zoo import FixedOpponentModel, load_zoo_league, load_zoo_policy
    if fix_opponent_path is None:
        raise ValueError("opponent_mode='fix' needs fix_opponent_path=<policy_zoo .npy> (reference default: "
                         "robosumo/robosumo/policy_zoo/assets/ant/mlp/agent-params-v3.npy)")
    if isinstance(fix_opponent_path, (list, tuple)):
        env = runner.env
        if hasattr(env, "_gs") and any((env._gs(g).start % 16 or env._gs(g).stop % 16) for g in range(getattr(env, "groups", 1))):
            raise ValueError("a league deals its members over 16-env tiles: the env groups must start and end on multiples of 16")
        zoo = load_zoo_league(fix_opponent_path, ac_dim, runner.nenv, device=dev)
    else:
        zoo = load_zoo_policy(fix_opponent_path, ac_dim, device=dev)
    zoo.seed(seed)
    runner.models[1] = FixedOpponentModel(zoo)


def assign_league(runner, update):
    """Start of an update in fix mode: a league re-deals its members over the env tiles, rotated by one tile per update (no-op for
    a single zoo net).  Returns the league or None."""
    from .policy_zoo import ZooLeague
    zoo = getattr(runner.models[1], "act_model", None)
    if type(zoo) is not ZooLeague:
        return None
    zoo.assign(update - 1)
    return zoo


def league_note(history, runner, league):
    """After a rollout against a league: append the update's per-member tally (episodes, learner wins, losses, draws as
    ``policy_zoo.league_scores`` estimates them from the episode returns) and the tile assignment to ``history``; returns the learner's win rate per member for the log line."""
    if league is None:
        return ""
    sc = runner.league_scores          # None where the Runner kept no tally (host mode: the episode records are the env's dicts)
    history["league_scores"].append(None if sc is None else sc.tolist())
    history["league_tiles"].append([int(x) for x in league.tile_member])
    if sc is None:
        return ""
    rates = ["%d:%s" % (k, "%.2f" % (row[1] / row[0]) if row[0] else "-") for k, row in enumerate(sc)]
    return "  [league win rate, estimated from returns, %s]" % " ".join(rates)


def check_opponent_pool(opponent_mode, runner, fused):
    """What ``opponent_pool`` > 1 refuses; ``fused``: the pool is read by the fused rollout launch (MLP policies)."""
    if opponent_mode == "fix":
        raise ValueError("opponent_pool > 1 makes no sense with a fixed opponent")
    if fused and not runner.fused_ok():
        raise NotImplementedError("opponent_pool > 1 with MLP policies runs inside the fused rollout launch (SUMO_FUSED_ROLLOUT != 0)")


def check_fused_selector(network, opponent_mode, model_fn):
    """What ``fused_selector=True`` refuses, before anything touches the env or the device: the selector's table holds MLP(64,64)
    policies as flat parameter vectors and serves the 'ours' mode, the only one that scores candidates."""
    if network == "lstm":
        raise ValueError("fused_selector scores MLP(64,64) checkpoints: not available with network='lstm'")
    if opponent_mode != "ours":
        raise ValueError("fused_selector serves opponent_mode='ours' (the other modes score no candidates); got %r" % (opponent_mode,))
    if model_fn is not None and not (isinstance(model_fn, type) and issubclass(model_fn, PPOModel)):
        raise ValueError("fused_selector needs models with a flat ``params`` vector (PPOModel and its subclasses), not a custom model_fn")


def upload(dev, *arrays):
    """The arrays of a host-mode Runner (recurrent models), moved to the device so that the update continues there like the MLP path."""
    import torch
    return [torch.as_tensor(np.ascontiguousarray(x)).to(dev) for x in arrays]


def env_fault_delta(env, prev, history):
    """The engine's fault counters of one update (the reference is loud here: a MuJoCo warning raises MujocoException, mujoco-py
    builder.py:351-369; the fused launch's abort already raised in Runner.run): diverged env steps (episodes ended by the bad-value
    guard), contacts dropped for lack of room, aborted hand-over waits.  ``prev``: ``env.stats()`` at the end of the previous update
    (None: the env keeps no counters).  Appends the three deltas to ``history``; returns (stats now, note for the log line or "")."""
    if prev is None:
        return None, ""
    now = env.stats()
    dv, dc = now["diverged"] - prev["diverged"], now["dropped"] - prev["dropped"]
    ab = now["rollout_aborts"] + now.get("handover_mismatches", 0) - prev["rollout_aborts"] - prev.get("handover_mismatches", 0)
    history["env_diverged"].append(int(dv)); history["env_dropped_contacts"].append(int(dc)); history["env_rollout_aborts"].append(int(ab))
    note = "  [env: %d diverged steps, %d dropped contacts, %d rollout aborts]" % (dv, dc, ab) if dv or dc or ab else ""
    return now, note


def choose_opponents(opponent_mode, update, npaths, K, score_fn=None):
    """(shared; pure) ``K`` of the ``npaths`` checkpoints for agent 1 (alg_ppo.py:217-244; 'latest': fewer where fewer exist).  Draws from numpy's
    global stream: 'random' over ``range(update)``, 'ours' the 30-subset if there are more, then by the probabilities ``score_fn(subset)`` returns."""
    if opponent_mode == "random":
        return [int(x) for x in np.random.choice(update, K)]
    if opponent_mode == "latest":
        return list(range(npaths - 1, max(-1, npaths - 1 - K), -1))
    if opponent_mode == "ours":                                          # ratio-divergence sampling (:227-244)
        sub = np.sort(np.random.choice(npaths, 30, replace=False)) if npaths > 30 else np.arange(npaths)
        rd = score_fn(sub)
        return [int(sub[j]) for j in np.random.choice(len(rd), K, p=rd)]
    raise ValueError("opponent_mode %r" % (opponent_mode,))


def candidate_probs(paths, sub, *, ref, opponent_data, selector, model_util):
    """The ``score_fn`` of 'ours': sampling probabilities of the candidates ``paths[i], i in sub`` against the opponent ``ref`` on the last
    rollout's opponent samples -- one launch over the selector's table, or candidate by candidate through the scratch ``model_util``."""
    obs, actions = opponent_data
    if selector is not None:
        selector.ensure(paths, sub)
        return selection_probs_from_scores(selector.scores(ref.params, sub, obs, actions))
    ap = ref.act_model.action_probability(obs, given_action=actions)
    naps = []
    for i in sub:
        model_util.load(paths[i])
        naps.append(model_util.act_model.action_probability(obs, given_action=actions))
    return selection_probs(ap, naps)


def install_opponents(opp_ref, pool, files):
    """(shared) The chosen checkpoint files into place: the first into the single reference opponent (agent 1 itself without an LSTM pool),
    file k into pool slot k, and the envs (16-env tiles) dealt over those slots round robin."""
    opp_ref.load(files[0])
    if pool is not None:
        for k, f in enumerate(files):
            pool.set_snapshot(k, f)
        pool.assign_round_robin(range(len(files)))


def select_opponents(update, opponent_mode, checkdir, opp_ref, pool, history, score_fn, comm, dev):
    """Self-play selection of one update (alg_ppo.py:207-247): 00000 at update 1, then ``choose_opponents`` over the checkpoint
    directory; rank 0 decides and everyone loads the same files.  ``version_gap`` grows at update 1 and in 'random' mode only."""
    if update == 1:
        paths, choices = [osp.join(checkdir, "00000")], [0]
        history["version_gap"].append(0)
    else:
        paths = sorted(osp.join(checkdir, f) for f in os.listdir(checkdir))
        K = pool.capacity if pool is not None else 1
        choices = choose_opponents(opponent_mode, update, len(paths), K, lambda sub: score_fn(paths, sub))
        if opponent_mode == "random":
            history["version_gap"].append(update - 1 - choices[0])
        if comm is not None:                                             # rank 0 decides, everyone loads the same files
            import torch
            c = torch.tensor(choices + [-1] * (K - len(choices)), device=dev)
            torch.distributed.broadcast(c, 0, group=comm)
            choices = [int(x) for x in c.tolist() if x >= 0]
    history["opponent_versions"].append(list(choices))
    install_opponents(opp_ref, pool, [paths[c] for c in choices])


Rollout = namedtuple("Rollout", "obs returns masks actions values neglogpacs rewards opponent_neglogpacs opp_obs_s opp_act_s states epinfos "
                                "off_policy_ratio off_env_ratio total_ratio")         # what Runner.run returns, in its order


def collect_rollout(runner, update, dev, tstart):
    """One rollout, left on the device (a host-mode Runner's arrays are moved there).  Returns (Rollout, seconds since ``tstart``)."""
    import torch
    ro = Rollout(*runner.run(update))
    torch.cuda.synchronize(dev)
    t_roll = time.perf_counter() - tstart
    if isinstance(ro.obs, np.ndarray):       # host-mode Runner (recurrent models): continue on the device like the MLP path
        names = [n for n in Rollout._fields if n not in ("opp_obs_s", "opp_act_s", "states", "epinfos")]
        ro = ro._replace(**dict(zip(names, upload(dev, *[getattr(ro, n) for n in names]))))
    return ro, t_roll


def clean_and_assemble(ro, history, *, rho_bar, recurrent, shadow_state0, nenvs, nbatch, neglogp_threshold, use_opponent_data, vgap):
    """Ratio hygiene (alg_ppo.py:258-280), then the usable opponent samples, the batch and its weights (:286-344); ``obs`` comes back
    contiguous.  A recurrent learner's batch also carries ``states``, ``nseq`` and ``valid`` (None without opponent-data reuse)."""
    import torch
    clean = {}
    for name in ("off_policy_ratio", "off_env_ratio", "total_ratio"):
        clean[name], m, f = clean_ratio(getattr(ro, name), rho_bar)
        history[name + "_mean"].append(m); history[name + "_clip_frac"].append(f)
    kw = dict(neglogp_threshold=neglogp_threshold, use_opponent_data=use_opponent_data, vgap=vgap,
              version_gap=history["version_gap"][-1] if history["version_gap"] else None)      # its last entry, whatever the mode
    if recurrent and use_opponent_data is not None:
        ub = assemble_recurrent_update_batch(*ro[:7], clean["off_policy_ratio"], clean["total_ratio"], ro.states, shadow_state0, nenv=nenvs, **kw)
    else:
        ub = assemble_update_batch(*ro[:7], clean["off_policy_ratio"], clean["total_ratio"], nbatch=nbatch, **kw)
        if recurrent:
            st0 = ro.states if torch.is_tensor(ro.states) else torch.as_tensor(np.asarray(ro.states, np.float32)).to(ro.returns.device)
            ub.update(states=st0, nseq=nenvs, valid=None)
    history["useful_ratio"].append(ub["useful_ratio"])
    ub["obs"] = ub["obs"].contiguous()
    return ub


def optimise_recurrent(model, ub, lrnow, cliprangenow, *, nsteps, nminibatches, noptepochs, dev):
    """Minibatch SGD of a recurrent learner, baselines ppo2 convention: minibatches of whole env sequences, each with its own start state
    and masks; under opponent-data reuse agent 1's sequences follow agent 0's and the row mask ``valid`` goes along (a minibatch without
    a valid row steps on a zero gradient, LstmPPOModel.train).  Returns (mean loss row, None): no KL early stop here."""
    import torch
    nseq, valid = ub["nseq"], ub["valid"]
    rows = [ub[k] for k in ("obs", "returns", "masks", "actions", "values", "neglogpacs")]
    envsperbatch = nseq // nminibatches
    envinds = np.arange(nseq)
    flatinds = np.arange(nseq * nsteps).reshape(nseq, nsteps)
    mblossvals = []
    for epoch in range(noptepochs):
        np.random.shuffle(envinds)
        for start in range(0, nseq, envsperbatch):
            mbenv = envinds[start:start + envsperbatch]
            mbflat = torch.from_numpy(flatinds[mbenv].ravel()).to(dev)
            kw = dict(valid=valid[mbflat]) if valid is not None else {}
            out = model.train(lrnow, cliprangenow, *[x[mbflat] for x in rows], None, ub["weights"][mbflat],
                              ub["states"][torch.from_numpy(mbenv).to(dev)], nsteps=nsteps, **kw)
            mblossvals.append(torch.tensor([float(x) for x in out[:5]], dtype=torch.float64))
    return torch.stack(mblossvals).mean(dim=0).cpu().numpy().astype(np.float64), None


def optimise_indexed(model, ub, lrnow, cliprangenow, *, nbatch_train, noptepochs, kl_threshold, shuffle_gen, comm, dev):
    """Minibatch SGD of an MLP learner (alg_ppo.py:355-398): the batch is handed over once and every step gathers its rows by index
    inside the gradient kernel.  Returns (mean loss row, [epoch, minibatch] of the KL early stop or None)."""
    import torch
    batch = [ub[k] for k in ("obs", "returns", "actions", "values", "neglogpacs", "weights")]
    if hasattr(model, "begin_update"):
        model.begin_update(*batch)                                       # the update's batch, handed over once (model.py)
    # minibatch steps per epoch (alg_ppo.py:378): with opponent-data reuse the ranks hold different numbers of rows, so they
    # agree on the largest count and short ranks finish the epoch with empty minibatches (same collectives on every rank)
    nsamp = batch[0].shape[0]
    nmb_steps = -(-nsamp // nbatch_train)
    if comm is not None and not model.equal_counts:
        nmb_steps = sdist.agree_max(nmb_steps, comm, device=dev)
    mblossvals, stop_info = [], None
    for epoch in range(noptepochs):
        inds = torch.randperm(nsamp, device=dev, generator=shuffle_gen).to(torch.int32)   # np.random.shuffle (:375), on the device
        if comm is not None and hasattr(model, "prepare_epoch"):
            # equal shards: the advantage moments of all the epoch's minibatches in ONE all-reduce, so that every optimiser step
            # issues exactly one collective; a no-op with opponent-data reuse (unequal shards)
            model.prepare_epoch(inds, nbatch_train)
        for ii in range(nmb_steps):
            mb = inds[ii * nbatch_train:(ii + 1) * nbatch_train]       # empty once this rank's rows are used up
            # statistics stay on the device unless the KL early stop needs them now (alg_ppo.py:389-398)
            out = model.train_indexed(lrnow, cliprangenow, *batch, mb, int(mb.numel()), sync=kl_threshold is not None, mb_index=ii)
            mblossvals.append(out[:5] if kl_threshold is not None else out)
            if kl_threshold is not None and out[3] > kl_threshold * 1.5:
                stop_info = [epoch, ii]
                break
        if stop_info is not None:
            break
    if hasattr(model, "end_update"):
        model.end_update()
    if kl_threshold is None:                                             # device rows: one transfer for the update
        return torch.stack(mblossvals).mean(dim=0).cpu().numpy().astype(np.float64), stop_info
    return np.mean(np.array(mblossvals, dtype=np.float64), axis=0), stop_info


def save_checkpoint(model, checkdir, name, selector=None):
    """(shared) ``checkdir/name``, and its row of the fused selector's table where there is one."""
    path = osp.join(checkdir, name)
    model.save(path)
    if selector is not None:
        selector.note_saved(sorted(os.listdir(checkdir)).index(name), model, path)


def report_update(update, middle, ub, lossvals, epinfos, env_stats_prev, time_elapsed, *, nupdates, nsteps, nbatch, env, runner, league,
                  history, model, report, epinfobuf, update_fn, log_interval, verbose, save_interval, checkdir, selector=None, rank=0,
                  comm=None, resume_save=None):
    """(shared) The tail of an update: the engine's fault counters and the league's tally into ``history``, ``update_fn``, the run log and
    the evaluation (``report``, rank 0's), the printed line around the learner's own ``middle``, the checkpoint and, with ``comm``, the
    check that all ranks hold the same weights; last of all ``resume_save(update)``, which writes the resume state where one is due
    (resume.py).  ``nbatch`` counts all ranks.  Returns ``env.stats()``: the next ``env_stats_prev``."""
    env_stats, env_note = env_fault_delta(env, env_stats_prev, history)
    lg_note = league_note(history, runner, league)
    if update_fn is not None:
        update_fn(update)
    log_now = update % log_interval == 0 or update == 1
    logged = report is not None and report.update(update, nupdates, update * nbatch, epinfos)       # evaluates where due; is a row of the run log due?
    if rank == 0 and (logged or (verbose and log_now)):
        ev = explained_variance(ub["values"].cpu().numpy(), ub["returns"].cpu().numpy())
    if logged:
        report.log(update=update, nsteps=nsteps, nbatch=nbatch, explained_variance=ev, epinfobuf=epinfobuf, time_elapsed=time_elapsed,
                   lossvals=lossvals, league=league)
    if verbose and rank == 0 and log_now:
        print("update %d/%d  %s  ev %.3f  eprewmean %.2f  eplenmean %.1f  %s" % (
            update, nupdates, middle, ev, safemean([e["r"] for e in epinfobuf]), safemean([e["l"] for e in epinfobuf]),
            " ".join("%s %.4g" % (n, v) for n, v in zip(model.loss_names, lossvals))) + lg_note + env_note, flush=True)
    elif env_note and rank == 0:
        print("update %d/%d%s" % (update, nupdates, env_note), flush=True)
    if save_interval and (update % save_interval == 0 or update == 1) and rank == 0:
        save_checkpoint(model, checkdir, "%.5i" % update, selector)       # alg_ppo.py:459-464
    if comm is not None:
        import torch
        sdist.assert_synced(model.params, comm)                           # MpiAdamOptimizer.check_synced (mpi_adam_optimizer.py:54-67)
        torch.distributed.barrier(comm)
    if resume_save is not None:
        resume_save(update)
    return env_stats


def learn(*, network, env, total_timesteps, opponent_mode="ours", use_opponent_data=None, eval_env=None, seed=None, nsteps=2048,
          ent_coef=0.0, lr=3e-4, vf_coef=0.5, max_grad_norm=0.5, gamma=0.99, lam=0.95, rho_bar=1.0, c_bar=1.0, log_interval=10,
          nminibatches=4, noptepochs=4, cliprange=0.2, save_interval=1, load_path=None, model_fn=None, update_fn=None, init_fn=None,
          nagent=1, anneal_bound=500, vgap=None, kl_threshold=None, neglogp_threshold=10000.0, log_dir=None, comm=None,
          verbose=True, fix_opponent_path=None, opponent_pool=1, fused_fix_opponent=False, fused_selector=False, selector_table_mb=1024,
          run_log=False, eval_interval=0, eval_opponents=None, eval_trials=64, eval_num_env=64, eval_deterministic=True, eval_seed=0,
          eval_cross_family=False, resume_interval=0, resume=False, **network_kwargs):
    """``resume_interval=k`` writes the run's whole state into ``log_dir/resume/state.pt`` after every k-th update and after the last;
    ``resume=True`` continues from that file -- the same checkpoints, history and run-log rows as the uninterrupted run, bit for bit --
    or starts from update 1 where there is none (resume.py).  Single GPU, no ``opponent_pool`` / ``fused_selector`` /
    mixed match-up; a custom ``model_fn`` must be a ``learner.Learner`` subclass (or a ``functools.partial`` of one).
    ``run_log=True`` writes the run's files into ``log_dir`` (runlog.py); ``eval_interval`` / ``eval_opponents`` make rank 0 play the
    live learner against fixed opponents every so many updates (train_eval.py), on ``eval_env`` (the reference's parameter) or on
    an env of its own.  With the defaults neither happens and the run writes and draws exactly what it did without them."""
    # a mixed match-up (the two sides differ) trains in fix mode only, through mixed.MixedRunner; the other modes meet the Runner's refusal
    from . import mixed
    resume_interval = int(resume_interval or 0)
    zoo_net = network == "zoo_mlp"      # fine-tune a policy-zoo MLP net (zoo_learner.py); everything it cannot do is refused here, before the device
    if zoo_net:
        from . import zoo_learner
        zoo_learner.check_learn(env, opponent_mode=opponent_mode, opponent_pool=opponent_pool, fused_selector=fused_selector,
                                fused_fix_opponent=fused_fix_opponent, eval_interval=eval_interval, eval_opponents=eval_opponents, comm=comm,
                                resume=resume, resume_interval=resume_interval, load_path=load_path, zoo_init=network_kwargs.get("zoo_init"))
    if resume or resume_interval:                                        # refused before anything touches the device
        if resume_interval < 0:
            raise ValueError("resume_interval must be >= 0 (0: no resume state is written), got %d" % resume_interval)
        resume_state.check_supported(env=env, opponent_mode=opponent_mode, comm=comm, opponent_pool=opponent_pool,
                                     fused_selector=fused_selector, model_fn=model_fn)
    mixed_env = mixed.is_mixed(env) and opponent_mode == "fix"
    if mixed_env:
        mixed.check_learn(env, network=network, opponent_mode=opponent_mode, use_opponent_data=use_opponent_data, opponent_pool=opponent_pool,
                          fused_fix_opponent=fused_fix_opponent, fused_selector=fused_selector, eval_interval=eval_interval,
                          eval_opponents=eval_opponents, comm=comm)
        from . import zoo_pairs
        zoo_seat = zoo_pairs.seat_for(env, 1, mixed.fix_paths(fix_opponent_path))     # a file of another species is refused here
    if fused_selector:
        check_fused_selector(network, opponent_mode, model_fn)
    # evaluation: everything unsupported is refused here, before anything touches the device (None: evaluation is off)
    eval_plan = train_eval.plan_for(env, network, network_kwargs, eval_env=eval_env, eval_interval=eval_interval, eval_opponents=eval_opponents,
                                    eval_trials=eval_trials, eval_num_env=eval_num_env, eval_cross_family=eval_cross_family)
    import torch
    if seed is not None:                                                # set_global_seeds (misc_util.py:48-62)
        np.random.seed(seed)
        torch.manual_seed(seed)
    lr = constfn(lr) if isinstance(lr, float) else lr
    cliprange = constfn(cliprange) if isinstance(cliprange, float) else cliprange
    total_timesteps = int(total_timesteps)
    rank, world = (0, 1) if comm is None else (torch.distributed.get_rank(comm), torch.distributed.get_world_size(comm))
    log_dir = log_dir or os.environ.get("OPENAI_LOGDIR") or "/tmp/robosumo_selfplay_amd"
    saved = fingerprint = None          # resume.py: the state to continue from; what a state file of this run opens with
    if resume or resume_interval:
        fingerprint = resume_state.fingerprint(env=env, nsteps=nsteps, total_timesteps=total_timesteps, network=network,
                                               network_kwargs=network_kwargs, opponent_mode=opponent_mode, use_opponent_data=use_opponent_data,
                                               seed=seed, nminibatches=nminibatches, noptepochs=noptepochs, lr=lr, cliprange=cliprange,
                                               fix_opponent_path=fix_opponent_path)
    if resume:
        saved = resume_state.read_state(log_dir)                         # a file that does not load is refused by name
        if saved is None:
            print("resume: no state file %s, starting from update 1" % resume_state.state_path(log_dir), flush=True)
        else:
            resume_state.check_fingerprint(saved["fingerprint"], fingerprint, resume_state.state_path(log_dir))
    policy = build_policy(env, network, **network_kwargs)
    nenvs = env.num_envs
    ob_space, ac_space = env.observation_space[0], env.action_space[0]
    nbatch = nenvs * nsteps
    nbatch_train = nbatch // nminibatches
    recurrent = network == "lstm"
    if recurrent:
        from .lstm_model import LstmPPOModel
        if use_opponent_data is not None:
            if use_opponent_data not in ("direct", "off_policy", "both"):
                raise ValueError("use_opponent_data %r" % (use_opponent_data,))
            check_recurrent_reuse(opponent_mode, comm)
        assert nenvs % nminibatches == 0, "recurrent minibatches are whole env sequences: nenvs %% nminibatches must be 0"
    model_fn = model_fn or (LstmPPOModel if recurrent else zoo_learner.ZooPPOModel if zoo_net else PPOModel)
    dev = getattr(env, "device", torch.device("cuda", 0))
    mk = lambda scope, trainable: model_fn(policy=policy, ob_space=ob_space, ac_space=ac_space, nbatch_act=nenvs,
                                           nbatch_train=nbatch_train, nsteps=nsteps, ent_coef=ent_coef, vf_coef=vf_coef,
                                           max_grad_norm=max_grad_norm, trainable=trainable, model_scope=scope, device=dev.index or 0,
                                           comm=comm if trainable else None)
    model = mk("model_0", True)
    model.equal_counts = use_opponent_data is None      # opponent-data reuse makes per-rank minibatch sizes differ
    sdist.broadcast_params(model.params, comm)                          # sync_from_root (ppo2/model.py:129-131)
    models = [model] + [mk("model_%d" % i, False) for i in range(1, 1 if mixed_env else nagent)]   # a mixed match-up has no second net of the learner's shape
    checkdir = osp.join(log_dir, "checkpoints")
    nupdates = total_timesteps // nbatch
    selector = model_util = None
    if mixed_env:
        pass                                                             # no candidates to score
    elif not fused_selector:
        model_util = mk("model_util", False)
    else:
        # the candidates live in a device table and are scored in one launch (policy_selector.py); no scratch model is built, but the
        # initial-weight draws that PPOModel's own constructor makes (one init_param_list) are still taken from numpy's global stream,
        # so with PPOModel both settings make the same opponent draws.  A subclass whose constructor draws more than that passes
        # check_fused_selector but loses this alignment: its fused run is a valid run on another random stream.
        from .policy_selector import FusedSelector
        init_param_list(policy.ob_dim, policy.ac_dim)
        names = set(os.listdir(checkdir)) if osp.isdir(checkdir) else set()      # a run directory may already hold checkpoints
        # history mode takes its whole table (one row per checkpoint of the run, at most selector_table_mb) here, before the first update
        selector = FusedSelector(policy, dev, len(names | set("%.5i" % u for u in range(nupdates + 1))), table_mb=selector_table_mb)
    if rank == 0 and saved is None:                                     # (a resumed run keeps the 00000 it wrote)
        save_checkpoint(model, checkdir, "00000", selector)              # alg_ppo.py:122-123
    if comm is not None:
        torch.distributed.barrier(comm)
    if load_path is not None:
        for m in models:
            m.load(load_path)
    for i, m in enumerate(models):
        m.act_model.seed((seed or 0) * 1000 + 17 * i + rank)
    if mixed_env:     # agent 1's noise generator is seeded as install_fixed_opponent seeds a zoo net
        runner = mixed.MixedRunner(env, model, zoo_seat, nsteps, gamma, lam, anneal_bound, seat_seed=(seed or 0) * 1000 + 17 + rank)
    else:
        runner = Runner(env=env, models=models, nsteps=nsteps, nagent=nagent, gamma=gamma, lam=lam, rho_bar=rho_bar, c_bar=c_bar,
                        anneal_bound=anneal_bound)
    # opt-in: in opponent_mode='fix' the zoo net (MLP or LSTM) plays inside the fused rollout launch (Runner.fused_fix_opponent: another noise stream)
    runner.fused_fix_opponent = bool(fused_fix_opponent)
    if recurrent and use_opponent_data is not None:       # the learner carries a shadow state along agent 1's stream (Runner.reuse_opponent)
        check_recurrent_reuse(opponent_mode, comm, runner.device_mode)
        runner.reuse_opponent = True
    # opponent_pool = K > 1 (extension, BASELINE config 5): K frozen snapshots stay resident in HBM and every env plays against its own
    # one (opponent_pool.py); each update draws K snapshots by the selection law of ``opponent_mode`` instead of one.  K = 1 is the
    # reference: one snapshot for all parallel envs (alg_ppo.py:213-214).
    pool = None
    # the single-snapshot opponent: every selection loads its first choice here and the 'ours' selector scores against it.  It is agent
    # 1 itself unless an LSTM pool takes that seat below (alg_ppo.py:208: it holds 00000 when update 2 scores the opponent update 1 faced)
    opp_ref = None if mixed_env else runner.models[1]
    if int(opponent_pool) > 1:
        check_opponent_pool(opponent_mode, runner, fused=not recurrent)
        from .opponent_pool import LstmOpponentPool, OpponentPool
        pool = (LstmOpponentPool if recurrent else OpponentPool)(policy, int(opponent_pool), nenvs, dev)
        if recurrent:
            pool.seed((seed or 0) * 1000 + 17 + rank)
            runner.models[1] = pool           # acts for agent 1 and scores agent 0's actions, each env tile with its own snapshot
        else:
            runner.opponent_pool = pool
    epinfobuf = deque(maxlen=100)
    shuffle_gen = torch.Generator(device=dev)
    shuffle_gen.manual_seed((seed or 0) * 7919 + 13)          # same minibatch order on every rank (equal shards)
    # the optimiser phase, resolved once: whole-sequence minibatches for a recurrent learner, row-indexed ones for an MLP learner
    optimise = partial(optimise_recurrent, nsteps=nsteps, nminibatches=nminibatches, noptepochs=noptepochs, dev=dev) if recurrent else partial(
        optimise_indexed, nbatch_train=nbatch_train, noptepochs=noptepochs, kl_threshold=kl_threshold, shuffle_gen=shuffle_gen, comm=comm, dev=dev)
    if init_fn is not None:
        init_fn()
    tfirststart = time.perf_counter()
    history = dict(version_gap=[], off_policy_ratio_mean=[], off_env_ratio_mean=[], total_ratio_mean=[], off_policy_ratio_clip_frac=[],
                   off_env_ratio_clip_frac=[], total_ratio_clip_frac=[], useful_ratio=[], opponent_versions=[], ppo_clip_frac=[],
                   approxkl=[], early_stop_info=[], lossvals=[], fps=[], rollout_s=[], update_s=[],
                   env_diverged=[], env_dropped_contacts=[], env_rollout_aborts=[],     # per update, from the engine's counters
                   league_scores=[], league_tiles=[])       # fix mode with a list of files: per update and member (league_note)
    env_stats = env.stats() if hasattr(env, "stats") else None
    # rank 0 reports: the evaluator loads its opponents here, once (the other ranks meet it at the loop's barrier)
    report = train_eval.Report(run_log=run_log, plan=eval_plan, log_dir=log_dir, env=env, model=model, history=history, eval_env=eval_env,
                               deterministic=eval_deterministic, seed=eval_seed, first_checkpoint=osp.join(checkdir, "00000"),
                               log_interval=log_interval, verbose=verbose, opponent_mode=opponent_mode,
                               resume_log=saved["run_log"] if saved is not None else None) if rank == 0 else None
    tail = dict(nupdates=nupdates, nsteps=nsteps, nbatch=nbatch * world, env=env, runner=runner, history=history, model=model, report=report,
                epinfobuf=epinfobuf, update_fn=update_fn, log_interval=log_interval, verbose=verbose, save_interval=save_interval,
                checkdir=checkdir, selector=selector, rank=rank, comm=comm)
    opponent_data = league = None
    first_update = 1
    if saved is not None:
        # set-up has built the same objects as ever; the saved state now overwrites what it drew, and the loop goes on after the saved update
        if opponent_mode == "fix":                                       # what update 1 installs
            install_fixed_opponent(runner, fix_opponent_path, ac_space.shape[0], dev, (seed or 0) * 1000 + 17 + rank)
        resume_state.drop_later_checkpoints(checkdir, saved["update"])
        done, opponent_data = resume_state.apply(saved, runner=runner, env=env, shuffle_gen=shuffle_gen, epinfobuf=epinfobuf, history=history,
                                                 device=dev)
        env_stats = env.stats()                                          # the restored engines count their own faults, from here
        report.resumed()
        tfirststart = time.perf_counter() - saved["time_elapsed"]
        first_update = done + 1
        if verbose:
            print("resume: continuing after update %d/%d from %s" % (done, nupdates, resume_state.state_path(log_dir)), flush=True)

    def resume_save(update):
        """The state after ``update`` into log_dir/resume/state.pt, where one is due; agent 1's rows only where the next selection reads them."""
        if update % resume_interval == 0 or update == nupdates:
            resume_state.write_state(log_dir, resume_state.capture(
                fingerprint=fingerprint, update=update, runner=runner, env=env, shuffle_gen=shuffle_gen,
                opponent_data=opponent_data if opponent_mode == "ours" else None, epinfobuf=epinfobuf, history=history,
                time_elapsed=time.perf_counter() - tfirststart, run_log=report.log_state(), device=dev))
    if resume_interval:
        tail["resume_save"] = resume_save
    for update in range(first_update, nupdates + 1):
        assert nbatch % nminibatches == 0
        tstart = time.perf_counter()
        frac = 1.0 - (update - 1.0) / nupdates
        lrnow, cliprangenow = lr(frac), cliprange(frac)
        # ---- opponent selection (alg_ppo.py:191-247)
        if mixed_env:                                                    # the seat's nets re-dealt over the tiles; there is no version to choose
            league = runner.assign(update)
            history["version_gap"].append(0); history["opponent_versions"].append(list(range(len(zoo_seat))))
        elif opponent_mode == "fix":                                     # alg_ppo.py:194-206: a policy-zoo net
            if update == 1:
                install_fixed_opponent(runner, fix_opponent_path, ac_space.shape[0], dev, (seed or 0) * 1000 + 17 + rank)
            league = assign_league(runner, update)
        else:
            select_opponents(update, opponent_mode, checkdir, opp_ref, pool, history, partial(
                candidate_probs, ref=opp_ref, opponent_data=opponent_data, selector=selector, model_util=model_util), comm, dev)
        # ---- rollout; agent 1's (obs, action) rows, env-major, are the 'ours' selector's data of the next update
        ro, t_roll = collect_rollout(runner, update, dev, tstart)
        opponent_data = (ro.obs[1], ro.actions[1])
        # ---- ratio hygiene, usable opponent samples, batch assembly, weights (alg_ppo.py:258-344)
        ub = clean_and_assemble(ro, history, rho_bar=rho_bar, recurrent=recurrent, shadow_state0=runner.shadow_state0, nenvs=nenvs,
                                nbatch=nbatch, neglogp_threshold=neglogp_threshold, use_opponent_data=use_opponent_data, vgap=vgap)
        epinfobuf.extend(ro.epinfos[-epinfobuf.maxlen:])                 # the deque keeps the last 100 anyway (alg_ppo.py:160,347)
        # ---- minibatch SGD (alg_ppo.py:355-398)
        lossvals, stop_info = optimise(model, ub, lrnow, cliprangenow)
        history["early_stop_info"].append(stop_info); history["lossvals"].append(lossvals)
        history["ppo_clip_frac"].append(lossvals[-1]); history["approxkl"].append(lossvals[-2])
        torch.cuda.synchronize(dev)
        tnow = time.perf_counter()
        history["rollout_s"].append(t_roll); history["update_s"].append(tnow - tstart - t_roll)
        history["fps"].append(nbatch * world / (tnow - tstart))
        # ---- report: counters, run log, evaluation, the printed line, checkpoint
        middle = "fps %.0f  rollout %.2fs  sgd %.2fs" % (history["fps"][-1], t_roll, tnow - tstart - t_roll)
        env_stats = report_update(update, middle, ub, lossvals, ro.epinfos, env_stats, tnow - tfirststart, league=league, **tail)
    if report is not None:
        report.close()
    model.history = history
    model.time_elapsed = time.perf_counter() - tfirststart
    return model
