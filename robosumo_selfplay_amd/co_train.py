"""Two species trained against each other on a MIXED match-up (``RoboSumo-Ant-vs-Bug-v0``, ...): both seats learn.

The reference cannot do this -- its Runner sizes both policies from ``observation_space[0]`` (runner.py:14-16).  Here both sides are
:class:`mixed.LearnerSeat` tables of MLP(64,64) rows.  :func:`pair_step` makes both seats' actions and rollout records of one step --
fused: ONE ``ppo_mixed_pair_step`` launch; ``fused=False``: the definition, ``mixed.learner_side_definition`` per side.
:class:`PairRunner` splits the 16-env tiles in two halves: in the first agent 0's live net meets agent 1's frozen checkpoint (these
envs train learner 0), in the second agent 0's frozen checkpoint meets agent 1's live net (they train learner 1).  :func:`learn` is
the reference's self-play law lifted to two species -- each side's frozen opponent is chosen from the OTHER side's checkpoint
directory -- over ``alg_ppo``'s named stages.  :func:`play_checkpoint_pairs` / :func:`compare_history_versions` play the two sides'
checkpoints against each other.
"""
import os
import os.path as osp
import time
from collections import deque

import numpy as np

from . import capi, matches, mixed, ppo_capi, zoo_pairs
from .mixed import LearnerSeat, RECORD_KEYS
from .policy_zoo import EVAL_ADJUST_Z, LEAGUE_TILE

PAIR_TILES = 2 * LEAGUE_TILE      # the envs come in pairs of tiles: one trains learner 0, one learner 1
ROW_SIDES = ("agent 0's row", "agent 1's row")


def tile_halves(nenvs):
    """The table row (0 = live learner, 1 = frozen checkpoint) every 16-env tile plays, per side: int32 ``(rows0, rows1)`` of
    ``[nenvs / 16]`` each.  Tiles ``[0, nenvs / 32)``: agent 0 live against agent 1 frozen; tiles ``[nenvs / 32, nenvs / 16)``:
    agent 0 frozen against agent 1 live."""
    nenvs = int(nenvs)
    if nenvs < PAIR_TILES or nenvs % PAIR_TILES:
        raise ValueError("co-training splits the 16-env tiles in two equal halves: num_envs = %d is not a multiple of %d" % (nenvs, PAIR_TILES))
    h = nenvs // PAIR_TILES
    rows0 = np.array([0] * h + [1] * h, np.int32)
    return rows0, (1 - rows0).astype(np.int32)


def own_envs(nenvs, side):
    """The envs that train learner ``side``: the half in which its live row plays."""
    h = int(nenvs) // 2
    return slice(side * h, (side + 1) * h)


def check_engine_fused(env, engine_fused, what, instead):
    """The fused launch evaluates the policies inside its launch, ``cfrc_mode='rne_post'`` fills the observations in a second launch per
    step: ``what`` on such an env is refused, before the device is touched, with a pointer to ``instead``."""
    if engine_fused and getattr(env, "cfrc_mode", "zero") != "zero":
        raise ValueError("%s is not available on an env with cfrc_mode=%r (its observations are completed by a second launch per step, "
                         "the fused launch reads them inside its own): use %s" % (what, env.cfrc_mode, instead))


def pair_step(env, seats, tile_rows, noise, records, fused=True, status=None, runs=None):
    """Both agents' actions of one step of a mixed match-up, each by a :class:`mixed.LearnerSeat` (``seats[s]`` fitted to agent s of
    ``env``), into ``env.act_dev``.  Per side s (each of the four arguments is a pair or None, and so is each entry):
    ``tile_rows[s]`` int32 CUDA [N / 16] (None = row 0 everywhere), ``noise[s]`` float32 [N][A_s] standard-normal rows (None = the
    means), ``records[s]`` the dict of ``mixed.mixed_step``'s ``record`` with that agent's own done flag, ``runs[s]`` the
    definition's runs of tiles sharing a row (default: read from ``tile_rows[s]``).  ``env``: a ``SumoVecEnv`` or a
    :class:`mixed.EnvRows` of one env group.

    ``fused``: one ``ppo_mixed_pair_step`` launch; a tile whose row names no table row writes nothing for that side and leaves
    ``ppo_capi.mixed_status(tile, side)`` in ``status`` (int32 CUDA [1], optional).  ``fused=False`` is the definition: per side
    ``ppo_forward`` per run and torch copies (``mixed.learner_side_definition``).  The two agree bit for bit."""
    pair = lambda x: (None, None) if x is None else tuple(x)
    tile_rows, noise, records, runs = pair(tile_rows), pair(noise), pair(records), pair(runs)
    if len(seats) != 2:
        raise ValueError("pair_step plays two seats, got %d" % len(seats))
    recs = []
    for s in range(2):
        mixed._check_mixed_step(seats[s], env, tile_rows[s], noise[s], records[s], side=s)
        rec = dict.fromkeys(RECORD_KEYS)
        rec.update(records[s] or {})
        recs.append(rec)
    if not fused:
        for s in range(2):
            mixed.learner_side_definition(env, seats[s], s, tile_rows[s], noise[s], recs[s], runs[s])
        return
    obs, act, done = env.obs_dev, env.act_dev, env.done_dev
    sides = (ppo_capi.PairSide * 2)()
    for s in range(2):
        p = sides[s]
        p.seat = seats[s].struct(tile_rows[s])
        p.obs, p.noise, p.done, p.action = obs[:, s].data_ptr(), ppo_capi.ptr(noise[s]), done[:, s].data_ptr(), act[:, s].data_ptr()
        r = p.record
        r.obs, r.action, r.neglogp, r.value, r.done = (ppo_capi.ptr(recs[s][k]) for k in RECORD_KEYS)
    ppo_capi.chk(ppo_capi.lib().ppo_mixed_pair_step(sides, env.num_envs, obs.stride(0), done.stride(0), act.stride(0), ppo_capi.ptr(status),
                                                    env._stream()))


def _group_runs(runs, tiles):
    """The runs of the tiles ``tiles`` (a slice), in that group's own tile numbers."""
    return [(max(a, tiles.start) - tiles.start, min(b, tiles.stop) - tiles.start, e) for a, b, e in runs if a < tiles.stop and b > tiles.start]


def running_episode_sums(rew, ep_done, carry):
    """Agent 1's episode figure: per-env running sums of ``rew`` [T][N] (its annealed reward) in float64, started from ``carry`` [N] (the
    open episodes' sums of the previous rollout) and restarted after every step whose ``ep_done`` [T][N] (bool) is set.  Returns
    (sums [T][N], whose entries at ``ep_done`` are the closed episodes' returns; the new carry [N])."""
    import torch
    sums = torch.empty(rew.shape, dtype=torch.float64, device=rew.device)
    acc = carry
    for s in range(rew.shape[0]):
        acc = acc + rew[s].double()
        sums[s] = acc
        acc = torch.where(ep_done[s], torch.zeros_like(acc), acc)
    return sums, acc


class PairRunner(object):
    """Device-mode rollouts of two MLP learners (``models[s]``, a ``PPOModel`` on agent s's spaces) against each other's frozen
    checkpoints on a mixed ``SumoVecEnv``.  Each side holds a 2-row device table: row 0 the live learner, copied from ``model.params``
    at the start of every :meth:`run`; row 1 that side's frozen checkpoint (:meth:`set_frozen`; the initial parameters until then).
    The tiles are split by :func:`tile_halves`, fixed for the run.  Per step and env group, on the group's stream: :func:`pair_step`
    (writing slice s of both sides' buffers), ``env.step_device[_group]``, ``ppo_post_step``.  The action noise is drawn ONCE per
    rollout and side, ``[T][N][A_s]`` from ``models[s].act_model.gen``, so the number of env groups does not change the numbers.

    Agent 0's episode records are ``ppo_post_step``'s (the env's monitor figure).  Agent 1's side has no monitor: its episode return
    is the running per-env sum of its ANNEALED reward ``rew[1]`` (what it is trained on, not the monitor's figure), carried
    across rollouts and closed where ``ep_done`` is set; the lengths are ``ep_l``.  ``fused``: the one-launch step; default from the
    environment, ``SUMO_MIXED_STEP=0`` selects the definition (same numbers, bit for bit).

    ``engine_fused``: the steps of a rollout run inside the engine's fused launch (``sumo_rollout_steps_pair``):
    per env group ONE launch of all ``nsteps`` steps on the group's stream, or launches of ``rollout_chunk`` steps each where that
    is > 0.  Both seats act in the wave that owns the env; each side records (and evaluates its value net) only on the half of the
    tiles its live row plays, so the other half of every side's record stays zero -- the halves a learner trains on, the env, the
    rewards and the episode records are the step-by-step path's, bit for bit.  Not available with ``cfrc_mode='rne_post'``."""

    def __init__(self, env, models, nsteps, gamma, lam, anneal_bound=500, fused=None, engine_fused=False, rollout_chunk=0):
        check_engine_fused(env, engine_fused, "PairRunner(engine_fused=True)", "engine_fused=False")
        import torch
        self._t = torch
        if not hasattr(env, "step_device"):
            raise ValueError("PairRunner is device mode only: it needs a SumoVecEnv")
        mixed.check_groups(env)
        rows = tile_halves(env.num_envs)
        ppo_capi.lib()
        self.env, self.models = env, list(models)
        if len(self.models) != 2:
            raise ValueError("PairRunner trains two models, got %d" % len(self.models))
        self.nenv, self.nsteps, self.gamma, self.lam, self.anneal_bound = env.num_envs, int(nsteps), gamma, lam, anneal_bound
        self.device = env.device
        D, A = env.model.obs_dims, env.model.act_dims
        self.seats = []
        for s, m in enumerate(self.models):
            live = LearnerSeat.live(m)
            if (live.ob_dim, live.ac_dim) != (D[s], A[s]):
                raise ValueError("learner %d (%d observations, %d actions) does not fit agent %d of %s (%d, %d)"
                                 % (s, live.ob_dim, live.ac_dim, s, env.spec.id, D[s], A[s]))
            table = torch.stack([m.params, m.params]).contiguous()
            self.seats.append(LearnerSeat(D[s], A[s], device=self.device, table=table))
        self.fused = os.environ.get("SUMO_MIXED_STEP", "1") != "0" if fused is None else bool(fused)
        self.engine_fused, self.rollout_chunk = bool(engine_fused), int(rollout_chunk)
        if self.rollout_chunk < 0:
            raise ValueError("rollout_chunk = %d: the steps per fused launch, or 0 for the whole rollout in one" % self.rollout_chunk)
        self.tile_rows = tuple(torch.from_numpy(r).to(self.device) for r in rows)
        self._runs = tuple(matches._runs(r) for r in rows)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.ep_sum1 = torch.zeros(self.nenv, dtype=torch.float64, device=self.device)      # agent 1's running episode sums
        self.device_mode, self.recurrent, self.shadow_state0, self.league_scores = True, False, None, None
        self._gstreams = None
        self.obs = env.reset_device()
        self.dones = env.done_dev
        self.dones.zero_()

    def set_frozen(self, side, src):
        """Side ``side``'s frozen checkpoint (table row 1) from a checkpoint path, model, array list or flat vector."""
        seat = self.seats[side]
        seat.table[1].copy_(self._t.from_numpy(seat.vector(src, "agent %d's frozen net" % side)).to(self.device))

    def _group_streams(self):
        t, G = self._t, getattr(self.env, "groups", 1)
        if G > 1 and self._gstreams is None:
            self._gstreams = [t.cuda.Stream(device=self.device) for _ in range(G)]
        return self._gstreams

    def _alloc(self, T):
        t, N, dev = self._t, self.nenv, self.device
        f32 = t.float32
        new = t.zeros if self.engine_fused else t.empty      # the fused launch leaves the halves nobody trains on unwritten: zeros there
        B = dict(rew=t.empty((2, T, N), dtype=f32, device=dev), ep_done=t.empty((T, N), dtype=t.uint8, device=dev),
                 ep_r=t.empty((T, N), dtype=t.float64, device=dev), ep_l=t.empty((T, N), dtype=t.int32, device=dev), side=[])
        for s, seat in enumerate(self.seats):
            D, A = seat.ob_dim, seat.ac_dim
            B["side"].append(dict(obs=new((T, N, D), dtype=f32, device=dev), act=new((T, N, A), dtype=f32, device=dev),
                                  val=new((T, N), dtype=f32, device=dev), nlp=new((T, N), dtype=f32, device=dev),
                                  done=new((T, N), dtype=t.uint8, device=dev),
                                  noise=t.randn((T, N, A), generator=self.models[s].act_model.gen, device=dev, dtype=f32)))
        return B

    def _step_group(self, B, s, alpha, g, sl):
        env, T, N = self.env, self.nsteps, self.nenv
        n = sl.stop - sl.start
        view = env if g is None else mixed.EnvRows(env, sl)
        tiles = slice(sl.start // LEAGUE_TILE, sl.stop // LEAGUE_TILE)
        runs = None if self.fused else tuple(_group_runs(r, tiles) for r in self._runs)
        records = tuple({k: b[k][s, sl] for k in RECORD_KEYS} for b in B["side"])
        pair_step(view, self.seats, tuple(r[tiles] for r in self.tile_rows), tuple(b["noise"][s, sl] for b in B["side"]), records,
                  self.fused, self.status, runs)
        if g is None:
            env.step_device(env.act_dev)
        else:
            env.step_device_group(g, env.act_dev)
        st = self._t.cuda.current_stream(self.device).cuda_stream
        ppo_capi.chk(ppo_capi.lib().ppo_post_step(env.info_dev[sl].data_ptr(), n, alpha, B["rew"][0, s, sl].data_ptr(), T * N,
                                                  env.done_dev[sl].data_ptr(), env.ep_r_dev[sl].data_ptr(), env.ep_l_dev[sl].data_ptr(),
                                                  B["ep_done"][s, sl].data_ptr(), B["ep_r"][s, sl].data_ptr(), B["ep_l"][s, sl].data_ptr(), st))

    def _launch_group(self, B, alpha, g, sl):
        """The rollout's steps of env group ``g`` (envs ``sl``) in fused launches on the current stream."""
        T, N = self.nsteps, self.nenv
        K = self.rollout_chunk or T
        ro = capi.RolloutPair()
        for s, (seat, b) in enumerate(zip(self.seats, B["side"])):
            p = ro.side[s]
            p.table, p.tile_row = seat.table.data_ptr(), self.tile_rows[s].data_ptr()
            p.nrows, p.row_stride, p.ob_dim, p.ac_dim = len(seat), int(seat.table.stride(0)), seat.ob_dim, seat.ac_dim
            p.record_row = 0                                            # the live row: each learner records its own half of the tiles
            p.noise, p.obs, p.act, p.val, p.nlp, p.done = (b[k].data_ptr() for k in ("noise", "obs", "act", "val", "nlp", "done"))
        ro.T, ro.Ntot, ro.env_offset, ro.alpha = T, N, sl.start, float(alpha)
        ro.rew, ro.ep_done, ro.ep_r, ro.ep_l = (B[k].data_ptr() for k in ("rew", "ep_done", "ep_r", "ep_l"))
        for s0 in range(0, T, K):
            ro.s0, ro.K = s0, min(K, T - s0)
            self.env.rollout_steps_pair_group(g, ro)

    def _side_rollout(self, B, side, cur):
        """The 15 fields of learner ``side`` over its own half of the envs, in ``MixedRunner.run``'s placeholder form."""
        from .runner import sf0, sf01
        t, T, dev = self._t, self.nsteps, self.device
        sl, b = own_envs(self.nenv, side), B["side"][side]
        n = sl.stop - sl.start
        f32 = t.float32
        last_values = t.zeros((2, n), dtype=f32, device=dev)
        self.models[side].act_model.evaluate(self.obs[sl, side, :], ppo_capi.FWD_VF, out=dict(value=last_values[0]))
        # ppo_vtrace's agent-0 returns read the agent-0 slot only (its clips are the constant 1): this side's own rewards, values and
        # done flags go there, the other slot is zero-filled, and so are both neglogp arrays, which makes the three ratios exactly 1
        rew, val, zeros = (t.zeros((2, T, n), dtype=f32, device=dev) for _ in range(3))
        rew[0].copy_(B["rew"][side][:, sl])
        val[0].copy_(b["val"][:, sl])
        done = t.zeros((2, T, n), dtype=t.uint8, device=dev)
        done[0].copy_(b["done"][:, sl])
        last_done = t.zeros((n, 2), dtype=t.uint8, device=dev)
        last_done[:, 0].copy_(self.dones[sl, side])
        returns = t.empty((2, T, n), dtype=f32, device=dev)
        opr, oer, ratio = (t.empty((T, n), dtype=f32, device=dev) for _ in range(3))
        ppo_capi.chk(ppo_capi.lib().ppo_vtrace(rew.data_ptr(), val.data_ptr(), zeros.data_ptr(), zeros.data_ptr(), done.data_ptr(),
                                               last_done.data_ptr(), last_values.data_ptr(), T, n, float(self.gamma), float(self.lam), 1.0, 1.0,
                                               returns.data_ptr(), opr.data_ptr(), oer.data_ptr(), ratio.data_ptr(), cur.cuda_stream))
        nlp = t.full((2, T, n), float("inf"), dtype=f32, device=dev)
        nlp[0].copy_(b["nlp"][:, sl])
        flat = lambda x: x[:, sl].swapaxes(0, 1).reshape(n * T, *x.shape[2:])          # [T][N][...] -> env-major rows of the half
        return [(flat(b["obs"]), None), sf01(returns), sf01(done.bool()), (flat(b["act"]), None), sf01(val), sf01(nlp), sf01(rew), sf01(zeros),
                None, None, None, None, sf0(opr), sf0(oer), sf0(ratio)]

    def _episodes(self, B):
        """(EpInfoList of agent 0's side, of agent 1's side), each over its own half of the envs."""
        from .runner import EpInfoList
        N = self.nenv
        d = B["ep_done"].bool()
        r1, self.ep_sum1 = running_episode_sums(B["rew"][1], d, self.ep_sum1)
        dn, ll = d.cpu().numpy(), B["ep_l"].cpu().numpy()
        out = []
        for side, rr in enumerate((B["ep_r"].cpu().numpy(), r1.cpu().numpy())):
            sl = own_envs(N, side)
            m = dn[:, sl]
            out.append(EpInfoList(rr[:, sl][m], ll[:, sl][m]))
        return out

    def run(self, update):
        """One rollout of ``nsteps`` steps.  Returns two 15-field rollouts (``alg_ppo.Rollout`` order, ``MixedRunner.run``'s placeholder
        form: slot 0 is the learner, slot 1 the zero-filled placeholder), learner 0's over envs ``[0, N / 2)`` and learner 1's over
        ``[N / 2, N)``: ``N / 2 * nsteps`` rows each, env-major.  Returns are plain GAE(lambda) on the side's own annealed rewards,
        values and done flags; learner 1's episode returns are sums of its annealed reward (see the class)."""
        from .runner import anneal_alpha
        t, env = self._t, self.env
        T, N = self.nsteps, self.nenv
        for seat, m in zip(self.seats, self.models):
            seat.table[0].copy_(m.params)
        B = self._alloc(T)
        self.last_buffers = B
        alpha = anneal_alpha(update, self.anneal_bound)
        self.status.zero_()
        streams = self._group_streams()
        cur = t.cuda.current_stream(self.device)

        def on_groups(fn):                                              # fn(group, its envs) for every env group, on its stream
            if streams is None:
                return fn(None, slice(0, N))
            for g, st in enumerate(streams):
                with t.cuda.stream(st):
                    fn(g, env._gs(g))

        for st in streams or ():
            st.wait_stream(cur)
        if self.engine_fused:
            on_groups(lambda g, sl: self._launch_group(B, alpha, g or 0, sl))
        else:
            for s in range(T):
                on_groups(lambda g, sl: self._step_group(B, s, alpha, g, sl))
        for st in streams or ():
            cur.wait_stream(st)
        if self.engine_fused:
            for E in env.engines:                                       # waits for the group's launches; raises if one was cut short
                E.rollout_status()
        self.obs, self.dones = env.obs_dev, env.done_dev
        out = [self._side_rollout(B, side, cur) for side in range(2)]
        mixed.raise_status(self.status, ROW_SIDES)
        for side, ep in enumerate(self._episodes(B)):
            out[side][11] = ep
        return tuple(out[0]), tuple(out[1])


# ---- training -------------------------------------------------------------------------------------------------------------
def check_learn(env, *, network, opponent_mode, nsteps, nminibatches, fused_rollout=False):
    """What :func:`learn` refuses, each with its own message, before anything touches the device or a file is written."""
    if not mixed.is_mixed(env):
        raise ValueError("co_train.learn grows two species against each other: %s is a homogeneous match-up, which alg_ppo.learn trains "
                         "in self-play" % env.spec.id)
    D, A = env.model.obs_dims, env.model.act_dims
    where = "co-training on a mixed match-up (observations %d / %d, actions %d / %d)" % (D[0], D[1], A[0], A[1])
    if opponent_mode not in ("latest", "random"):
        raise ValueError("%s: opponent_mode must be 'latest' or 'random', got %r ('ours' would score another species' samples; 'fix' "
                         "against policy-zoo nets is alg_ppo.learn's)" % (where, opponent_mode))
    if network != "mlp":
        raise NotImplementedError("%s: network=%r is not available, both seats hold MLP(64,64) policies" % (where, network))
    if env.num_envs < PAIR_TILES or env.num_envs % PAIR_TILES:
        raise ValueError("%s: num_envs = %d is not a multiple of %d (each learner trains on its own half of the 16-env tiles)"
                         % (where, env.num_envs, PAIR_TILES))
    nbatch = env.num_envs // 2 * int(nsteps)
    if nbatch % int(nminibatches):
        raise ValueError("%s: each learner's batch of num_envs / 2 * nsteps = %d rows does not split into nminibatches = %d"
                         % (where, nbatch, int(nminibatches)))
    check_engine_fused(env, fused_rollout, "%s: fused_rollout=True (--fused_rollout)" % where, "fused_rollout=False")


def choose_frozen(update, opponent_mode, checkdirs, histories):
    """The selection of one update, the reference's self-play law (alg_ppo.py:207-247) lifted to two species: for side 0, then side 1,
    the frozen version of the OTHER side from that side's checkpoint directory -- ``00000`` at update 1, then the newest file
    ('latest') or a uniform draw among the files present ('random': one ``np.random.choice`` per side, in that order).  Records
    ``opponent_versions`` and ``version_gap`` in ``histories[s]`` as ``alg_ppo.select_opponents`` does; returns the two paths."""
    out = []
    for s in range(2):
        ck = checkdirs[1 - s]
        if update == 1:
            paths, choice = [osp.join(ck, "00000")], 0
            histories[s]["version_gap"].append(0)
        else:
            paths = sorted(osp.join(ck, f) for f in os.listdir(ck))
            if opponent_mode == "random":
                choice = int(np.random.choice(len(paths)))
                histories[s]["version_gap"].append(update - 1 - choice)
            elif opponent_mode == "latest":
                choice = len(paths) - 1
            else:
                raise ValueError("opponent_mode %r" % (opponent_mode,))
        histories[s]["opponent_versions"].append([choice])
        out.append(paths[choice])
    return out


def _new_history():
    return dict(version_gap=[], off_policy_ratio_mean=[], off_env_ratio_mean=[], total_ratio_mean=[], off_policy_ratio_clip_frac=[],
                off_env_ratio_clip_frac=[], total_ratio_clip_frac=[], useful_ratio=[], opponent_versions=[], ppo_clip_frac=[], approxkl=[],
                early_stop_info=[], lossvals=[], fps=[], rollout_s=[], update_s=[])


def learn(*, env, total_timesteps, network="mlp", opponent_mode="latest", seed=None, nsteps=2048, nminibatches=4, noptepochs=4, lr=3e-4,
          cliprange=0.2, gamma=0.99, lam=0.95, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, kl_threshold=None, anneal_bound=500,
          save_interval=1, log_interval=10, log_dir=None, verbose=True, fused_rollout=False, **network_kwargs):
    """Train one MLP(64,64) learner per side of a mixed match-up against the other side's checkpoints.  Per update: selection
    (:func:`choose_frozen`), one :meth:`PairRunner.run`, then per side (0, then 1) ``alg_ppo.clean_and_assemble`` and
    ``alg_ppo.optimise_indexed`` on that side's half of the envs (``num_envs / 2 * nsteps`` rows), its printed line and its
    checkpoint ``log_dir/agentS/checkpoints/NNNNN`` (``00000`` before the first update).  ``total_timesteps`` counts each learner's
    own rows.  Each ``log_dir/agentS`` is a run directory of its own for ``eval_against_fix.py`` and ``compare_versions.py``.
    ``fused_rollout``: the rollouts run in the engine's fused launch (``PairRunner(engine_fused=True)``): the same checkpoints, bit for
    bit.  Returns ``(model0, model1)``, ``model_s.history`` that side's history.  Agent 1's ``eprewmean`` is the mean of its ANNEALED
    episode reward sums (``PairRunner``), not the monitor's figure."""
    from . import alg_ppo
    from .model import PPOModel
    from .policies import PolicySpec
    check_learn(env, network=network, opponent_mode=opponent_mode, nsteps=nsteps, nminibatches=nminibatches, fused_rollout=fused_rollout)
    import torch
    if seed is not None:                                                # as alg_ppo.learn (set_global_seeds)
        np.random.seed(seed)
        torch.manual_seed(seed)
    lr = alg_ppo.constfn(lr) if isinstance(lr, float) else lr
    cliprange = alg_ppo.constfn(cliprange) if isinstance(cliprange, float) else cliprange
    nenvs, half = env.num_envs, env.num_envs // 2
    nbatch = half * nsteps
    nbatch_train = nbatch // nminibatches
    nupdates = int(total_timesteps) // nbatch
    dev = getattr(env, "device", torch.device("cuda", 0))
    models = []
    for s in range(2):
        ob_space, ac_space = env.observation_space[s], env.action_space[s]
        spec = PolicySpec(ob_space.shape[0], ac_space.shape[0], network, **dict(dict(value_network="copy"), **network_kwargs))
        models.append(PPOModel(policy=spec, ob_space=ob_space, ac_space=ac_space, nbatch_act=nenvs, nbatch_train=nbatch_train, nsteps=nsteps,
                               ent_coef=ent_coef, vf_coef=vf_coef, max_grad_norm=max_grad_norm, trainable=True, model_scope="model_%d" % s,
                               device=dev.index or 0))
        models[s].equal_counts = True
    log_dir = log_dir or os.environ.get("OPENAI_LOGDIR") or "/tmp/robosumo_selfplay_amd"
    checkdirs = [osp.join(log_dir, "agent%d" % s, "checkpoints") for s in range(2)]
    for s in range(2):
        alg_ppo.save_checkpoint(models[s], checkdirs[s], "00000")
        models[s].act_model.seed((seed or 0) * 1000 + 17 * s)
    runner = PairRunner(env, models, nsteps, gamma, lam, anneal_bound, engine_fused=bool(fused_rollout))
    shuffle_gens = []
    for s in range(2):
        g = torch.Generator(device=dev)
        g.manual_seed((seed or 0) * 7919 + 13 + s)
        shuffle_gens.append(g)
    histories = [_new_history() for _ in range(2)]
    epinfobufs = [deque(maxlen=100) for _ in range(2)]
    tfirststart = time.perf_counter()
    for update in range(1, nupdates + 1):
        tstart = time.perf_counter()
        frac = 1.0 - (update - 1.0) / nupdates
        lrnow, cliprangenow = lr(frac), cliprange(frac)
        # ---- selection: each side's frozen net is what the OTHER learner meets
        for s, path in enumerate(choose_frozen(update, opponent_mode, checkdirs, histories)):
            runner.set_frozen(1 - s, path)
        # ---- one rollout for both learners
        ros = [alg_ppo.Rollout(*r) for r in runner.run(update)]
        torch.cuda.synchronize(dev)
        t_roll = time.perf_counter() - tstart
        for s, (ro, model, history) in enumerate(zip(ros, models, histories)):
            tside = time.perf_counter()
            ub = alg_ppo.clean_and_assemble(ro, history, rho_bar=1.0, recurrent=False, shadow_state0=None, nenvs=half, nbatch=nbatch,
                                            neglogp_threshold=10000.0, use_opponent_data=None, vgap=None)
            epinfobufs[s].extend(ro.epinfos[-100:])
            lossvals, stop_info = alg_ppo.optimise_indexed(model, ub, lrnow, cliprangenow, nbatch_train=nbatch_train, noptepochs=noptepochs,
                                                           kl_threshold=kl_threshold, shuffle_gen=shuffle_gens[s], comm=None, dev=dev)
            history["early_stop_info"].append(stop_info); history["lossvals"].append(lossvals)
            history["ppo_clip_frac"].append(lossvals[-1]); history["approxkl"].append(lossvals[-2])
            torch.cuda.synchronize(dev)
            t_sgd = time.perf_counter() - tside
            history["rollout_s"].append(t_roll); history["update_s"].append(t_sgd)
            history["fps"].append(nbatch / (t_roll + t_sgd))
            if verbose and (update % log_interval == 0 or update == 1):
                ev = alg_ppo.explained_variance(ub["values"].cpu().numpy(), ub["returns"].cpu().numpy())
                print("agent%d update %d/%d  fps %.0f  rollout %.2fs  sgd %.2fs  opponent %05d  ev %.3f  eprewmean %.2f  eplenmean %.1f  %s" % (
                    s, update, nupdates, history["fps"][-1], t_roll, t_sgd, history["opponent_versions"][-1][0], ev,
                    alg_ppo.safemean([e["r"] for e in epinfobufs[s]]), alg_ppo.safemean([e["l"] for e in epinfobufs[s]]),
                    " ".join("%s %.4g" % (n, v) for n, v in zip(model.loss_names, lossvals))), flush=True)
            if save_interval and (update % save_interval == 0 or update == 1):
                alg_ppo.save_checkpoint(model, checkdirs[s], "%.5i" % update)
    for s in range(2):
        models[s].history = histories[s]
        models[s].time_elapsed = time.perf_counter() - tfirststart
    return models[0], models[1]


# ---- matches between the two sides -----------------------------------------------------------------------------------------
def _pair_steps(env, seats, tiles, score, quota, K, noise, fused):
    """K steps of a batch: :func:`pair_step` without a record, ``env.step_device`` and the score update of ``matches``.  A tile without
    a table row raises ``ValueError``: before the first step on the step-by-step path, after the K steps on the fused one."""
    import torch
    runs = status = None
    if fused:
        status = torch.zeros(1, dtype=torch.int32, device=env.device)
    else:
        runs = tuple(matches._runs(x.cpu().numpy()) for x in tiles)
        for side in range(2):
            for t0, _, e in runs[side]:
                if not 0 <= e < len(seats[side]):
                    raise ValueError("tile %d of seat %d: row %d names no net of the seat (%d nets)" % (t0, side, e, len(seats[side])))
    for k in range(int(K)):
        pair_step(env, seats, tiles, None if noise is None else (noise[0][k], noise[1][k]), None, fused, status, runs)
        _, info, done, _, _, _ = env.step_device(env.act_dev)
        matches._score_step(score, info, done, quota)
    if fused:
        mixed.raise_status(status, ROW_SIDES)


def play_checkpoint_pairs(env, seat0, seat1, pairs, rounds_per_env, envs_per_pair, deterministic=True, seed=0, adjust_z=EVAL_ADJUST_Z,
                          chunk=64, fused=True):
    """``mixed.play_checkpoints_against_seat`` with a :class:`mixed.LearnerSeat` on BOTH sides: every match-up ``pairs[p] = (i, j)`` --
    row i of ``seat0`` as agent 0 against row j of ``seat1`` as agent 1 -- on ``envs_per_pair`` envs (a multiple of 16),
    ``rounds_per_env`` finished episodes per env, through the same batch loop (``mixed.play_seat_batches``).  Returns one dict per
    pair: wins (agent 0's), losses, draws, rounds, env_steps."""
    mixed.check_batch_args(env, rounds_per_env, envs_per_pair, chunk)
    pairs = [(int(i), int(j)) for i, j in pairs]
    for i, j in pairs:
        if not (0 <= i < len(seat0) and 0 <= j < len(seat1)):
            raise ValueError("pair (%d, %d) refers to a non-existent net (%d rows of agent 0 / %d rows of agent 1)" % (i, j, len(seat0), len(seat1)))
    seats = (seat0, seat1)
    return mixed.play_seat_batches(env, seats, pairs, rounds_per_env, envs_per_pair, deterministic, seed, adjust_z, chunk,
                                   lambda idx0, idx1: (seat0.tile_rows(idx0), seat1.tile_rows(idx1)), lambda: None,
                                   lambda tiles, _state, score, K, noise: _pair_steps(env, seats, tiles, score, int(rounds_per_env), K, noise, fused))


def compare_history_versions(path0, path1, trials, interval=1, num_env=256, deterministic=False, seed=0, adjust_z=EVAL_ADJUST_Z,
                             env_id="RoboSumo-Ant-vs-Bug-v0", chunk=64, env=None, fused=True):
    """``matches.compare_history_versions`` for the two sides of a co-trained run: version k of ``path0`` (agent 0's run directory,
    ``<log_dir>/agent0``) against version k of ``path1`` (agent 1's), for every ``interval``-th version (``00000`` excluded) that both
    runs hold, exactly ``trials`` games each -- a multiple of 16, split by ``zoo_pairs.split_trials16``.  Returns the same dict:
    versions=[(id, id)], win_rate=[agent 0's wins / trials], results, network='mlp', nlstm=None."""
    interval = int(interval)
    if interval < 1:
        raise ValueError("interval must be >= 1")
    ids1 = set(matches.list_checkpoints(path1))
    ids = [c for c in matches.list_checkpoints(path0) if c in ids1][::interval]
    if not ids:
        raise ValueError("no versions that both %s and %s hold" % (path0, path1))
    paths = [[osp.join(matches.checkpoint_dir(p), c) for c in ids] for p in (path0, path1)]
    for p in (paths[0][0], paths[1][0]):
        kind = matches.checkpoint_kind(p)
        if kind[0] != "mlp":
            raise NotImplementedError("mixed match-ups: both seats hold MLP(64,64) checkpoints, %s is an %s one" % (p, matches._kind_name(kind)))
    epp, rounds = zoo_pairs.split_trials16(trials, num_env if env is None else env.num_envs)
    env, own = matches._make_env(env_id, num_env, seed, env)
    try:
        if not mixed.is_mixed(env):
            raise ValueError("%s is a homogeneous match-up: matches.compare_history_versions compares its runs" % env.spec.id)
        seats = [LearnerSeat(env.model.obs_dims[s], env.model.act_dims[s], paths[s], env.device) for s in range(2)]
        res = play_checkpoint_pairs(env, seats[0], seats[1], [(k, k) for k in range(len(ids))], rounds, epp, deterministic=deterministic,
                                    seed=seed, adjust_z=adjust_z, chunk=chunk, fused=fused)
    finally:
        if own:
            env.close()
    return dict(versions=[(c, c) for c in ids], win_rate=[r["wins"] / float(trials) for r in res], results=res, network="mlp", nlstm=None)
