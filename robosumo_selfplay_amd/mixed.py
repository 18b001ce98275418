"""A learner on the MIXED match-ups (``RoboSumo-Ant-vs-Bug-v0``, ``RoboSumo-Spider-vs-Ant-v0``, ...: six of the nine scenes, whose two
sides differ in observation and action width) against policy-zoo nets: training in ``opponent_mode='fix'`` and batched offline
evaluation.

The reference cannot do this -- its Runner sizes both policies from ``observation_space[0]`` (runner.py:14-16) -- but nothing
forbids it in fix mode: the learner only ever needs agent 0's stream, and the zoo net only agent 1's observation without its last
column.  A :class:`LearnerSeat` holds the MLP(64,64) parameter rows that may play agent 0, a :class:`zoo_pairs.ZooSeat` the zoo nets
of agent 1.  :func:`mixed_step` makes both seats' actions of one step -- fused: ONE ``ppo_mixed_step`` launch from the env's
observation / done buffers into its action buffer and agent 0's rollout record; ``fused=False``: the definition, ``ppo_forward``
per run of tiles that share a row, ``zoo_pairs.seat_act(fused=False)`` and torch copies.  :class:`MixedRunner` drives
``SumoVecEnv.step_device`` with it and returns the 15-field rollout ``alg_ppo.learn``'s stages index;
:func:`play_checkpoints_against_seat` / :func:`evaluate_history_against_zoo` are ``zoo_pairs.play_zoo_pairs`` with a learner seat
on side 0.  The engine's fused launches stay homogeneous.
"""
import ctypes as C
import os

import numpy as np

from . import matches, policies, policy_zoo, ppo_capi, zoo_pairs
from .policy_zoo import EVAL_ADJUST_Z, LEAGUE_TILE


def is_mixed(env):
    """The env's two sides differ in observation or action width."""
    m = getattr(env, "model", None)
    if m is None or not hasattr(m, "obs_dims"):
        return False
    return m.obs_dims[0] != m.obs_dims[1] or m.act_dims[0] != m.act_dims[1]


def _shape_of_count(P):
    """(ob_dim, ac_dim) of the MLP(64,64)+copy-value policy with ``P`` parameters, ac_dim in [1, 16]; None if there is none."""
    for A in range(1, 17):
        p0, p1 = matches.param_count(0, A), matches.param_count(1, A)
        if P > p0 and (P - p0) % (p1 - p0) == 0:
            return (P - p0) // (p1 - p0), A
    return None


def _shape_of(src):
    """The policy shape a learner-seat source was made for, where it can be read without loading anything; else None."""
    if hasattr(src, "params") and hasattr(src, "spec"):
        return int(src.spec.ob_dim), int(src.spec.ac_dim)
    if isinstance(src, (list, tuple)) and len(src) == 13:
        s0, s8 = np.shape(src[0]), np.shape(src[8])
        return (int(s0[0]), int(s8[1])) if len(s0) == 2 and len(s8) == 2 else None
    if isinstance(src, (str, os.PathLike, dict)):
        return None
    n = src.numel() if hasattr(src, "numel") else np.size(src)
    return _shape_of_count(int(n))


class LearnerSeat(object):
    """The MLP(64,64)+copy-value nets that may play ONE side of a mixed match-up: a device table ``[nrows][P]`` of parameter rows in
    ``PPOModel``'s flat order.  ``LearnerSeat.live(model)`` is the training seat: its one row IS the model's ``params`` (no copy, the
    optimiser's steps show at once).  ``LearnerSeat(ob_dim, ac_dim, sources)`` fills its rows through
    :func:`matches.snapshot_vector` from checkpoints paths, models, array lists or flat vectors (evaluation).  A net of another
    shape is refused with both shapes named (an ant checkpoint cannot sit on a bug seat)."""

    def __init__(self, ob_dim, ac_dim, sources=(), device=0, table=None):
        self.device = zoo_pairs._device(device)
        self.ob_dim, self.ac_dim = int(ob_dim), int(ac_dim)
        self.spec = policies.PolicySpec(self.ob_dim, self.ac_dim, value_network="copy", activation="relu")
        self.P = matches.param_count(self.ob_dim, self.ac_dim)
        self.labels = []
        if table is not None:
            self.table, self.labels = table, [None] * int(table.shape[0])
            return
        sources = list(sources)
        if not sources:
            raise ValueError("a learner seat needs at least one net")
        rows = [self.vector(src, "net %d" % k) for k, src in enumerate(sources)]
        self.labels = [str(s) if isinstance(s, (str, os.PathLike)) else None for s in sources]
        import torch
        self.table = torch.from_numpy(np.stack(rows)).to(self.device)

    @classmethod
    def live(cls, model):
        """The training seat: row 0 aliases ``model.params``."""
        D, A = model.spec.ob_dim, model.spec.ac_dim
        if int(model.params.numel()) != matches.param_count(D, A) or not model.params.is_contiguous():
            raise ValueError("the model's flat parameter vector does not hold an MLP(64,64) policy of (%d, %d)" % (D, A))
        return cls(D, A, device=model.params.device, table=model.params.view(1, -1))

    def vector(self, src, name="net"):
        """``src`` as a flat parameter row of this seat; ``ValueError`` naming both shapes where it was made for another one."""
        got = _shape_of(src)
        if got is not None and got != (self.ob_dim, self.ac_dim):
            raise ValueError("%s is an MLP(64,64) policy of %d observations and %d actions, the seat plays %d observations and %d "
                             "actions (another species?)" % (name, got[0], got[1], self.ob_dim, self.ac_dim))
        try:
            return matches.snapshot_vector(self.spec, src)
        except ValueError as e:
            raise ValueError("%s does not fit this seat (%d observations, %d actions; another species?): %s"
                             % (name, self.ob_dim, self.ac_dim, e))

    def __len__(self):
        return int(self.table.shape[0])

    def tile_rows(self, env_net):
        """int32 [n / 16] rows of the tiles of a batch whose env e plays row ``env_net[e]``; the 16 envs of a tile share their row."""
        env_net = np.asarray(env_net, np.int64)
        if env_net.ndim != 1 or env_net.size < LEAGUE_TILE or env_net.size % LEAGUE_TILE:
            raise ValueError("a seat plays whole tiles of %d envs, got %d envs" % (LEAGUE_TILE, env_net.size))
        tiles = env_net.reshape(-1, LEAGUE_TILE)
        if (tiles != tiles[:, :1]).any():
            raise ValueError("the %d envs of a tile play one net" % LEAGUE_TILE)
        if tiles.min() < 0 or tiles.max() >= len(self):
            raise ValueError("row index outside [0, %d)" % len(self))
        return tiles[:, 0].astype(np.int32)

    def struct(self, tile_row=None):
        """The ``ppo_capi.LearnerSeat`` launch struct (``tile_row``: int32 CUDA [n / 16] or None = row 0 everywhere)."""
        s = ppo_capi.LearnerSeat()
        s.table, s.tile_row = self.table.data_ptr(), None if tile_row is None else tile_row.data_ptr()
        s.nrows, s.row_stride, s.ob_dim, s.ac_dim = len(self), int(self.table.stride(0)), self.ob_dim, self.ac_dim
        return s


class EnvRows(object):
    """The rows ``sl`` of an env's device buffers behind the attributes :func:`mixed_step` and ``zoo_pairs.seat_act`` read: one env
    group of a ``SumoVecEnv``."""

    def __init__(self, env, sl):
        self.num_envs, self.device, self.model, self.spec = sl.stop - sl.start, env.device, env.model, env.spec
        self.obs_dev, self.act_dev, self.done_dev = env.obs_dev[sl], env.act_dev[sl], env.done_dev[sl]
        self._stream = env._stream


RECORD_KEYS = ("obs", "act", "nlp", "val", "done")


def _check_mixed_step(lseat, env, tile_row, noise0, record, side=0):
    """The arguments of a learner seat on ``side`` of one step (``noise0`` / ``record``: that side's)."""
    import torch
    N, D0, A0 = env.num_envs, lseat.ob_dim, lseat.ac_dim
    if (D0, A0) != (env.model.obs_dims[side], env.model.act_dims[side]):
        raise ValueError("the learner seat (%d observations, %d actions) does not fit agent %d of %s (%d, %d)"
                         % (D0, A0, side, env.spec.id, env.model.obs_dims[side], env.model.act_dims[side]))
    if tile_row is not None and (not torch.is_tensor(tile_row) or tile_row.dtype != torch.int32 or not tile_row.is_contiguous()
                                 or tuple(tile_row.shape) != (N // LEAGUE_TILE,) or tile_row.device != env.device):
        raise ValueError("tile_row must be a contiguous int32 tensor [%d] on the env's device" % (N // LEAGUE_TILE))
    if noise0 is not None and (tuple(noise0.shape) != (N, A0) or noise0.dtype != torch.float32 or not noise0.is_contiguous()):
        raise ValueError("noise%d must be a contiguous float32 tensor [%d][%d]" % (side, N, A0))
    shapes = dict(obs=((N, D0), torch.float32), act=((N, A0), torch.float32), nlp=((N,), torch.float32), val=((N,), torch.float32),
                  done=((N,), torch.uint8))
    for k, x in (record or {}).items():
        if k not in shapes:
            raise ValueError("unknown record entry %r (known: %s)" % (k, ", ".join(RECORD_KEYS)))
        if x is not None and (tuple(x.shape) != shapes[k][0] or x.dtype != shapes[k][1] or not x.is_contiguous()):
            raise ValueError("record[%r] must be a contiguous %s tensor of shape %s" % (k, shapes[k][1], shapes[k][0]))


def mixed_step(env, learner_seat, zoo_seat, tile_entry, state, noise0=None, noise1=None, tile_row=None, record=None, fused=True,
               status=None, runs0=None, runs1=None):
    """Both agents' actions of one step of a mixed match-up, into ``env.act_dev``: agent 0 by ``learner_seat`` (tile t with row
    ``tile_row[t]``, int32 CUDA [N / 16]; None = row 0 everywhere) on ``env.obs_dev[:, 0]``, agent 1 by ``zoo_seat`` as
    :func:`zoo_pairs.seat_act` plays it (``tile_entry``, ``state``, ``noise1``).  ``noise0``: float32 [N][A0] standard-normal rows, None
    = the means.  ``record``: dict of optional contiguous tensors that receive agent 0's rollout record of the step -- ``obs``
    [N][D0], ``act`` [N][A0], ``nlp`` [N], ``val`` [N] (float32) and ``done`` [N] (uint8, agent 0's flag of the previous step);
    without ``val`` the value trunk is not evaluated.  ``env``: a ``SumoVecEnv`` or :class:`EnvRows` of one of its groups.

    ``fused``: one ``ppo_mixed_step`` launch; a tile whose learner row or zoo entry names no table row writes nothing for that
    side and leaves ``ppo_capi.mixed_status(tile, side)`` in ``status`` (int32 CUDA [1], optional).  ``fused=False`` is the
    definition: ``ppo_forward`` (PI, and VF with ``val``) per run of tiles sharing a row (``runs0``, default the runs of
    ``tile_row``, a device read), torch copies into the action buffer and the record, then ``zoo_pairs.seat_act(fused=False)``
    (``runs1``); runs whose row names no net are skipped."""
    _check_mixed_step(learner_seat, env, tile_row, noise0, record)
    zoo_pairs._check_step(zoo_seat, env, 1, tile_entry, state, noise1)
    rec = dict.fromkeys(RECORD_KEYS)
    rec.update(record or {})
    if fused:
        N, L, st, obs, act, done = env.num_envs, ppo_capi.lib(), env._stream(), env.obs_dev, env.act_dev, env.done_dev
        ls, zs = learner_seat.struct(tile_row), zoo_seat.struct(tile_entry, state)
        r = ppo_capi.MixedRecord()
        r.obs, r.action, r.neglogp, r.value, r.done = (ppo_capi.ptr(rec[k]) for k in RECORD_KEYS)
        ppo_capi.chk(L.ppo_mixed_step(C.byref(ls), C.byref(zs), obs[:, 0].data_ptr(), obs[:, 1].data_ptr(), N, obs.stride(0),
                                      done.data_ptr(), done.stride(0), ppo_capi.ptr(noise0), ppo_capi.ptr(noise1), act[:, 0].data_ptr(),
                                      act[:, 1].data_ptr(), act.stride(0), C.byref(r), ppo_capi.ptr(status), st))
        return
    learner_side_definition(env, learner_seat, 0, tile_row, noise0, rec, runs0)
    zoo_pairs.seat_act(zoo_seat, env, 1, tile_entry, state, noise1, fused=False, runs=runs1)


def learner_side_definition(env, learner_seat, side, tile_row, noise0, rec, runs0=None):
    """The definition of a learner seat's step on ``side``: ``ppo_forward`` (PI, and VF with ``rec['val']``) per run of tiles sharing a
    row (``runs0``, default the runs of ``tile_row``, a device read), torch copies into ``act_dev[:, side, :A]`` and the record
    ``rec`` (every key of ``RECORD_KEYS`` present, None = skip); runs whose row names no net are skipped."""
    import torch
    N, D0, A0 = env.num_envs, learner_seat.ob_dim, learner_seat.ac_dim
    L, st, obs, act, done = ppo_capi.lib(), env._stream(), env.obs_dev, env.act_dev, env.done_dev
    if runs0 is None:
        runs0 = [(0, N // LEAGUE_TILE, 0)] if tile_row is None else matches._runs(tile_row.cpu().numpy())
    out = torch.empty((N, A0), dtype=torch.float32, device=env.device) if rec["act"] is None else rec["act"]
    flags = ppo_capi.FWD_PI | (ppo_capi.FWD_VF if rec["val"] is not None else 0)
    for t0, t1, row in runs0:
        if not 0 <= row < len(learner_seat):
            continue
        rows = slice(LEAGUE_TILE * t0, LEAGUE_TILE * t1)
        n = rows.stop - rows.start
        sub = lambda x: None if x is None else x[rows].data_ptr()
        ppo_capi.chk(L.ppo_forward(learner_seat.table[row].data_ptr(), obs[rows, side].data_ptr(), n, obs.stride(0), D0, A0, flags,
                                   sub(noise0), None, out[rows].data_ptr(), sub(rec["nlp"]), sub(rec["val"]), None, st))
        act[rows, side, :A0] = out[rows]
        if rec["obs"] is not None:
            rec["obs"][rows] = obs[rows, side, :D0]
        if rec["done"] is not None:
            rec["done"][rows] = done[rows, side]


def raise_status(status, sides=("learner row", "zoo entry")):
    """``ValueError`` naming tile and side if a ``ppo_mixed_step`` status word is set (a device read)."""
    bad = int(status.item())
    if bad:
        tile, side = ppo_capi.mixed_status_decode(bad)
        raise ValueError("tile %d: its %s names no table row of the seat" % (tile, sides[side]))


# ---- training -------------------------------------------------------------------------------------------------------------
def league_tiles(nmembers, nenvs, update):
    """The member every 16-env tile faces in ``update`` (1-based): ``policy_zoo.league_plan`` rotated by one tile per update."""
    return policy_zoo.league_plan(nmembers, nenvs, offset=int(update) - 1)


def check_groups(env):
    """Env groups must start and end on multiples of 16 (a tile belongs to one group's launch)."""
    N = env.num_envs
    if N < LEAGUE_TILE or N % LEAGUE_TILE:
        raise ValueError("mixed match-ups play whole tiles of %d envs: num_envs = %d" % (LEAGUE_TILE, N))
    gs = getattr(env, "group_size", N)
    if gs % LEAGUE_TILE:
        raise ValueError("mixed match-ups: the env groups must start and end on multiples of %d (group size %d)" % (LEAGUE_TILE, gs))


def check_learn(env, *, network, opponent_mode, use_opponent_data, opponent_pool, fused_fix_opponent, fused_selector, eval_interval,
                eval_opponents, comm):
    """What ``alg_ppo.learn`` refuses on a mixed env in ``opponent_mode='fix'``, each with its own message, before anything touches
    the device."""
    D, A = env.model.obs_dims, env.model.act_dims
    where = "mixed match-up (observations %d / %d, actions %d / %d)" % (D[0], D[1], A[0], A[1])
    if opponent_mode != "fix":
        raise ValueError("%s: only opponent_mode='fix' trains here, got %r" % (where, opponent_mode))
    if use_opponent_data is not None:
        raise NotImplementedError("%s: use_opponent_data=%r is not available, the learner cannot score another species' action"
                                  % (where, use_opponent_data))
    if network != "mlp":
        raise NotImplementedError("%s: network=%r is not available, the learner's seat holds MLP(64,64) policies" % (where, network))
    if int(opponent_pool) > 1:
        raise ValueError("%s: opponent_pool > 1 makes no sense with a fixed opponent; give fix_opponent_path a list for a league" % where)
    if fused_fix_opponent:
        raise NotImplementedError("%s: fused_fix_opponent selects the engine's fused rollout launch, which is built for one observation "
                                  "and action space" % where)
    if fused_selector:
        raise ValueError("%s: fused_selector serves opponent_mode='ours', which a mixed match-up cannot run" % where)
    if eval_interval or eval_opponents:
        raise NotImplementedError("%s: evaluation while training (eval_interval / eval_opponents) is out of scope; evaluate the run "
                                  "afterwards with eval_against_fix.py --fused" % where)
    if comm is not None:
        raise NotImplementedError("%s: training runs on a single GPU (comm must be None)" % where)
    if env.num_envs < LEAGUE_TILE or env.num_envs % LEAGUE_TILE:
        raise ValueError("%s: num_envs = %d is not a multiple of %d (the seats play whole tiles)" % (where, env.num_envs, LEAGUE_TILE))


def fix_paths(fix_opponent_path):
    if fix_opponent_path is None:
        raise ValueError("opponent_mode='fix' needs fix_opponent_path=<policy_zoo .npy> of agent 1's species (one file or a list)")
    return list(fix_opponent_path) if isinstance(fix_opponent_path, (list, tuple)) else [fix_opponent_path]


class MixedRunner(object):
    """Device-mode rollouts of an MLP learner (``model``, a ``PPOModel`` on agent 0's spaces) against the zoo nets of ``zoo_seat`` on
    a mixed ``SumoVecEnv``.  Per step and env group, on the group's stream: :func:`mixed_step` (writing slice s of the buffers),
    ``env.step_device[_group]``, ``ppo_post_step``.  The buffers hold agent 0's stream only (the ``[2][T][N]`` reward buffer stays:
    ``ppo_post_step`` writes both agents).  The action noise is drawn ONCE per rollout for the whole buffer -- ``[T][N][A0]`` from the
    learner's generator, ``[T][N][A1]`` from the seat's (``gen1``) -- so the number of env groups does not change the numbers.  A seat
    of several nets is a league: :meth:`assign` deals them over the tiles per update and ``league_scores`` holds the last rollout's
    tally.  The zoo LSTM state rows persist across ``run()`` calls.  ``fused``: the one-launch step; default from the environment,
    ``SUMO_MIXED_STEP=0`` selects the definition (same numbers, bit for bit)."""

    def __init__(self, env, model, zoo_seat, nsteps, gamma, lam, anneal_bound=500, fused=None, seat_seed=0):
        import torch
        self._t = torch
        if not hasattr(env, "step_device"):
            raise ValueError("MixedRunner is device mode only: it needs a SumoVecEnv")
        check_groups(env)
        ppo_capi.lib()
        self.env, self.model, self.zoo_seat = env, model, zoo_seat
        self.models = [model]
        self.nenv, self.nsteps, self.gamma, self.lam, self.anneal_bound = env.num_envs, int(nsteps), gamma, lam, anneal_bound
        self.device = env.device
        self.learner_seat = LearnerSeat.live(model)
        D, A = env.model.obs_dims, env.model.act_dims
        if (self.learner_seat.ob_dim, self.learner_seat.ac_dim) != (D[0], A[0]):
            raise ValueError("the learner (%d observations, %d actions) does not fit agent 0 of %s (%d, %d)"
                             % (self.learner_seat.ob_dim, self.learner_seat.ac_dim, env.spec.id, D[0], A[0]))
        if (zoo_seat.ob_dim, zoo_seat.ac_dim) != (D[1] - 1, A[1]):
            raise ValueError("the seat's nets (%d observation columns, %d actions) do not fit agent 1 of %s (%d, %d)"
                             % (zoo_seat.ob_dim, zoo_seat.ac_dim, env.spec.id, D[1] - 1, A[1]))
        self.fused = os.environ.get("SUMO_MIXED_STEP", "1") != "0" if fused is None else bool(fused)
        self.gen1 = torch.Generator(device=self.device)
        self.gen1.manual_seed(int(seat_seed))
        self.state = zoo_seat.new_state(self.nenv)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.league_scores = None
        self.device_mode, self.recurrent, self.shadow_state0 = True, False, None
        self._gstreams = None
        self.assign(1)
        self.obs = env.reset_device()
        self.dones = env.done_dev
        self.dones.zero_()

    def assign(self, update):
        """Start of an update: the seat's nets re-dealt over the tiles, rotated by one tile per update.  Returns self for a league
        (what ``alg_ppo.league_note`` reads ``tile_member`` of), None for a single net."""
        member = league_tiles(len(self.zoo_seat), self.nenv, update)
        prev = getattr(self, "tile_member", None)
        if prev is not None and self.state is not None:      # a tile that changes its net starts from a zero state, as ZooLeague.assign
            changed = self._t.from_numpy(np.repeat(member != prev, LEAGUE_TILE)).to(self.device)
            self.state[changed] = 0.0
        self.tile_member = member
        self.tile_entry = self._t.from_numpy(self.zoo_seat.entries[self.tile_member].astype(np.int32)).to(self.device)
        self._runs1 = matches._runs(self.tile_entry.cpu().numpy())
        return self if len(self.zoo_seat) > 1 else None

    def _group_streams(self):
        t, G = self._t, getattr(self.env, "groups", 1)
        if G > 1 and self._gstreams is None:
            self._gstreams = [t.cuda.Stream(device=self.device) for _ in range(G)]
        return self._gstreams

    def _alloc(self, T):
        t, N, dev = self._t, self.nenv, self.device
        D0, A0 = self.learner_seat.ob_dim, self.learner_seat.ac_dim
        f32 = t.float32
        B = dict(obs=t.empty((T, N, D0), dtype=f32, device=dev), act=t.empty((T, N, A0), dtype=f32, device=dev),
                 val=t.empty((T, N), dtype=f32, device=dev), nlp=t.empty((T, N), dtype=f32, device=dev),
                 done=t.empty((T, N), dtype=t.uint8, device=dev), rew=t.empty((2, T, N), dtype=f32, device=dev),
                 ep_done=t.empty((T, N), dtype=t.uint8, device=dev), ep_r=t.empty((T, N), dtype=t.float64, device=dev),
                 ep_l=t.empty((T, N), dtype=t.int32, device=dev))
        B["noise0"] = t.randn((T, N, A0), generator=self.model.act_model.gen, device=dev, dtype=f32)
        B["noise1"] = t.randn((T, N, self.zoo_seat.ac_dim), generator=self.gen1, device=dev, dtype=f32)
        return B

    def _step_group(self, B, s, alpha, g, sl):
        env, T, N = self.env, self.nsteps, self.nenv
        n = sl.stop - sl.start
        view = env if g is None else EnvRows(env, sl)
        tiles = slice(sl.start // LEAGUE_TILE, sl.stop // LEAGUE_TILE)
        runs1 = None
        if not self.fused:     # the group's runs of equal entries, in the group's own tile numbers
            runs1 = [(max(a, tiles.start) - tiles.start, min(b, tiles.stop) - tiles.start, e) for a, b, e in self._runs1
                     if a < tiles.stop and b > tiles.start]
        record = dict(obs=B["obs"][s, sl], act=B["act"][s, sl], nlp=B["nlp"][s, sl], val=B["val"][s, sl], done=B["done"][s, sl])
        mixed_step(view, self.learner_seat, self.zoo_seat, self.tile_entry[tiles], None if self.state is None else self.state[sl],
                   B["noise0"][s, sl], B["noise1"][s, sl], None, record, self.fused, self.status, None, runs1)
        if g is None:
            env.step_device(env.act_dev)
        else:
            env.step_device_group(g, env.act_dev)
        st = self._t.cuda.current_stream(self.device).cuda_stream
        ppo_capi.chk(ppo_capi.lib().ppo_post_step(env.info_dev[sl].data_ptr(), n, alpha, B["rew"][0, s, sl].data_ptr(), T * N,
                                                  env.done_dev[sl].data_ptr(), env.ep_r_dev[sl].data_ptr(), env.ep_l_dev[sl].data_ptr(),
                                                  B["ep_done"][s, sl].data_ptr(), B["ep_r"][s, sl].data_ptr(), B["ep_l"][s, sl].data_ptr(), st))

    def run(self, update):
        """One rollout of ``nsteps`` steps.  Returns the 15 fields of ``alg_ppo.Rollout`` in ``Runner.run``'s order and env-major
        layout, agent 0's entries real and agent 1's PLACEHOLDERS: ``obs`` / ``actions`` are pairs (agent 0's rows, None); ``returns``
        / ``masks`` / ``values`` / ``rewards`` are [2][N T] with row 1 from zero-filled inputs (``rewards[1]`` is agent 1's real reward);
        ``neglogpacs[1]`` is +inf, so that no opponent sample counts as usable (``useful_ratio`` 0.0); ``opponent_neglogpacs`` is all
        zeros; ``opp_obs_s`` / ``opp_act_s`` / ``states`` are None; the three ratios are exactly 1."""
        from .runner import EpInfoList, anneal_alpha, sf0, sf01
        t, env = self._t, self.env
        T, N = self.nsteps, self.nenv
        B = self._alloc(T)
        self.last_buffers = B
        alpha = anneal_alpha(update, self.anneal_bound)
        self.status.zero_()
        streams = self._group_streams()
        cur = t.cuda.current_stream(self.device)
        if streams is None:
            for s in range(T):
                self._step_group(B, s, alpha, None, slice(0, N))
        else:
            for st in streams:
                st.wait_stream(cur)
            for s in range(T):
                for g, st in enumerate(streams):
                    with t.cuda.stream(st):
                        self._step_group(B, s, alpha, g, env._gs(g))
            for st in streams:
                cur.wait_stream(st)
        self.obs, self.dones = env.obs_dev, env.done_dev
        f32 = t.float32
        last_values = t.zeros((2, N), dtype=f32, device=self.device)
        self.model.act_model.evaluate(self.obs[:, 0, :], ppo_capi.FWD_VF, out=dict(value=last_values[0]))
        # ppo_vtrace's agent-0 returns read agent 0's rewards, values and done flags only (its clips are the constant 1): agent 1's
        # arrays are zero-filled, and so are both neglogp arrays, which makes the three ratios exactly 1
        val = t.zeros((2, T, N), dtype=f32, device=self.device)
        val[0].copy_(B["val"])
        done = t.zeros((2, T, N), dtype=t.uint8, device=self.device)
        done[0].copy_(B["done"])
        zeros = t.zeros((2, T, N), dtype=f32, device=self.device)
        returns = t.empty((2, T, N), dtype=f32, device=self.device)
        opr, oer, ratio = (t.empty((T, N), dtype=f32, device=self.device) for _ in range(3))
        ppo_capi.chk(ppo_capi.lib().ppo_vtrace(B["rew"].data_ptr(), val.data_ptr(), zeros.data_ptr(), zeros.data_ptr(), done.data_ptr(),
                                               self.dones.contiguous().data_ptr(), last_values.data_ptr(), T, N, float(self.gamma),
                                               float(self.lam), 1.0, 1.0, returns.data_ptr(), opr.data_ptr(), oer.data_ptr(),
                                               ratio.data_ptr(), cur.cuda_stream))
        raise_status(self.status)
        d = B["ep_done"].cpu().numpy().astype(bool)
        rr, ll = B["ep_r"].cpu().numpy(), B["ep_l"].cpu().numpy()
        epinfos = EpInfoList(rr[d], ll[d])
        self.league_scores = None
        if len(self.zoo_seat) > 1:
            self.league_scores = policy_zoo.league_scores(d, rr, ll, self.tile_member, len(self.zoo_seat),
                                                          getattr(env.model, "timestep_limit", 500))
        nlp = t.full((2, T, N), float("inf"), dtype=f32, device=self.device)
        nlp[0].copy_(B["nlp"])
        flat = lambda x: x.swapaxes(0, 1).reshape(N * T, *x.shape[2:])          # [T][N][...] -> env-major rows, as sf01 orders them
        return ((flat(B["obs"]), None), sf01(returns), sf01(done.bool()), (flat(B["act"]), None), sf01(val), sf01(nlp), sf01(B["rew"]),
                sf01(zeros), None, None, None, epinfos, sf0(opr), sf0(oer), sf0(ratio))


# ---- evaluation -----------------------------------------------------------------------------------------------------------
def _seat_steps(env, seats, tiles, state, score, quota, K, noise, fused):
    """K steps of a batch: :func:`mixed_step`, ``env.step_device`` and the score update of ``matches``.  A tile without a table row
    raises ``ValueError``: before the first step on the step-by-step path, after the K steps on the fused one."""
    import torch
    lseat, zseat = seats
    runs0 = runs1 = status = None
    if fused:
        status = torch.zeros(1, dtype=torch.int32, device=env.device)
    else:
        runs0, runs1 = matches._runs(tiles[0].cpu().numpy()), zoo_pairs.seat_runs(tiles[1])
        for side, (runs, seat) in enumerate(((runs0, lseat), (runs1, zseat))):
            for t0, _, e in runs:
                if not 0 <= e < len(seat):
                    raise ValueError("tile %d of seat %d: entry %d names no net of the seat (%d nets)" % (t0, side, e, len(seat)))
    for k in range(int(K)):
        mixed_step(env, lseat, zseat, tiles[1], state, None if noise is None else noise[0][k], None if noise is None else noise[1][k],
                   tiles[0], None, fused, status, runs0, runs1)
        _, info, done, _, _, _ = env.step_device(env.act_dev)
        matches._score_step(score, info, done, quota)
    if fused:
        raise_status(status)


def check_batch_args(env, rounds_per_env, envs_per_pair, chunk, every=1):
    """The four counts of a seat match as ints; ``ValueError`` where a pair would not play whole tiles or a count is below 1."""
    rounds_per_env, envs_per_pair, chunk, every = int(rounds_per_env), int(envs_per_pair), int(chunk), int(every)
    if envs_per_pair < LEAGUE_TILE or envs_per_pair % LEAGUE_TILE:
        raise ValueError("envs_per_pair = %d: a pair plays whole tiles of %d envs" % (envs_per_pair, LEAGUE_TILE))
    if env.num_envs % LEAGUE_TILE:
        raise ValueError("num_envs = %d is not a multiple of %d" % (env.num_envs, LEAGUE_TILE))
    if rounds_per_env < 1 or chunk < 1 or every < 1:
        raise ValueError("rounds_per_env, chunk and every must be >= 1")
    return rounds_per_env, envs_per_pair, chunk, every


def play_seat_batches(env, seats, pairs, rounds_per_env, envs_per_pair, deterministic, seed, adjust_z, chunk, tiles_of, new_state, steps,
                      record=None, every=1):
    """The batch loop of :func:`play_checkpoints_against_seat` and ``co_train.play_checkpoint_pairs``: the pairs in batches of contiguous
    env blocks (:func:`matches.plan_batches`, :func:`matches.env_assignment` over whole tiles); per batch a seeded reset (``seed`` +
    batch number * N + env), ``tiles_of(idx0, idx1)`` (the two seats' int32 tile arrays), a fresh ``new_state()`` and
    ``steps(tiles, state, score, K, noise)`` calls of ``chunk`` steps until every env of the batch has its quota; ``adjust_z``
    imposed and restored.  ``record``: see :func:`play_checkpoints_against_seat`.  Returns one dict per pair."""
    import torch
    N = env.num_envs
    rounds_per_env, envs_per_pair, chunk, every = check_batch_args(env, rounds_per_env, envs_per_pair, chunk, every)
    batches = matches.plan_batches(len(pairs), envs_per_pair, N)
    max_calls = -(-rounds_per_env * (env.model.timestep_limit + 1) // chunk) + 1      # every episode ends by the time limit
    gen = torch.Generator(device=env.device)
    gen.manual_seed(int(seed))
    out = [None] * len(pairs)
    prev_adjust, prev_seeds = getattr(env, "adjust_z", 0.0), env.seeds.copy()
    change_z = adjust_z is not None and float(adjust_z) != prev_adjust
    if change_z:
        env.set_adjust_z(adjust_z)
    try:
        for bn, batch in enumerate(batches):
            idx0, idx1, active = matches.env_assignment(pairs, batch, envs_per_pair, N)
            tiles = tuple(torch.from_numpy(x).to(env.device) for x in tiles_of(idx0, idx1))
            act_t = torch.from_numpy(active).to(env.device)
            score = torch.zeros((N, 3), dtype=torch.int32, device=env.device)
            env.seeds = np.uint64(seed) + np.uint64(bn * N) + np.arange(N, dtype=np.uint64)
            env._needs_seed = True
            env.reset_device()
            env.act_dev.zero_()
            state = new_state()
            rec = record is not None and bn == 0
            qpos, dones, calls = [], [], 0
            while True:
                noise = None if deterministic else tuple(torch.randn((chunk, N, s.ac_dim), generator=gen, device=env.device) for s in seats)
                if rec:                  # the same steps one at a time, the joint positions read in between
                    for k in range(chunk):
                        steps(tiles, state, score, 1, None if noise is None else tuple(z[k:k + 1] for z in noise))
                        if (calls * chunk + k + 1) % every == 0:
                            torch.cuda.synchronize(env.device)
                            qpos.append(np.concatenate([E.get_state()[0] for E in env.engines]))
                            dones.append(env.done_dev[:, 0].cpu().numpy())
                else:
                    steps(tiles, state, score, chunk, noise)
                calls += 1
                if not bool((score.sum(1)[act_t] < rounds_per_env).any()):
                    break
                if calls >= max_calls:
                    raise RuntimeError("matches did not finish within %d calls of %d steps" % (calls, chunk))
            sc = score.cpu().numpy().astype(np.int64)
            for b, p in enumerate(batch):
                s = sc[b * envs_per_pair:(b + 1) * envs_per_pair].sum(0)
                out[p] = dict(wins=int(s[0]), losses=int(s[1]), draws=int(s[2]), rounds=int(s.sum()), env_steps=calls * chunk * envs_per_pair)
            if rec:
                from . import render
                if not qpos:
                    raise ValueError("no frame was recorded: every = %d exceeds the %d steps played" % (every, calls * chunk))
                os.makedirs(str(record), exist_ok=True)
                names = [" ".join(s.labels[k] or "net %d" % k for k in sorted({pairs[p][side] for p in batch})) for side, s in enumerate(seats)]
                render.save_trajectory(os.path.join(str(record), "traj.npz"), np.stack(qpos), np.stack(dones), sc.astype(np.int32),
                                       env.spec.id, names[0], names[1], every)
    finally:
        env.seeds = prev_seeds
        if change_z:
            torch.cuda.synchronize(env.device)
            env.set_adjust_z(prev_adjust)
    return out


def play_checkpoints_against_seat(env, learner_seat, zoo_seat, pairs, rounds_per_env, envs_per_pair, deterministic=True, seed=0,
                                  adjust_z=EVAL_ADJUST_Z, chunk=64, fused=True, record=None, every=1):
    """:func:`zoo_pairs.play_zoo_pairs` with a :class:`LearnerSeat` on side 0: every match-up ``pairs[p] = (i, j)`` -- row i of
    ``learner_seat`` as agent 0 against net j of ``zoo_seat`` as agent 1 -- on ``envs_per_pair`` envs (a multiple of 16),
    ``rounds_per_env`` finished episodes per env, with the same batching (:func:`matches.plan_batches`,
    :func:`matches.env_assignment` over whole tiles), seeded reset (``seed`` + batch number * N + env), per-env quota, score update
    and ``adjust_z`` imposed and restored (:func:`play_seat_batches`).  Deterministic by default, as the reference's evaluator plays.
    ``record``: a directory that receives ``traj.npz`` of the first batch (every ``every``-th step), which ``play.py --replay``
    renders.  Returns one dict per pair: wins, losses, draws, rounds, env_steps."""
    check_batch_args(env, rounds_per_env, envs_per_pair, chunk, every)
    pairs = [(int(i), int(j)) for i, j in pairs]
    for i, j in pairs:
        if not (0 <= i < len(learner_seat) and 0 <= j < len(zoo_seat)):
            raise ValueError("pair (%d, %d) refers to a non-existent net (%d learner rows / %d zoo nets)" % (i, j, len(learner_seat), len(zoo_seat)))
    if getattr(env, "cfrc_mode", "zero") != "zero":
        raise ValueError("the zoo nets were trained on cfrc_mode 'zero' observations")
    seats = (learner_seat, zoo_seat)
    return play_seat_batches(env, seats, pairs, rounds_per_env, envs_per_pair, deterministic, seed, adjust_z, chunk,
                             lambda idx0, idx1: (learner_seat.tile_rows(idx0), zoo_seat.tile_entries(idx1)),
                             lambda: zoo_seat.new_state(env.num_envs),
                             lambda tiles, state, score, K, noise: _seat_steps(env, seats, tiles, state, score, int(rounds_per_env), K, noise, fused),
                             record, every)


def evaluate_history_against_zoo(path, opponent_paths, trials, start=0, interval=1, num_env=256, deterministic=True, fused=True, seed=0,
                                 adjust_z=EVAL_ADJUST_Z, env_id="RoboSumo-Ant-vs-Bug-v0", chunk=64, env=None, record=None, every=1):
    """:func:`matches.evaluate_history_against_zoo` for a run on a mixed match-up: every selected checkpoint of run ``path`` as agent
    0 against every policy-zoo file of ``opponent_paths`` (agent 1's species, MLP and LSTM mixed: one seat plays both families) as
    agent 1, exactly ``trials`` games per (checkpoint, opponent) -- a multiple of 16, split by :func:`zoo_pairs.split_trials16` --
    batched over the envs by :func:`play_checkpoints_against_seat`.  Returns the same dict: checkpoints, opponents,
    results={(id, k): dict(win, draw, lose, rounds, env_steps)}, opponent_networks, network / nlstm of the run."""
    if isinstance(opponent_paths, (str, os.PathLike)):
        opponent_paths = [opponent_paths]
    opponent_paths = [str(p) for p in opponent_paths]
    ck = matches.checkpoint_dir(path)
    ids = matches.select_checkpoints([f for f in os.listdir(ck) if f.isdigit() and os.path.isfile(os.path.join(ck, f))], start, interval)
    if not ids:
        raise ValueError("no checkpoints to evaluate in %s" % ck)
    ck_paths = [os.path.join(ck, "%.5i" % c) for c in ids]
    kind = matches.checkpoint_kind(ck_paths[0])
    if kind[0] != "mlp":
        raise NotImplementedError("mixed match-ups: the learner's seat holds MLP(64,64) checkpoints, %s holds %s ones" % (ck, matches._kind_name(kind)))
    epp, rounds = zoo_pairs.split_trials16(trials, num_env if env is None else env.num_envs)
    env, own = matches._make_env(env_id, num_env, seed, env)
    try:
        if not is_mixed(env):
            raise ValueError("%s is a homogeneous match-up: matches.evaluate_history_against_zoo evaluates it" % env.spec.id)
        lseat = LearnerSeat(env.model.obs_dims[0], env.model.act_dims[0], ck_paths, env.device)
        zseat = zoo_pairs.seat_for(env, 1, opponent_paths)
        pairs = [(c, o) for c in range(len(lseat)) for o in range(len(zseat))]
        res = play_checkpoints_against_seat(env, lseat, zseat, pairs, rounds, epp, deterministic=deterministic, seed=seed,
                                            adjust_z=adjust_z, chunk=chunk, fused=fused, record=record, every=every)
    finally:
        if own:
            env.close()
    results = {}
    for (c, o), r in zip(pairs, res):
        n = float(r["rounds"])
        results[(ids[c], o)] = dict(win=r["wins"] / n, draw=r["draws"] / n, lose=r["losses"] / n, rounds=r["rounds"], env_steps=r["env_steps"])
    return dict(checkpoints=ids, opponents=opponent_paths, results=results, opponent_networks=list(zseat.kinds), **matches._network(kind))
