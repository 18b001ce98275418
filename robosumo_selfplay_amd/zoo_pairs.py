"""Policy-zoo nets against each other on any of the nine match-ups: one zoo net on each side, MLP and LSTM mixed, the two
sides of different species where the scene is mixed (``RoboSumo-Ant-vs-Bug-v0``, ...).

Reference: robosumo/demos/play.py (one zoo net per side of any scene, ``stochastic=True``, ``agent._adjust_z = -0.5``,
``policy.reset()`` at every episode start).

A :class:`ZooSeat` holds the nets that may play ONE side: a :class:`policy_zoo.ZooTable` of its MLP nets and a
:class:`policy_zoo.ZooLstmTable` of its LSTM nets.  Every 16-env tile of a batch plays one of them, named by its table entry in
the encoding of :func:`policy_zoo.league_entries`.  :func:`seat_act` makes one seat's actions of one step -- fused: ONE
``ppo_zoo_seat_act`` launch straight from the env's observation / done buffers into its action buffer; ``fused=False``: the
definition, the existing ``ppo_forward_filtered`` / ``ppo_lstm_step`` launches per run of tiles that share a net -- and
:func:`pair_steps` / :func:`play_zoo_pairs` / :func:`tournament` drive ``SumoVecEnv.step_device`` with it.  ``matches`` and
``play.py`` keep refusing mixed scenes and zoo nets on agent 0: their launches put both policies inside the engine's fused
kernel, which is built for one observation / action space.
"""
import ctypes as C
import os

import numpy as np

from . import matches, policy_zoo, ppo_capi
from .policy_zoo import EVAL_ADJUST_Z, LEAGUE_TILE

STATE_WIDTH = 2 * policy_zoo.HIDDEN    # c | h of a zoo LSTM(64) net


def _device(device):
    import torch
    if isinstance(device, torch.device):
        return device
    return torch.device(device) if isinstance(device, str) else torch.device("cuda", int(device))


def _zoo_dims(nparams, kind, ac_dim):
    """Observation width of a flat zoo vector of family ``kind`` with ``ac_dim`` actions."""
    count = policy_zoo.zoo_mlp_param_count if kind == "mlp" else policy_zoo.zoo_lstm_param_count
    c0 = count(0, ac_dim)
    return (int(nparams) - c0) // (count(1, ac_dim) - c0)


class ZooSeat(object):
    """The zoo nets of one side.  ``sources``: ``.npy`` paths or flat vectors, each sorted into its family by
    :func:`policy_zoo.zoo_file_kind`; ``kinds[k]`` / ``entries[k]`` / ``labels[k]`` are net k's family, table entry
    (:func:`policy_zoo.league_entries`) and path (None for a vector).  ``mlp_table`` / ``lstm_table``: the device tables, None
    where the seat has no net of that family.  A net whose observation or action width is not the seat's is refused (an ant net
    cannot sit on a bug seat)."""

    def __init__(self, sources, ob_dim, ac_dim, device=0):
        self.device = _device(device)
        self.ob_dim, self.ac_dim = int(ob_dim), int(ac_dim)
        sources = list(sources)
        if not sources:
            raise ValueError("a seat needs at least one zoo net")
        flats, self.labels, self.kinds = [], [], []
        for k, src in enumerate(sources):
            is_path = isinstance(src, (str, os.PathLike))
            label = str(src) if is_path else None
            flat = np.asarray(np.load(os.path.expanduser(str(src)), allow_pickle=False) if is_path else src, np.float32).ravel()
            name = "net %d%s" % (k, " (%s)" % label if label else "")
            try:
                kind = policy_zoo.zoo_file_kind(flat.size, self.ac_dim)
            except ValueError as e:
                raise ValueError("%s does not fit this seat (%d observation columns, %d actions; another species?): %s"
                                 % (name, self.ob_dim, self.ac_dim, e))
            D = _zoo_dims(flat.size, kind, self.ac_dim)
            if D != self.ob_dim:
                raise ValueError("%s reads %d observation columns, the seat has %d (another species?)" % (name, D, self.ob_dim))
            flats.append(flat)
            self.labels.append(label)
            self.kinds.append(kind)
        self.entries, self.n_mlp, self.n_lstm = policy_zoo.league_entries(self.kinds)
        self.flats = flats
        mlp = [f for f, k in zip(flats, self.kinds) if k == "mlp"]
        lstm = [f for f, k in zip(flats, self.kinds) if k == "lstm"]
        self.mlp_table = policy_zoo.ZooTable(mlp, self.ac_dim, self.device) if mlp else None
        self.lstm_table = policy_zoo.ZooLstmTable(lstm, self.ac_dim, self.device) if lstm else None

    def __len__(self):
        return len(self.kinds)

    @property
    def recurrent(self):
        return self.n_lstm > 0

    def new_state(self, n):
        """Fresh all-zero recurrent state rows [n][128] (c | h) for this seat; None for a seat without LSTM nets."""
        import torch
        return torch.zeros((int(n), STATE_WIDTH), dtype=torch.float32, device=self.device) if self.recurrent else None

    def tile_entries(self, env_net):
        """int32 [n / 16] table entries of the tiles of a batch whose env e plays net ``env_net[e]`` of this seat; the 16 envs of
        a tile must share their net."""
        env_net = np.asarray(env_net, np.int64)
        if env_net.ndim != 1 or env_net.size < LEAGUE_TILE or env_net.size % LEAGUE_TILE:
            raise ValueError("a seat plays whole tiles of %d envs, got %d envs" % (LEAGUE_TILE, env_net.size))
        tiles = env_net.reshape(-1, LEAGUE_TILE)
        if (tiles != tiles[:, :1]).any():
            raise ValueError("the %d envs of a tile play one net" % LEAGUE_TILE)
        if tiles.min() < 0 or tiles.max() >= len(self):
            raise ValueError("net index outside [0, %d)" % len(self))
        return self.entries[tiles[:, 0]].astype(np.int32)

    def struct(self, tile_entry, state):
        """The ``ppo_capi.ZooSeat`` launch struct (the tensors stay owned by their holders)."""
        z = ppo_capi.ZooSeat()
        if self.mlp_table is not None:
            z.mlp_params, z.mlp_filt = self.mlp_table.params.data_ptr(), self.mlp_table.filt.data_ptr()
        if self.lstm_table is not None:
            z.lstm_params, z.lstm_filt = self.lstm_table.params.data_ptr(), self.lstm_table.filt.data_ptr()
        z.tile_entry = tile_entry.data_ptr()
        z.state = None if state is None else state.data_ptr()
        z.n_mlp, z.n_lstm, z.ob_dim, z.ac_dim = self.n_mlp, self.n_lstm, self.ob_dim, self.ac_dim
        z.obs_clip, z.forget_bias = policy_zoo.ZooTable.obs_clip, policy_zoo.ZooLstmTable.forget_bias
        return z


def seat_for(env, side, sources):
    """The :class:`ZooSeat` of agent ``side`` of ``env``: the zoo nets read the agent's observation without its last column."""
    return ZooSeat(sources, env.model.obs_dims[side] - 1, env.model.act_dims[side], env.device)


def seat_runs(tile_entry):
    """Host runs (first tile, end tile, entry) of equal consecutive tile entries: what the step-by-step path launches on."""
    import torch
    te = tile_entry.cpu().numpy() if torch.is_tensor(tile_entry) else np.asarray(tile_entry)
    return matches._runs(te)


def _check_step(seat, env, side, tile_entry, state, noise):
    import torch
    N = env.num_envs
    if N < LEAGUE_TILE or N % LEAGUE_TILE:
        raise ValueError("a seat plays whole tiles of %d envs: num_envs = %d" % (LEAGUE_TILE, N))
    if (seat.ob_dim, seat.ac_dim) != (env.model.obs_dims[side] - 1, env.model.act_dims[side]):
        raise ValueError("the seat's nets (%d observation columns, %d actions) do not fit agent %d of %s (%d, %d)"
                         % (seat.ob_dim, seat.ac_dim, side, env.spec.id, env.model.obs_dims[side] - 1, env.model.act_dims[side]))
    if not torch.is_tensor(tile_entry) or tile_entry.dtype != torch.int32 or tuple(tile_entry.shape) != (N // LEAGUE_TILE,) \
            or not tile_entry.is_contiguous() or tile_entry.device != env.device:
        raise ValueError("tile_entry must be a contiguous int32 tensor [%d] on the env's device" % (N // LEAGUE_TILE))
    if seat.recurrent and (state is None or tuple(state.shape) != (N, STATE_WIDTH) or state.dtype != torch.float32
                           or not state.is_contiguous()):
        raise ValueError("a seat with LSTM nets needs a contiguous float32 state [%d][%d] (c | h)" % (N, STATE_WIDTH))
    if noise is not None and (tuple(noise.shape) != (N, seat.ac_dim) or noise.dtype != torch.float32 or not noise.is_contiguous()):
        raise ValueError("noise must be a contiguous float32 tensor [%d][%d]" % (N, seat.ac_dim))


def seat_act(seat, env, side, tile_entry, state, noise, fused=True, runs=None, status=None):
    """Agent ``side``'s actions of one step, from ``env.obs_dev[:, side]`` into ``env.act_dev[:, side, :ac_dim]``: tile t is played
    by the net with table entry ``tile_entry[t]`` (int32 CUDA [N / 16]).  ``state``: the seat's recurrent state [N][128], rows of
    LSTM tiles zeroed where ``env.done_dev[:, 0]`` (agent 0's flag of the previous step, as ``policy_zoo._evaluate_against``
    resets its opponent) is set and then advanced in place; None for a seat without LSTM nets.  ``noise``: float32 [N][ac_dim]
    standard-normal rows, None = the means.

    ``fused``: one ``ppo_zoo_seat_act`` launch; a tile whose entry names no net writes nothing and leaves 1 + tile in ``status``
    (int32 CUDA [1], optional).  ``fused=False`` is the definition: for every run of tiles with one entry (``runs``, default
    :func:`seat_runs` of ``tile_entry``, a device read) ``ppo_forward_filtered`` with that row's parameters and filter, or
    ``ppo_lstm_step`` with that row's ``ZooLstmTable.nets[k]`` on the run's state rows, float mask and noise rows, copied into
    the action buffer; runs whose entry names no net are skipped."""
    import torch
    _check_step(seat, env, side, tile_entry, state, noise)
    N, D, A = env.num_envs, seat.ob_dim, seat.ac_dim
    L, st, obs, act = ppo_capi.lib(), env._stream(), env.obs_dev, env.act_dev
    if fused:
        z = seat.struct(tile_entry, state)
        ppo_capi.chk(L.ppo_zoo_seat_act(C.byref(z), obs[:, side].data_ptr(), N, obs.stride(0), env.done_dev.data_ptr(), env.done_dev.stride(0),
                                        ppo_capi.ptr(noise), act[:, side].data_ptr(), act.stride(0), ppo_capi.ptr(status), st))
        return
    out = torch.empty((N, A), dtype=torch.float32, device=env.device)
    mask = env.done_dev[:, 0].to(torch.float32) if seat.recurrent else None
    for t0, t1, e in (seat_runs(tile_entry) if runs is None else runs):
        rows = slice(LEAGUE_TILE * t0, LEAGUE_TILE * t1)
        n, nz = rows.stop - rows.start, None if noise is None else noise[rows]
        if 0 <= e < seat.n_mlp:
            tb = seat.mlp_table
            ppo_capi.chk(L.ppo_forward_filtered(tb.params[e].data_ptr(), obs[rows, side].data_ptr(), n, obs.stride(0), D, A,
                                                ppo_capi.FWD_PI | ppo_capi.FWD_TANH, tb.filt[e, 0].data_ptr(), tb.filt[e, 1].data_ptr(),
                                                tb.obs_clip, ppo_capi.ptr(nz), None, out[rows].data_ptr(), None, None, None, st))
        elif seat.n_mlp <= e < seat.n_mlp + seat.n_lstm:
            S = state[rows]
            ppo_capi.chk(L.ppo_lstm_step(C.byref(seat.lstm_table.nets[e - seat.n_mlp]), obs[rows, side].data_ptr(), n, obs.stride(0),
                                         mask[rows].data_ptr(), S.data_ptr(), S.data_ptr() + 4 * policy_zoo.HIDDEN, STATE_WIDTH,
                                         ppo_capi.ptr(nz), None, out[rows].data_ptr(), None, None, None, st))
        else:
            continue
        act[rows, side, :A] = out[rows]


def pair_steps(env, seats, tile_entries, states, score, quota, K, noise=None, fused=True):
    """K steps of a batch of zoo-vs-zoo games: per step :func:`seat_act` for seat 0 and for seat 1, ``env.step_device`` on the
    env's own action buffer and the score update of ``matches`` (score int32 CUDA [N][3]: agent 0 wins, agent 1 wins, draws; an
    env stops counting at ``quota`` finished episodes).  ``tile_entries`` / ``states``: one per seat, as :func:`seat_act` takes
    them; ``noise``: None or a pair of float32 CUDA [K][N][ac_dim of that side] tensors (the widths differ on mixed scenes).  A
    tile entry that names no net raises ``ValueError``: before the first step on the step-by-step path, after the K steps
    (which such a tile played with the actions left in the buffer) on the fused one."""
    import torch
    K = int(K)
    runs = [None, None]
    status = None
    if fused:
        status = torch.zeros(1, dtype=torch.int32, device=env.device)
    else:
        for side in range(2):
            runs[side] = seat_runs(tile_entries[side])
            for t0, _, e in runs[side]:
                if not 0 <= e < len(seats[side]):
                    raise ValueError("tile %d of seat %d: entry %d names no net of the seat (%d nets)" % (t0, side, e, len(seats[side])))
    for k in range(K):
        for side in range(2):
            seat_act(seats[side], env, side, tile_entries[side], states[side], None if noise is None else noise[side][k], fused,
                     runs[side], status)
        _, info, done, _, _, _ = env.step_device(env.act_dev)
        matches._score_step(score, info, done, quota)
    if fused:
        bad = int(status.item())
        if bad:
            raise ValueError("tile %d: its entry names no net of the seat" % (bad - 1))


def play_zoo_pairs(env, seat0, seat1, pairs, rounds_per_env, envs_per_pair, deterministic=False, seed=0, adjust_z=EVAL_ADJUST_Z,
                   chunk=64, fused=True, record=None, every=1):
    """Plays every match-up ``pairs[p] = (i, j)`` -- net i of ``seat0`` as agent 0 against net j of ``seat1`` as agent 1 -- on
    ``envs_per_pair`` envs (a multiple of 16), ``rounds_per_env`` finished episodes per env, with the batching of
    :func:`matches.play_matches` (:func:`matches.plan_batches`, :func:`matches.env_assignment`): per batch a seeded reset
    (``seed`` + batch number * N + env), fresh zero recurrent states and ``chunk``-step calls of :func:`pair_steps` until every
    env of the batch has its quota.  Stochastic by default, as the reference's demo plays.  ``adjust_z`` is imposed for the games
    and the env's value restored afterwards (None: leave it).  ``record``: a directory that receives ``traj.npz``
    (``render.save_trajectory``) with every ``every``-th joint position of the FIRST batch's envs, which ``play.py --replay``
    renders.  Returns one dict per pair: wins, losses, draws, rounds (== envs_per_pair * rounds_per_env), env_steps."""
    import torch
    N = env.num_envs
    rounds_per_env, envs_per_pair, chunk, every = int(rounds_per_env), int(envs_per_pair), int(chunk), int(every)
    if envs_per_pair < LEAGUE_TILE or envs_per_pair % LEAGUE_TILE:
        raise ValueError("envs_per_pair = %d: a pair plays whole tiles of %d envs" % (envs_per_pair, LEAGUE_TILE))
    if N % LEAGUE_TILE:
        raise ValueError("num_envs = %d is not a multiple of %d" % (N, LEAGUE_TILE))
    if rounds_per_env < 1 or chunk < 1 or every < 1:
        raise ValueError("rounds_per_env, chunk and every must be >= 1")
    pairs = [(int(i), int(j)) for i, j in pairs]
    for i, j in pairs:
        if not (0 <= i < len(seat0) and 0 <= j < len(seat1)):
            raise ValueError("pair (%d, %d) refers to a non-existent zoo net (%d / %d nets)" % (i, j, len(seat0), len(seat1)))
    if getattr(env, "cfrc_mode", "zero") != "zero":
        raise ValueError("the zoo nets were trained on cfrc_mode 'zero' observations")
    seats = (seat0, seat1)
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
            tiles = tuple(torch.from_numpy(s.tile_entries(idx)).to(env.device) for s, idx in zip(seats, (idx0, idx1)))
            act_t = torch.from_numpy(active).to(env.device)
            score = torch.zeros((N, 3), dtype=torch.int32, device=env.device)
            env.seeds = np.uint64(seed) + np.uint64(bn * N) + np.arange(N, dtype=np.uint64)
            env._needs_seed = True
            env.reset_device()
            env.act_dev.zero_()
            states = tuple(s.new_state(N) for s in seats)
            rec = record is not None and bn == 0
            qpos, dones, calls = [], [], 0
            while True:
                noise = None if deterministic else tuple(torch.randn((chunk, N, s.ac_dim), generator=gen, device=env.device) for s in seats)
                if rec:                  # the same steps one at a time, the joint positions read in between
                    for k in range(chunk):
                        pair_steps(env, seats, tiles, states, score, rounds_per_env, 1, None if noise is None else tuple(z[k:k + 1] for z in noise), fused)
                        if (calls * chunk + k + 1) % every == 0:
                            torch.cuda.synchronize(env.device)
                            qpos.append(np.concatenate([E.get_state()[0] for E in env.engines]))
                            dones.append(env.done_dev[:, 0].cpu().numpy())
                else:
                    pair_steps(env, seats, tiles, states, score, rounds_per_env, chunk, noise, fused)
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


def split_trials16(trials, num_env):
    """(envs_per_pair, rounds_per_env) for ``trials`` games of a pair on whole tiles: envs_per_pair the largest multiple of 16 that
    divides ``trials`` and fits ``num_env`` envs.  ``trials`` must be a multiple of 16."""
    trials, num_env = int(trials), int(num_env)
    if trials < LEAGUE_TILE or trials % LEAGUE_TILE:
        raise ValueError("trials = %d: a pair plays whole tiles of %d envs, so a multiple of %d games" % (trials, LEAGUE_TILE, LEAGUE_TILE))
    if num_env < LEAGUE_TILE or num_env % LEAGUE_TILE:
        raise ValueError("num_env = %d must be a multiple of %d" % (num_env, LEAGUE_TILE))
    epp = max(d for d in range(LEAGUE_TILE, min(trials, num_env) + 1, LEAGUE_TILE) if trials % d == 0)
    return epp, trials // epp


def tournament(env_id, files0, files1, trials, num_env=256, env=None, **kw):
    """Every net of ``files0`` as agent 0 against every net of ``files1`` as agent 1 of ``env_id``, ``trials`` games per pair (a
    multiple of 16) on ``num_env`` envs; ``kw`` goes to :func:`play_zoo_pairs` (deterministic, seed, adjust_z, chunk, fused,
    record, every).  Returns dict(env_id, trials, labels0, labels1, kinds0, kinds1, counts int64 [len0][len1][3] = agent 0 wins,
    agent 1 wins, draws, results = the dicts of :func:`play_zoo_pairs` in row-major pair order)."""
    files0, files1 = list(files0), list(files1)
    epp, rounds = split_trials16(trials, num_env)
    env, own = matches._make_env(env_id, num_env, int(kw.get("seed", 0)), env)
    try:
        seat0, seat1 = seat_for(env, 0, files0), seat_for(env, 1, files1)
        pairs = [(i, j) for i in range(len(seat0)) for j in range(len(seat1))]
        res = play_zoo_pairs(env, seat0, seat1, pairs, rounds, epp, **kw)
        counts = np.zeros((len(seat0), len(seat1), 3), np.int64)
        for (i, j), r in zip(pairs, res):
            counts[i, j] = r["wins"], r["losses"], r["draws"]
        label = lambda seat: [seat.labels[k] or "%s %d" % (seat.kinds[k], k) for k in range(len(seat))]
        return dict(env_id=env.spec.id, trials=int(trials), labels0=label(seat0), labels1=label(seat1), kinds0=list(seat0.kinds),
                    kinds1=list(seat1.kinds), counts=counts, results=res)
    finally:
        if own:
            env.close()
