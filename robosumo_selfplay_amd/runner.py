"""Rollout engine with the reference ``Runner``'s constructor and 15-tuple ``run(update)`` contract (runner.py:7-252).

Two modes, same arithmetic (csrc/ppo_kernels.hip: reward curriculum, IS ratios, V-trace):
  * device mode  -- ``env`` is a ``SumoVecEnv`` and the models are ``PPOModel``s: observations, actions, rewards and
    dones never leave HBM between the env step kernel and the policy kernels; ``run`` returns CUDA tensors.
  * host mode    -- any duck-typed VecEnv / models like the reference's: numpy per step (their API), then the collected
    buffers go through the same kernels; ``run`` returns numpy arrays (this is what the golden-vector tests drive).

Device mode is the product of two axes -- who the learner is (an MLP(64,64) ``PolicyWithValue`` or an ``LstmPPOModel``) and who
plays agent 1 (the other self-play net or a pool of its snapshots, one policy-zoo net, a league of them).  ``Runner.rollout_mode``
resolves the pair once per call into a :class:`RolloutMode`; the fused driver (``_launch_steps``), the step-by-step evaluator
(``_evaluate_step``) and the noise draw (``_noise_rows``) are each written once against the two sides.
"""
import ctypes as C
import functools
import os
from collections import namedtuple

import numpy as np

from . import capi, ppo_capi
from .lstm_model import LstmPPOModel
from .opponent_pool import LstmOpponentPool
from .policies import PolicyWithValue
from .policy_zoo import FixedOpponentModel, ZooLeague, ZooLSTMPolicy, ZooLstmTable, ZooMLPPolicy, ZooTable, league_scores


def sf01(arr):
    """runner.py:255-260 (numpy or torch)"""
    s = arr.shape
    return arr.swapaxes(1, 2).reshape(s[0], s[1] * s[2], *s[3:])


def sf0(arr):
    """runner.py:263-267"""
    return arr.swapaxes(0, 1).reshape(-1)


def anneal_alpha(update, anneal_bound):
    """runner.py:128-130"""
    if update <= anneal_bound:
        return float(np.linspace(1, 0, anneal_bound)[update - 1])
    return 0.0


class EpInfoList(object):
    """The rollout's episode records of agent 0 (monitor.py:63-78: ``{'r', 'l', 't'}`` per finished episode, in (step, env) order) as
    a read-only sequence that builds its dicts on demand: a 4096-env rollout ends ~10 000 episodes, the driver looks at the last
    100 (``epinfobuf = deque(maxlen=100)``, alg_ppo.py:160), and 10 000 Python dicts per update cost 8 ms of a 270 ms iteration.
    Behaves like the reference's list for ``len`` / iteration / indexing / slicing / ``deque.extend`` / ``==``."""

    def __init__(self, r, l):
        self._r = np.round(np.asarray(r, np.float64), 6)
        self._l = np.asarray(l, np.int64)

    def __len__(self):
        return int(self._r.shape[0])

    def _make(self, i):
        return {"r": float(self._r[i]), "l": int(self._l[i]), "t": 0.0}

    def arrays(self):
        """The episodes' returns and lengths as two arrays (what the run log's monitor file writes without building the dicts)."""
        return self._r, self._l

    def __getitem__(self, i):
        if isinstance(i, slice):
            return EpInfoList(self._r[i], self._l[i])
        return self._make(range(len(self))[i])

    def __iter__(self):
        return (self._make(i) for i in range(len(self)))

    def __eq__(self, other):
        if isinstance(other, EpInfoList):
            return np.array_equal(self._r, other._r) and np.array_equal(self._l, other._l)
        return list(self) == list(other)

    def __repr__(self):
        return "EpInfoList(%d episodes)" % len(self)


class _nullctx(object):
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


# ---- the rollout mode: (learner, who plays agent 1) ---------------------------------------------------------------------------
Launch = namedtuple("Launch", "entry struct selector family")
RolloutMode = namedtuple("RolloutMode", "learner opponent zoo reuse noise_rows fused entry launch one_launch")
RolloutMode.__doc__ = """What a device-mode rollout plays, resolved from the runner's state by ``Runner.rollout_mode``.

``learner``: 'mlp' or 'lstm'.  ``opponent``: 'self' (the other self-play net, or a pool of snapshots), 'zoo' (one policy-zoo net) or
'league'.  ``zoo``: the ``ZooMLPPolicy`` / ``ZooLSTMPolicy`` / ``ZooLeague`` on agent 1, else None.  ``reuse``: recurrent
opponent-data reuse.  ``noise_rows``: the action noise is drawn per group for the whole buffer (``Runner._noise_rows``), the rows a
fused launch reads; otherwise every net draws per step from its own generator.  ``fused``: a fused launch applies, and ``entry`` is
its ``SumoVecEnv`` method (else None).  ``launch``: the pair's :func:`rollout_launch`, whether it applies or not.  ``one_launch``:
the step-by-step path evaluates both nets in one ``ppo_selfplay_forward`` (MLP self-play of the env's shape)."""

REUSE_REFUSED = "reuse_opponent: recurrent self-play only (no policy-zoo opponent)"


def rollout_launch(learner, opponent, family=None, reuse=False):
    """The fused launch of a (learner, opponent) pair -- the engine's ``sumo_rollout_steps[_lstm][_zoo|_zoo_lstm|_zoo_league|_reuse]``;
    needs no GPU, env or model.  ``learner``: 'mlp' / 'lstm'; ``opponent``: 'self' / 'zoo' / 'league'; ``family``: 'mlp' / 'lstm' for a
    zoo net, the composition (nmlp, nlstm) for a league (of one family: that family's launch with its index array filled).
    Returns ``Launch(entry, struct, selector, family)``: the ``SumoVecEnv`` method (``sumo_`` + the name without ``_group`` is the
    library's symbol), the ``capi`` launch struct, the struct's field that selects agent 1's net -- ``opponent_index`` per env,
    ``tile_net_dev`` per 16-env tile; None for a mixed league, whose own struct carries the per-tile entries -- and the family
    ('mlp' / 'lstm' / 'league'; None in self-play).  None where the pair has no launch; reuse against a zoo net or a league raises."""
    if reuse and opponent != "self":
        raise NotImplementedError(REUSE_REFUSED)
    if reuse and learner != "lstm":
        return None
    lstm = learner == "lstm"
    if opponent == "self":
        family, suffix = None, "_reuse" if reuse else ""
    else:
        if not isinstance(family, str):
            nmlp, nlstm = family
            family = "league" if nmlp and nlstm else "lstm" if nlstm else "mlp"
        suffix = {"mlp": "_zoo", "lstm": "_zoo_lstm", "league": "_zoo_league"}[family]
    return Launch("rollout_steps" + ("_lstm" if lstm else "") + suffix + "_group",
                  ("RolloutLstmReuse" if reuse else "RolloutLstm") if lstm else "Rollout",
                  None if family == "league" else "tile_net_dev" if lstm else "opponent_index", family)


def _self_play(learner, reuse=False):
    la = rollout_launch(learner, "self", None, reuse)
    return RolloutMode(learner, "self", None, reuse, True, True, la.entry, la, False)


class AbstractEnvRunner(object):
    def __init__(self, *, env, models, nsteps, nagent, anneal_bound):
        self.env, self.models = env, models
        self.nenv = env.num_envs
        self.nagent = nagent
        self.nsteps = nsteps
        self.anneal_bound = anneal_bound
        self.states = [m.initial_state for m in models]


class Runner(AbstractEnvRunner):
    def __init__(self, *, env, models, nsteps, nagent, gamma, lam, rho_bar, c_bar, anneal_bound=500, device=None):
        super().__init__(env=env, models=models, nsteps=nsteps, nagent=nagent, anneal_bound=anneal_bound)
        import torch
        if not torch.cuda.is_available():
            raise ppo_capi.PpoHipError("Runner needs a HIP device (no CPU fallback in the product path)")
        ppo_capi.lib()
        self._t = torch
        if nagent != 2:
            raise ValueError("two-agent self-play only (runner.py assumes agents 0 and 1)")
        self.lam, self.gamma, self.rho_bar, self.c_bar = lam, gamma, rho_bar, c_bar
        self._side = None
        self._gstreams = None
        self._gsides = None
        # device mode, MLP policies: the whole step loop of a rollout runs inside the env engine's fused rollout launch
        # (sumo_rollout_steps); SUMO_FUSED_ROLLOUT=0 keeps the step-by-step launches (same numbers, bit for bit)
        self.fused_rollout = os.environ.get("SUMO_FUSED_ROLLOUT", "1") != "0"
        self.rollout_chunk = int(os.environ.get("SUMO_ROLLOUT_CHUNK", "0"))   # steps per launch (0 = the whole rollout)
        self.opponent_pool = None     # opponent_pool.OpponentPool: frozen snapshots + per-env snapshot index (fused path)
        # opt-in (learn(fused_fix_opponent=True)): a policy-zoo opponent (opponent_mode='fix') plays inside the fused launch
        # (sumo_rollout_steps_zoo for an MLP net, sumo_rollout_steps_zoo_lstm for an LSTM net; sumo_rollout_steps_lstm_zoo /
        # sumo_rollout_steps_lstm_zoo_lstm where the learner is an LSTM(128)).  The action noise is then drawn per
        # group and generator for the whole buffer, as the MLP self-play path draws it -- another, equally valid stream than the
        # per-step draws of the default fix-mode path; with SUMO_FUSED_ROLLOUT=0 the step-by-step launches play that same stream
        # (bit-identical rollouts).
        self.fused_fix_opponent = False
        self._zoo_table = None
        self.zoo_state = None         # device mode: agent 1's recurrent state [nenv][128] (c | h) when a zoo LSTM net plays it
        self.league_scores = None     # a league on agent 1: int64 [members][4] of the last rollout (policy_zoo.league_scores)
        self.recurrent = all(getattr(m, "recurrent", False) for m in models)
        # opt-in (learn(network='lstm', use_opponent_data=...)): opponent-data reuse for a recurrent learner.  BPTT re-evaluates agent 1's
        # rows along agent 1's sequence, so the learner carries a state of its own along that stream -- ``shadow_state`` -- and the
        # rollout records agent 1's value and neglogp from it (one evaluation) instead of the value from the opponent's state and the
        # neglogp from a zero state.  Everything else of the rollout is untouched.  Set before the first ``run``.
        self.reuse_opponent = False
        self.shadow_state = self.shadow_state0 = None
        self.device_mode = hasattr(env, "step_device") and (self.recurrent or all(
            hasattr(m, "act_model") and hasattr(m.act_model, "evaluate") for m in models))
        self.device = getattr(env, "device", None) or device or torch.device("cuda", 0)
        ob_shape = env.observation_space[0].shape
        self.ob_dim = ob_shape[0]
        if len(env.observation_space) > 1 and (env.observation_space[1].shape != ob_shape or
                                               env.action_space[1].shape != env.action_space[0].shape):
            # the reference sizes its buffers and both policies from observation_space[0] as well (runner.py:14-16)
            raise ValueError("self-play rollouts need both agents to share observation and action spaces; mixed match-ups "
                             "(%s vs %s) run in the env engine and the evaluator only"
                             % (ob_shape, env.observation_space[1].shape))
        if self.device_mode:
            self.obs = env.reset_device()                               # [N, 2, D] float32, stays in HBM
            self.dones = torch.zeros((self.nenv, 2), dtype=torch.uint8, device=self.device)
            if self.recurrent:                                          # recurrent states live on the device as well
                self.states = [torch.as_tensor(np.asarray(st, np.float32)).to(self.device) for st in self.states]
            # a zoo LSTM opponent (installed after construction, opponent_mode='fix') acts from these rows on either path; they
            # persist across run() calls and across the K-step launches of one rollout
            self.zoo_state = torch.zeros((self.nenv, 128), dtype=torch.float32, device=self.device)
            if self.recurrent:    # [nenv, 2 nlstm], persists across run() calls like ``states`` (read only with ``reuse_opponent``)
                self.shadow_state = torch.zeros_like(self.states[0])
        else:
            self.obs = np.zeros((self.nenv, len(env.observation_space)) + ob_shape,
                                dtype=models[0].train_model.X.dtype.name)
            self.obs[:] = env.reset()
            self.dones = np.array([[False for _ in range(nagent)] for _ in range(self.nenv)])

    # ---- shared tail: IS ratios + V-trace on the device ---------------------------------------------------------
    def _vtrace(self, rewards, values, nlp, onlp, dones, last_dones, last_values):
        t = self._t
        T, N = self.nsteps, self.nenv
        returns = t.empty((2, T, N), dtype=t.float32, device=self.device)
        opr = t.empty((T, N), dtype=t.float32, device=self.device)
        oer = t.empty_like(opr)
        ratio = t.empty_like(opr)
        st = t.cuda.current_stream(self.device).cuda_stream
        ppo_capi.chk(ppo_capi.lib().ppo_vtrace(rewards.data_ptr(), values.data_ptr(), nlp.data_ptr(), onlp.data_ptr(), dones.data_ptr(),
                                               last_dones.data_ptr(), last_values.data_ptr(), T, N, float(self.gamma), float(self.lam),
                                               float(self.rho_bar), float(self.c_bar), returns.data_ptr(), opr.data_ptr(),
                                               oer.data_ptr(), ratio.data_ptr(), st))
        return returns, opr, oer, ratio

    def run(self, update):
        return self._run_device(update) if self.device_mode else self._run_host(update)

    # ---- device mode: which rollout this is ---------------------------------------------------------------------
    def rollout_mode(self):
        """The :class:`RolloutMode` of the runner's state now -- ``models[1]`` is swapped after construction (a fixed opponent, an LSTM
        pool) and the opt-ins are set afterwards, so nothing here is cached.  No side effects."""
        env, (m0, m1), lstm = self.env, self.models, self.recurrent
        learner = "lstm" if lstm else "mlp"
        fixed = isinstance(m1, FixedOpponentModel)
        zoo = m1.act_model if fixed else None
        if not fixed:
            opponent, family = "self", None
        elif self.device_mode and type(zoo) is ZooLeague:
            opponent, family = "league", (zoo.nmlp, zoo.nlstm)
        else:
            opponent, family = "zoo", "lstm" if getattr(zoo, "recurrent", False) else "mlp"
        reuse = bool(self.reuse_opponent and lstm and not fixed)
        la = rollout_launch(learner, opponent, family, reuse)
        if not self.device_mode:
            return RolloutMode(learner, opponent, zoo, reuse, False, False, None, la, False)
        # the learner's net as the launches are built for it ...
        if lstm:
            sp = m0.spec if type(m0) is LstmPPOModel and m0.spec.nlstm == 128 else None
        else:
            a0 = getattr(m0, "act_model", None)
            sp = a0.spec if type(a0) is PolicyWithValue else None
        # ... and what plays agent 1: its kind, where it may stand, the widths it reads
        grid = lambda: not any(env._gs(g).start % 16 or env._gs(g).stop % 16 for g in range(getattr(env, "groups", 1)))
        if opponent == "self":
            a1 = m1 if lstm else getattr(m1, "act_model", None)
            if lstm:    # an LSTM pool is indexed per 16-env tile of the runner's own envs
                ok = (type(m1) in (LstmPPOModel, LstmOpponentPool) and m1.spec.nlstm == 128
                      and (type(m1) is LstmPPOModel or (m1.num_envs == self.nenv and grid())))
            else:
                ok = type(a1) is PolicyWithValue
            ob1, ac1 = (a1.spec.ob_dim, a1.spec.ac_dim) if ok else (None, None)
        else:
            if opponent == "league":    # dealt over this env set, per tile
                ok = zoo.num_envs == self.nenv and grid()
            else:                       # the recurrent learner's launches index the table per tile, the MLP learner's per env
                ok = type(zoo) in (ZooMLPPolicy, ZooLSTMPolicy) and (family == "mlp" or zoo.emb == zoo.hidden == 64) and (not lstm or grid())
            ok = ok and self.opponent_pool is None
            ob1, ac1 = (zoo.ob_dim, zoo.ac_dim) if ok else (None, None)
        # fits: the nets and their shapes; applies: the launch can play them (with cfrc_mode 'rne_post' a second launch per step fills
        # the force entries); the opt-in is asked of zoo opponents only
        fits = bool(sp is not None and ok and sp.ob_dim == self.ob_dim
                    and (ob1 == self.ob_dim if opponent == "self" else ob1 <= self.ob_dim)
                    and sp.ac_dim == ac1 == env.act_dev.shape[2] and env.obs_dev.stride(2) == 1)
        applies = fits and getattr(env, "cfrc_mode", "zero") == "zero" and hasattr(env, la.entry)
        optin = opponent == "self" or bool(self.fused_fix_opponent)
        fused = bool(applies and optin and self.fused_rollout)
        one_launch = fits and not lstm and opponent == "self"
        if opponent == "league":
            noise_rows = True
        elif opponent == "zoo":
            noise_rows = applies and optin
        else:
            noise_rows = bool(getattr(m0, "accepts_noise", False) and getattr(m1, "accepts_noise", False)) if lstm else one_launch
        return RolloutMode(learner, opponent, zoo, reuse, noise_rows, fused, la.entry if fused else None, la, one_launch)

    def fused_ok(self):
        """The fused rollout launch applies to device mode with two plain MLP policies of the env's own observation / action shape."""
        m = self.rollout_mode()
        return m.fused and (m.learner, m.opponent) == ("mlp", "self")

    def fused_lstm_ok(self):
        """The fused recurrent launch (``sumo_rollout_steps_lstm``) applies to device mode with the nets ``learn(network='lstm')``
        trains on both sides -- an ``LstmPPOModel`` learner against an ``LstmPPOModel`` or an ``LstmOpponentPool`` -- with
        nlstm = 128 and the env's own observation / action shape."""
        m = self.rollout_mode()
        return m.fused and (m.learner, m.opponent) == ("lstm", "self")

    def zoo_opponent(self):
        """The ``ZooMLPPolicy`` or ``ZooLSTMPolicy`` behind ``models[1]`` when the run opted into the fused fix-mode rollout
        (``fused_fix_opponent``) and the launch applies -- device mode, a plain MLP learner of the env's shape, a zoo net of either
        family (an LSTM net: embedding and cell of 64), cfrc_mode 'zero', no opponent pool -- else None.  ``fused_rollout`` is not
        asked: with it off the step-by-step path plays the noise rows the launch would read."""
        m = self.rollout_mode()
        return m.zoo if (m.learner, m.opponent, m.noise_rows) == ("mlp", "zoo", True) else None

    def lstm_zoo_opponent(self):
        """:meth:`zoo_opponent` for a recurrent learner: an ``LstmPPOModel`` with nlstm = 128 of the env's shape, and env groups that
        start and end on multiples of 16 (the launch indexes the table per 16-env tile)."""
        m = self.rollout_mode()
        return m.zoo if (m.learner, m.opponent, m.noise_rows) == ("lstm", "zoo", True) else None

    def league_opponent(self):
        """The :class:`policy_zoo.ZooLeague` behind ``models[1]`` (device mode), else None.  A league always plays on noise rows
        drawn for the whole buffer -- one stream per generator, the learner's and the league's -- with or without the opt-in."""
        m = self.rollout_mode()
        return m.zoo if m.opponent == "league" else None

    def fused_zoo_ok(self):
        """The fused launch against a policy-zoo net (``sumo_rollout_steps_zoo`` / ``sumo_rollout_steps_zoo_lstm``) applies: see
        :meth:`zoo_opponent`."""
        return self.fused_rollout and self.zoo_opponent() is not None

    def fused_lstm_zoo_ok(self):
        """The fused launch of a recurrent learner against a policy-zoo net (``sumo_rollout_steps_lstm_zoo`` /
        ``sumo_rollout_steps_lstm_zoo_lstm``) applies: see :meth:`lstm_zoo_opponent`."""
        return self.fused_rollout and self.lstm_zoo_opponent() is not None

    def fused_league_ok(self):
        """The league plays inside the fused launches: the opt-in (``fused_fix_opponent``), ``fused_rollout``, cfrc_mode 'zero', no
        opponent pool, a plain MLP learner or an ``LstmPPOModel`` with nlstm = 128 of the env's shape, the league dealt over this
        env set, env groups that start and end on multiples of 16.  Otherwise the step-by-step path plays the same noise rows."""
        m = self.rollout_mode()
        return m.fused and m.opponent == "league"

    def fused_steps(self, mode=None):
        """The bound ``steps(B, s0, K, alpha)`` of the current mode's fused launch, or None when no fused launch applies."""
        mode = mode or self.rollout_mode()
        return functools.partial(self._launch_steps, mode) if mode.fused else None

    # ---- device mode ------------------------------------------------------------------------------------------
    def _alloc_device(self, T):
        """Rollout buffers [agent, time, env, ...] in HBM."""
        t = self._t
        N, D, dev = self.nenv, self.ob_dim, self.device
        A = self.env.action_space[0].shape[0]
        f32 = t.float32
        B = dict(T=T, A=A)
        B["obs"] = t.empty((2, T, N, D), dtype=f32, device=dev)
        B["act"] = t.empty((2, T, N, A), dtype=f32, device=dev)
        for k in ("rew", "val", "nlp", "onlp"):
            B[k] = t.empty((2, T, N), dtype=f32, device=dev)
        B["done"] = t.empty((2, T, N), dtype=t.uint8, device=dev)
        B["ep_done"] = t.empty((T, N), dtype=t.uint8, device=dev)
        B["ep_r"] = t.empty((T, N), dtype=t.float64, device=dev)
        B["ep_l"] = t.empty((T, N), dtype=t.int32, device=dev)
        B["scratch_a"] = t.empty((N, A), dtype=f32, device=dev)
        B["scratch_b"] = t.empty((N, A), dtype=f32, device=dev)
        return B

    def _step_device(self, B, s, alpha, env_events=None, mode=None):
        """One rollout step (runner.py:62-151): 4 fused policy launches (the reference's 5 evaluations), env step, reward mix.
        With env groups (``SumoVecEnv(groups=G)``) every group runs this sequence on its own stream: a group's next step only
        waits for that group's envs, not for the slowest env of the whole batch (``join_groups`` before reading the buffers)."""
        mode = mode or self.rollout_mode()
        streams = self._group_streams()
        if streams is None:
            self._step_group(B, s, alpha, None, slice(0, self.nenv), env_events, mode)
            return
        for g, st in enumerate(streams):
            with self._t.cuda.stream(st):
                self._step_group(B, s, alpha, g, self.env._gs(g), env_events if g == 0 else None, mode)

    def _group_streams(self):
        """One stream per env group (None without groups), created at the first use."""
        t = self._t
        G = getattr(self.env, "groups", 1)
        if G > 1 and self._gstreams is None:
            cur = t.cuda.current_stream(self.device)
            self._gstreams = [t.cuda.Stream(device=self.device) for _ in range(G)]
            self._gsides = [None] * G
            for st in self._gstreams:
                st.wait_stream(cur)
        return self._gstreams

    def join_groups(self):
        """Make the current stream wait for every env group's stream (no-op without groups)."""
        if self._gstreams is not None:
            cur = self._t.cuda.current_stream(self.device)
            for st in self._gstreams:
                cur.wait_stream(st)

    def _draw_steps(self, gen, T, n, A):
        """Action noise [T, n, A] as T consecutive [n, A] draws of ``gen``: what ``step`` would draw call by call (so a one-group
        device rollout consumes the generator exactly like the reference-order host rollout)."""
        t = self._t
        buf = t.empty((T, n, A), dtype=t.float32, device=self.device)
        for k in range(T):
            t.randn((n, A), generator=gen, device=self.device, dtype=t.float32, out=buf[k])
        return buf

    def _noise_rows(self, B, s, sl, mode):
        """The action noise pair ([T, n, A] for agent 0, for agent 1) of the group of envs ``sl`` for the whole buffer, drawn when the
        group's first step is written and kept in ``B``: what the fused launch reads and the step-by-step path plays row by row.
        The learner's rows as its family draws them -- MLP: one call on its generator; LSTM: ``_draw_steps`` -- and agent 1's
        likewise in self-play, in one call on the zoo net's / the league's generator otherwise."""
        key = ("noise", sl.start)
        if s == 0 or key not in B:
            t, (m0, m1) = self._t, self.models
            T, n, A = B["T"], sl.stop - sl.start, B["A"]
            once = lambda gen: t.randn((T, n, A), generator=gen, device=self.device, dtype=t.float32)
            own = (lambda m: self._draw_steps(m.gen, T, n, A)) if mode.learner == "lstm" else (lambda m: once(m.act_model.gen))
            B[key] = (own(m0), own(m1) if mode.zoo is None else once(mode.zoo.gen))
        return B[key]

    # ---- the fused launches -----------------------------------------------------------------------------------
    def _opponent_side(self, mode):
        """Agent 1's part of a fused launch: (parameter pointer, selector tensor or None, npool, extra) -- the selector per env for an
        MLP learner and per 16-env tile for a recurrent one; ``extra(sl)`` the struct that follows the launch struct (a zoo table's,
        with the group's state rows where LSTM nets play) or None.  A single zoo net sits in a cached one-row table."""
        lstm, zoo, fam, m1 = mode.learner == "lstm", mode.zoo, mode.launch.family, self.models[1]
        if zoo is None and lstm:
            if hasattr(m1, "tile_net"):
                return m1._nets_dev.data_ptr(), m1.tile_net, m1.capacity, None
            return m1.net_dev().data_ptr(), None, 1, None
        if zoo is None:
            pool = self.opponent_pool
            if pool is not None:
                return pool.params.data_ptr(), pool.index, pool.capacity, None
            return m1.act_model.params.data_ptr(), None, 1, None
        if mode.opponent == "league":
            table = zoo if fam == "league" else zoo.lstm_table if fam == "lstm" else zoo.mlp_table
            sel = None if fam == "league" else zoo.tile_entry if lstm else zoo.env_entry
            npool, state = len(zoo.members), zoo.state
        else:
            if self._zoo_table is None or self._zoo_table[0] is not zoo:
                self._zoo_table = (zoo, (ZooLstmTable if fam == "lstm" else ZooTable)([zoo], zoo.ac_dim, self.device))
            table = self._zoo_table[1]
            sel, npool, state = None, table.capacity, self.zoo_state
        if fam == "mlp":
            zs = table.struct()
            return None, sel, npool, lambda sl: zs
        return None, sel, npool, lambda sl: table.struct(state[sl])

    def _launch_steps(self, mode, B, s0, K, alpha):
        """Rollout steps s0 .. s0+K-1 of every env group, one launch of ``mode.launch`` per group on the group's stream: the five
        evaluations of runner.py:62-96, env.step, the reward curriculum and the appends to ``B`` all happen inside the env engine;
        the recurrent states (``states``, ``shadow_state``, ``zoo_state`` / the league's) are advanced in place.  The launch reads
        the group's ``_noise_rows`` -- the draws of the step-by-step path, hence the same rollout bit for bit."""
        t, env, la, m0 = self._t, self.env, mode.launch, self.models[0]
        lstm = mode.learner == "lstm"
        ro_type, entry = getattr(capi, la.struct), getattr(env, la.entry)
        params, sel, npool, extra = self._opponent_side(mode)
        G = getattr(env, "groups", 1)
        streams = self._group_streams() if G > 1 else [None]
        for g in range(G):
            sl = env._gs(g)
            with (t.cuda.stream(streams[g]) if streams[g] is not None else _nullctx()):
                noise = self._noise_rows(B, s0, sl, mode)
                ro = ro_type()
                if lstm:
                    ro.learner, ro.opponents_dev, ro.state0 = C.addressof(m0._net), params, self.states[0][sl].data_ptr()
                    if mode.opponent == "self":
                        ro.state1 = self.states[1][sl].data_ptr()
                    if mode.reuse:
                        ro.state2 = self.shadow_state[sl].data_ptr()
                    if sel is not None:
                        ro.tile_net_dev = sel.data_ptr()
                else:
                    pi = m0.act_model
                    ro.learner_params, ro.opponent_params, ro.ob_dim, ro.ac_dim = pi.params.data_ptr(), params, pi.spec.ob_dim, pi.spec.ac_dim
                    if sel is not None:
                        ro.opponent_index = sel[sl].data_ptr()
                ro.npool = npool
                ro.T, ro.Ntot, ro.env_offset, ro.s0, ro.K, ro.alpha = B["T"], self.nenv, sl.start, int(s0), int(K), float(alpha)
                ro.noise0, ro.noise1 = noise[0].data_ptr(), noise[1].data_ptr()
                for f in ("obs", "act", "rew", "val", "nlp", "onlp", "done", "ep_done", "ep_r", "ep_l"):
                    setattr(ro, f, B[f].data_ptr())
                entry(g, ro) if extra is None else entry(g, ro, extra(sl))
        self.obs, self.dones = env.obs_dev, env.done_dev

    def _steps_fused(self, B, s0, K, alpha):
        """``_launch_steps`` of MLP self-play (``sumo_rollout_steps``; an ``opponent_pool`` plays through its per-env index)."""
        self._launch_steps(_self_play("mlp"), B, s0, K, alpha)

    def _steps_fused_lstm(self, B, s0, K, alpha, reuse=False):
        """``_launch_steps`` of recurrent self-play (``sumo_rollout_steps_lstm``; ``reuse``: ``sumo_rollout_steps_lstm_reuse``)."""
        self._launch_steps(_self_play("lstm", reuse), B, s0, K, alpha)

    # ---- the step-by-step launches ----------------------------------------------------------------------------
    def _step_group(self, B, s, alpha, g, sl, env_events, mode):
        t = self._t
        env = self.env
        n = sl.stop - sl.start
        ob, dn = env.obs_dev[sl], env.done_dev[sl]                      # [n, 2, D] / [n, 2]: the env's own buffers
        noise = self._noise_rows(B, s, sl, mode) if mode.noise_rows else None
        act = env.act_dev
        if mode.one_launch:                                             # records obs / dones, evaluates, fills env.act_dev
            self._selfplay_forward(B, s, self.models[0].act_model, self.models[1].act_model, ob, dn, sl, noise)
        else:
            B["obs"][:, s, sl].copy_(ob.permute(1, 0, 2))               # one strided copy per array instead of one per agent
            B["done"][:, s, sl].copy_(dn.t())
            self._evaluate_step(B, s, g, sl, dn, mode, noise)
            act[sl].copy_(B["act"][:, s, sl].permute(1, 0, 2))
        if env_events is not None:
            env_events[0].record()
        if g is None:
            env.step_device(act)
        else:
            env.step_device_group(g, act)
        if env_events is not None:
            env_events[1].record()
        st = t.cuda.current_stream(self.device).cuda_stream
        # reward mix (runner.py:134) + the step's episode records, one launch
        ppo_capi.chk(ppo_capi.lib().ppo_post_step(env.info_dev[sl].data_ptr(), n, alpha, B["rew"][0, s, sl].data_ptr(), B["T"] * self.nenv,
                                                  env.done_dev[sl].data_ptr(), env.ep_r_dev[sl].data_ptr(), env.ep_l_dev[sl].data_ptr(),
                                                  B["ep_done"][s, sl].data_ptr(), B["ep_r"][s, sl].data_ptr(),
                                                  B["ep_l"][s, sl].data_ptr(), st))
        self.obs, self.dones = env.obs_dev, env.done_dev

    def _evaluate_step(self, B, s, g, sl, dn, mode, noise):
        """The step's evaluations (runner.py:62-96), always in this order: the learner acts on agent 0, the opponent scores that
        action, the opponent acts on agent 1, the learner scores and values that action -- without ``noise`` (the group's
        ``_noise_rows``) each net draws inside these calls from its own generator.  A scoring call without a state starts from
        zeros, as the reference's calls do; a recurrent net acts from its rows of the state it carries (``states``, ``zoo_state``,
        the league's), masked by its agent's done flags of the previous step, and advances them."""
        PI, VF = ppo_capi.FWD_PI, ppo_capi.FWD_VF
        m0, m1 = self.models
        opp, lstm = m1.act_model, mode.learner == "lstm"
        o0, o1 = B["obs"][0, s, sl], B["obs"][1, s, sl]
        nk0, nk1 = ({}, {}) if noise is None else (dict(noise=noise[0][s]), dict(noise=noise[1][s]))
        zoo_lstm = mode.opponent != "league" and getattr(opp, "recurrent", False) and not (lstm and mode.opponent == "self")
        if not lstm and not zoo_lstm and mode.opponent != "league":
            return self._policy_evals(B, s, m0.act_model, opp, o0, o1, sl, g, nk0, nk1)
        act0, act1 = B["act"][0, s, sl], B["act"][1, s, sl]
        val, nlp, onlp = B["val"][:, s, sl], B["nlp"][:, s, sl], B["onlp"][:, s, sl]
        # the learner acts on agent 0
        if lstm:
            a0, v0, S0, n0 = m0.step(o0, S=self.states[0][sl], M=dn[:, 0], **nk0)
            self.states[0][sl] = S0
            act0.copy_(a0); val[0].copy_(v0); nlp[0].copy_(n0)
        else:
            m0.act_model.evaluate(o0, PI | VF, out=dict(action=act0, neglogp=nlp[0], value=val[0]), **nk0)
        # the opponent scores that action, then acts on agent 1
        if mode.opponent == "league":
            opp.score(o0, act0, sl.start, onlp[0])
            opp.act(o1, dn[:, 1], sl.start, nk1["noise"], act1, onlp[1])
        elif zoo_lstm:
            opp.evaluate(o0, given_action=act0, out=dict(neglogp=onlp[0], action=B["scratch_a"][sl]))
            opp.evaluate(o1, state=self.zoo_state[sl], mask=dn[:, 1], out=dict(action=act1, neglogp=onlp[1]), **nk1)
        elif mode.opponent == "self":
            pk = dict(first_env=sl.start) if hasattr(m1, "tile_net") else {}      # opponent pool: snapshots are indexed per env tile
            onlp[0].copy_(opp.action_probability(o0, given_action=act0, **pk))
            a1, _, S1, on1 = m1.step(o1, S=self.states[1][sl], M=dn[:, 1], **pk, **nk1)
            self.states[1][sl] = S1
            act1.copy_(a1); onlp[1].copy_(on1)
        else:
            opp.evaluate(o0, PI, given_action=act0, out=dict(neglogp=onlp[0], action=B["scratch_a"][sl]))
            opp.evaluate(o1, PI, out=dict(action=act1, neglogp=onlp[1]), **nk1)
        # the learner scores and values agent 1's action
        if not lstm:
            return m0.act_model.evaluate(o1, PI | VF, given_action=act1, out=dict(neglogp=nlp[1], value=val[1], action=B["scratch_b"][sl]))
        if mode.reuse:              # ONE evaluation from the shadow state: its value, its neglogp of the action, the new shadow rows
            v1, n1, S2 = m0.score_value_advance(o1, self.shadow_state[sl], dn[:, 1], act1)
            self.shadow_state[sl] = S2
        elif mode.opponent == "self":   # the value from agent 1's new state, the neglogp from a zero state
            v1, n1 = m0.value(o1, S=S1, M=dn[:, 1]), m0.act_model.action_probability(o1, given_action=act1)
        else:                       # a zoo net's state is not the learner's: both from a zero state, in one evaluation
            v1, n1 = m0.score_and_value(o1, act1)
        val[1].copy_(v1); nlp[1].copy_(n1)

    def _selfplay_forward(self, B, s, learner, opp, ob, dn, sl, noise):
        """runner.py:62-96 in one launch: learner acts on agent 0 (opponent scores it), opponent acts on agent 1 (learner scores
        it and evaluates the value); the kernel also records the observations / done flags and writes the env's action buffer.
        ``noise``: the group's ``_noise_rows`` -- each acting model's own generator, as in ``PolicyWithValue.evaluate``, drawn for
        the whole buffer (two launches per rollout instead of two per step between the env steps)."""
        t = self._t
        n = sl.stop - sl.start
        D, A = learner.spec.ob_dim, learner.spec.ac_dim
        noise0, noise1 = noise[0][s], noise[1][s]
        outs = [B["obs"][0, s, sl], B["obs"][1, s, sl], B["act"][0, s, sl], B["act"][1, s, sl], B["nlp"][0, s, sl], B["nlp"][1, s, sl],
                B["onlp"][0, s, sl], B["onlp"][1, s, sl], B["val"][0, s, sl], B["val"][1, s, sl]]
        fp = (C.c_void_p * 10)(*[x.data_ptr() for x in outs])
        dp = (C.c_void_p * 2)(B["done"][0, s, sl].data_ptr(), B["done"][1, s, sl].data_ptr())
        ppo_capi.chk(ppo_capi.lib().ppo_selfplay_forward(learner.params.data_ptr(), opp.params.data_ptr(), ob.data_ptr(), n, ob.stride(0),
                                                         ob.stride(1), D, A, noise0.data_ptr(), noise1.data_ptr(), dn.data_ptr(),
                                                         self.env.act_dev[sl].data_ptr(), fp, dp,
                                                         t.cuda.current_stream(self.device).cuda_stream))

    def _policy_evals(self, B, s, learner, opp, o0, o1, sl, g, nk0=None, nk1=None):
        """The two chains (learner acts on agent 0's stream and the opponent scores it; the opponent acts on agent 1's stream
        and the learner evaluates it) are independent: they run on two HIP streams and join before the env step.  ``nk0`` /
        ``nk1``: ``dict(noise=rows)`` for the two sampling evaluations (default: each net draws from its own generator)."""
        t = self._t
        PI, VF = ppo_capi.FWD_PI, ppo_capi.FWD_VF
        nk0, nk1 = nk0 or {}, nk1 or {}
        sa, sb = B["scratch_a"][sl], B["scratch_b"][sl]
        if g is not None:
            # env groups already overlap with each other; more streams than hardware queues (4 by default) only serialise
            learner.evaluate(o0, PI | VF, out=dict(action=B["act"][0, s, sl], neglogp=B["nlp"][0, s, sl], value=B["val"][0, s, sl]), **nk0)
            opp.evaluate(o0, PI, given_action=B["act"][0, s, sl], out=dict(neglogp=B["onlp"][0, s, sl], action=sa))
            opp.evaluate(o1, PI, out=dict(action=B["act"][1, s, sl], neglogp=B["onlp"][1, s, sl]), **nk1)
            learner.evaluate(o1, PI | VF, given_action=B["act"][1, s, sl],
                             out=dict(neglogp=B["nlp"][1, s, sl], value=B["val"][1, s, sl], action=sb))
            return
        cur = t.cuda.current_stream(self.device)
        if self._side is None:
            self._side = t.cuda.Stream(device=self.device)
        side = self._side
        side.wait_stream(cur)
        # agent 0 acts with the learner; the opponent net scores that action (runner.py:67-85)
        learner.evaluate(o0, PI | VF, out=dict(action=B["act"][0, s, sl], neglogp=B["nlp"][0, s, sl], value=B["val"][0, s, sl]), **nk0)
        opp.evaluate(o0, PI, given_action=B["act"][0, s, sl], out=dict(neglogp=B["onlp"][0, s, sl], action=sa))
        with t.cuda.stream(side):
            # agent 1 acts with the opponent; the learner net evaluates value and neglogp there (runner.py:86-96)
            opp.evaluate(o1, PI, out=dict(action=B["act"][1, s, sl], neglogp=B["onlp"][1, s, sl]), **nk1)
            learner.evaluate(o1, PI | VF, given_action=B["act"][1, s, sl],
                             out=dict(neglogp=B["nlp"][1, s, sl], value=B["val"][1, s, sl], action=sb))
        cur.wait_stream(side)

    def _run_device(self, update):
        t = self._t
        T, N = self.nsteps, self.nenv
        B = self._alloc_device(T)
        alpha = anneal_alpha(update, self.anneal_bound)
        mode = self.rollout_mode()
        lstm, m0 = mode.learner == "lstm", self.models[0]
        states0 = self.states[0].clone() if lstm else None               # BPTT starts from the rollout's initial state
        if self.reuse_opponent and not mode.reuse:
            raise NotImplementedError(REUSE_REFUSED)
        if mode.reuse:
            self.shadow_state0 = self.shadow_state.clone()               # ... and agent 1's sequences from the shadow state's
        if self._gstreams is not None:                                   # the group streams see the parameter update that preceded this rollout
            cur = t.cuda.current_stream(self.device)
            for st in self._gstreams:
                st.wait_stream(cur)
        steps = self.fused_steps(mode)
        if steps is not None:
            chunk = self.rollout_chunk if self.rollout_chunk > 0 else T
            for s0 in range(0, T, chunk):
                steps(B, s0, min(chunk, T - s0), alpha)
        else:
            if self.opponent_pool is not None:
                raise NotImplementedError("a per-env opponent pool needs the fused rollout path (MLP policies, SUMO_FUSED_ROLLOUT != 0)")
            for s in range(T):
                self._step_device(B, s, alpha, mode=mode)
        self.join_groups()
        last_values = t.empty((2, N), dtype=t.float32, device=self.device)
        if not lstm:
            m0.act_model.evaluate(self.obs[:, 0, :], ppo_capi.FWD_VF, out=dict(value=last_values[0]))   # runner.py:184: always models[0]
            m0.act_model.evaluate(self.obs[:, 1, :], ppo_capi.FWD_VF, out=dict(value=last_values[1]))
        else:
            last_values[0].copy_(m0.value(self.obs[:, 0, :], S=self.states[0], M=self.dones[:, 0]))
            if mode.opponent == "self":     # from the state the learner's values of agent 1 ran on: the opponent's, or the shadow state
                S1 = self.shadow_state if mode.reuse else self.states[1]
                last_values[1].copy_(m0.value(self.obs[:, 1, :], S=S1, M=self.dones[:, 1]))
            else:                           # a zoo net carries no state of the learner's (``_evaluate_step``): from a zero state
                last_values[1].copy_(m0.value(self.obs[:, 1, :]))
        returns, opr, oer, ratio = self._vtrace(B["rew"], B["val"], B["nlp"], B["onlp"], B["done"], self.dones.contiguous(), last_values)
        # A fused launch that was cut short (expired hand-over wait, hand-over tag / checksum mismatch) leaves unwritten rollout rows:
        # fail as loudly as a MuJoCo fault does in the reference (mujoco-py builder.py:351-369 raises out of env.step) instead of
        # training on them.  The call waits for the launch; this function synchronises right below anyway.
        if steps is not None:
            for E in self.env.engines:
                E.rollout_status()
        # episode infos of agent 0 (monitor.py:63-78), harvested with one host sync per rollout
        d = B["ep_done"].cpu().numpy().astype(bool)
        rr, ll = B["ep_r"].cpu().numpy(), B["ep_l"].cpu().numpy()
        epinfos = EpInfoList(rr[d], ll[d])          # (step, env) order of np.nonzero, dicts built on demand
        if mode.opponent == "league":               # per member: episodes, learner wins, losses, draws (policy_zoo.league_scores)
            self.league_scores = league_scores(d, rr, ll, mode.zoo.tile_member, len(mode.zoo.members),
                                               getattr(getattr(self.env, "model", None), "timestep_limit", 500))
        return (sf01(B["obs"]), sf01(returns), sf01(B["done"].bool()), sf01(B["act"]), sf01(B["val"]), sf01(B["nlp"]), sf01(B["rew"]),
                sf01(B["onlp"]), sf01(B["obs"][1]), sf01(B["act"][1]), states0, epinfos, sf0(opr), sf0(oer), sf0(ratio))

    # ---- host mode ----------------------------------------------------------------------------------------------
    def _run_host(self, update):
        t = self._t
        T, N, A_ = self.nsteps, self.nenv, self.nagent
        mb_obs = [[] for _ in range(A_)]
        mb_actions = [[] for _ in range(A_)]
        mb_values = [[] for _ in range(A_)]
        mb_dones = [[] for _ in range(A_)]
        mb_nlp = [[] for _ in range(A_)]
        mb_onlp = [[] for _ in range(A_)]
        opp_obs, opp_act, epinfos = [], [], []
        info_steps, env_rew_steps = [], []
        use_info = None
        # recurrent nets: the state at the START of the rollout is what back-propagation through time begins from (the
        # reference returns the list slot after the loop, i.e. the final state -- its recurrent training path is dead code)
        mb_states0 = None if self.states[0] is None else np.array(self.states[0], copy=True)
        for _ in range(T):
            acts = []
            for agt in range(A_):
                o = self.obs[:, agt, :]
                a, v, self.states[agt], nlp = self.models[agt].step(o, S=self.states[agt], M=self.dones[:, agt])
                mb_obs[agt].append(o.copy())
                mb_actions[agt].append(a)
                mb_dones[agt].append(self.dones[:, agt])
                if agt == 0:
                    mb_values[0].append(v)
                    mb_nlp[0].append(nlp)
                    mb_onlp[0].append(self.models[1].act_model.action_probability(o, given_action=a))
                else:
                    mb_onlp[agt].append(nlp)
                    mb_values[agt].append(self.models[0].value(o, S=self.states[agt], M=self.dones[:, agt]))
                    mb_nlp[agt].append(self.models[0].act_model.action_probability(o, given_action=a))
                    opp_obs.append(self.obs[:, 1, :].copy())
                    opp_act.append(a)
                acts.append(a)
            self.obs[:], rewards, self.dones, infos = self.env.step(np.stack(acts, axis=1))
            if use_info is None:
                use_info = "shaping_reward" in infos[0][0]                # runner.py:127
            if use_info:
                arr = np.zeros((N, 2, 8))
                for e in range(N):
                    for agt in range(A_):
                        arr[e, agt, 6] = infos[e][agt]["shaping_reward"]
                        arr[e, agt, 3] = infos[e][agt]["main_reward"]
                info_steps.append(arr)
            else:
                env_rew_steps.append(np.asarray(rewards))
            for e in range(N):
                ep = infos[e][0].get("episode")
                if ep:
                    epinfos.append(ep)
        dev, f32 = self.device, t.float32
        up = lambda x, dt=np.float32: t.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=dt))).to(dev)
        mb_obs = np.asarray(mb_obs, dtype=self.obs.dtype)
        mb_actions = np.asarray(mb_actions)
        opp_obs = np.asarray(opp_obs, dtype=self.obs.dtype)
        opp_act = np.asarray(opp_act)
        mb_dones_np = np.asarray(mb_dones, dtype=bool)
        rew = t.empty((2, T, N), dtype=f32, device=dev)
        if use_info:
            alpha = anneal_alpha(update, self.anneal_bound)
            st = t.cuda.current_stream(dev).cuda_stream
            info_dev = up(np.stack(info_steps), np.float64)               # [T, N, 2, 8]
            for s in range(T):
                ppo_capi.chk(ppo_capi.lib().ppo_reward_mix(info_dev[s].data_ptr(), N, alpha, rew[0, s].data_ptr(), T * N, st))
        else:
            rew.copy_(up(np.stack(env_rew_steps).transpose(2, 0, 1)))    # runner.py:146: rewards[:, agt], cast to float32
        val, nlp, onlp = up(mb_values), up(mb_nlp), up(mb_onlp)
        last_values = up(np.stack([self.models[0].value(self.obs[:, agt, :], S=self.states[agt], M=self.dones[:, agt])
                                   for agt in range(A_)]))
        returns, opr, oer, ratio = self._vtrace(rew, val, nlp, onlp, up(mb_dones_np, np.uint8), up(self.dones, np.uint8),
                                                last_values)
        n = lambda x: x.cpu().numpy()
        mb_onlp_np = np.asarray(mb_onlp)
        return (*map(sf01, (mb_obs, n(returns), mb_dones_np, mb_actions, np.asarray(mb_values, np.float32),
                            np.asarray(mb_nlp, np.float32), n(rew), mb_onlp_np, opp_obs, opp_act)),
                mb_states0, epinfos, *map(lambda x: sf0(n(x)), (opr, oer, ratio)))
