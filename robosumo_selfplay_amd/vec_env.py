"""Device-resident drop-in for the reference's ``SubprocVecEnv`` of RoboSumo envs.

Interface mirrored (same names, argument meaning, error behaviour):
  * baselines ``VecEnv`` contract  -- reference baselines/baselines/common/vec_env/vec_env.py:29-138
  * concrete behaviour             -- reference subproc_vec_env.py:35-116 (auto-reset on done[0], stacked
    observations ``[N, 2, D]``, ``infos`` = tuple over envs of tuple over agents of dicts)
  * what each "worker" wrapped     -- reference run.py:73-83: gym env -> SumoEnv wrapper (sumo_env.py) -> Monitor
    (baselines/baselines/bench/monitor.py:51-78)

One ``SumoVecEnv`` owns one GPU's shard of environments; all N envs advance in a single kernel launch
(csrc/sumo_engine.hip).  ``step_async``/``step_wait`` return numpy arrays like the reference; ``step_device`` keeps
everything in HBM for the device-side Runner.
"""
import time

import numpy as np

from . import capi, mjcf
from .spaces import Box, Tuple

_INFO_KEYS = ("ctrl_reward", "lose_penalty", "win_reward", "main_reward", "move_to_opp_reward", "push_opp_reward",
              "shaping_reward")


class VecEnv(object):
    """Subset of the baselines VecEnv ABC used by the hot path."""
    closed = False
    viewer = None
    metadata = {"render.modes": ["human", "rgb_array"]}

    def __init__(self, num_envs, observation_space, action_space):
        self.num_envs = num_envs
        self.observation_space = observation_space
        self.action_space = action_space

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def close_extras(self):
        pass

    def close(self):
        if self.closed:
            return
        self.close_extras()
        self.closed = True

    @property
    def unwrapped(self):
        return self

    def render(self, mode="human"):
        raise NotImplementedError("rendering is outside the hot path (SURVEY.md §2.4)")

    def get_images(self):
        raise NotImplementedError


class EnvSpec(object):
    def __init__(self, env_id):
        self.id = env_id


class SumoVecEnv(VecEnv):
    def __init__(self, env_id="RoboSumo-Ant-vs-Ant-v0", num_envs=1, seed=0, device=0, asset_dir=None, model=None, groups=1,
                 cfrc_mode="zero", adjust_z=0.0):
        """``groups`` > 1 splits the envs into that many equal, contiguous groups, each with its own engine: a group's step is
        its own kernel launch (``step_device_group``), so a caller that advances the groups on separate streams is not held
        back by the slowest env of the whole batch at every step (the device-mode Runner does that).  All buffers stay
        unified ``[N, ...]`` tensors; ``step_device`` / the host API step every group."""
        import torch
        if not torch.cuda.is_available():
            raise capi.SumoHipError("SumoVecEnv needs a HIP device (there is no CPU fallback in the product path)")
        self._torch = torch
        self.model = model if model is not None else mjcf.load_model(env_id, asset_dir)
        self.device = torch.device("cuda", int(device))
        groups = int(groups)
        if groups < 1 or num_envs % groups:
            raise ValueError("num_envs %d is not divisible into %d groups" % (num_envs, groups))
        self.groups, self.group_size = groups, num_envs // groups
        self.engines = [capi.Engine(self.model, self.group_size, device=int(device)) for _ in range(groups)]
        # 'zero' = the reference's observations (its MuJoCo 2.1 scenes carry no force sensor: cfrc_ext == 0); 'rne_post' fills the contact-force
        # entries as a sensor-equipped MuJoCo would (second launch per step, no fused rollout; include/sumo_hip.h: cfrc_mode)
        if cfrc_mode not in ("zero", "rne_post"):
            raise ValueError("cfrc_mode must be 'zero' or 'rne_post'")
        self.cfrc_mode = cfrc_mode
        if cfrc_mode != "zero":
            for E_ in self.engines:
                E_.set_cfrc_mode(cfrc_mode)
        # Agent._adjust_z (agents.py:33,155-161): offset of the z an agent REPORTS (observations, lose test).  0 = training
        # (run.py:76-77); the reference's evaluation / play scripts set -0.5 (eval_robosumo_against_fix.py:108-115)
        self.adjust_z = float(adjust_z)
        if self.adjust_z != 0.0:
            for E_ in self.engines:
                E_.set_adjust_z(self.adjust_z)
        self.engine = self.engines[0]                                   # dimensions / limits (identical for every group)
        E = self.engine
        obs_dims, act_dims = self.model.obs_dims, self.model.act_dims
        ob_spaces = [Box(-np.inf * np.ones(d), np.inf * np.ones(d)) for d in obs_dims]           # agents.py:85-90
        lo = self.model.actuator_ctrlrange[:, 0]
        hi = self.model.actuator_ctrlrange[:, 1]
        ac_spaces = []
        for a in range(2):                                                                        # agents.py:92-115
            u0, nu = int(self.model.agent_uadr[a]), int(self.model.agent_nu[a])
            ac_spaces.append(Box(lo[u0:u0 + nu], hi[u0:u0 + nu]))
        VecEnv.__init__(self, int(num_envs), Tuple(ob_spaces), Tuple(ac_spaces))
        self.spec = EnvSpec(mjcf.canonical_id(env_id))
        self.agents = list(self.model.body_names[int(b)].split("/")[0] for b in self.model.agent_torso)
        self.seeds = (np.uint64(seed) + np.arange(num_envs, dtype=np.uint64))                     # run.py:144 (seed + i)
        N = self.num_envs
        f32, f64 = torch.float32, torch.float64
        self.obs_dev = torch.zeros((N, 2, E.obs_stride), dtype=f32, device=self.device)
        self.act_dev = torch.zeros((N, 2, E.act_stride), dtype=f32, device=self.device)
        self.info_dev = torch.zeros((N, 2, capi.INFO_STRIDE), dtype=f64, device=self.device)
        self.done_dev = torch.zeros((N, 2), dtype=torch.uint8, device=self.device)
        self.ep_r_dev = torch.zeros(N, dtype=f64, device=self.device)
        self.ep_dr_dev = torch.zeros(N, dtype=f64, device=self.device)
        self.ep_l_dev = torch.zeros(N, dtype=torch.int32, device=self.device)
        self.waiting = False
        self.tstart = time.time()
        self._needs_seed = True
        self._same_dims = obs_dims[0] == obs_dims[1] and act_dims[0] == act_dims[1]

    # ---- device-side API -----------------------------------------------------------------------------------
    def _stream(self):
        return self._torch.cuda.current_stream(self.device).cuda_stream

    def _gs(self, g):
        return slice(g * self.group_size, (g + 1) * self.group_size)

    def reset_device(self):
        self._assert_not_closed()
        for g, E in enumerate(self.engines):
            sl = self._gs(g)
            E.reset(self.obs_dev[sl].data_ptr(), seeds=self.seeds[sl] if self._needs_seed else None, stream=self._stream())
        self._needs_seed = False
        return self.obs_dev

    def env_ptrs(self, g, actions=None):
        """The seven env-side pointers of group ``g`` in the order ``sumo_step`` and the fused launches take them: its rows of the
        action tensor (``actions``, default the env's own action buffer), obs, info, done, ep_r, ep_dr, ep_l."""
        sl = self._gs(g)
        bufs = (self.act_dev if actions is None else actions, self.obs_dev, self.info_dev, self.done_dev, self.ep_r_dev, self.ep_dr_dev,
                self.ep_l_dev)
        return tuple(b[sl].data_ptr() for b in bufs)

    def step_device_group(self, g, actions):
        """Advance group ``g`` only (its slice of every buffer), on the current stream.  ``actions`` is the FULL [N, 2, A]
        action tensor; the group's rows are read."""
        self.engines[g].step(*self.env_ptrs(g, actions), stream=self._stream())

    def rollout_steps_group(self, g, ro):
        """K fused self-play rollout steps of group ``g`` on the current stream (``capi.Engine.rollout_steps``): policies, env
        steps and the appends to the rollout buffers in one launch.  ``ro`` is a ``capi.Rollout`` whose ``env_offset`` is the
        group's first env."""
        self.engines[g].rollout_steps(ro, *self.env_ptrs(g), stream=self._stream())

    def rollout_steps_lstm_group(self, g, ro):
        """The same for recurrent policies (``capi.Engine.rollout_steps_lstm``, ``ro`` a ``capi.RolloutLstm``)."""
        self.engines[g].rollout_steps_lstm(ro, *self.env_ptrs(g), stream=self._stream())

    def rollout_steps_lstm_reuse_group(self, g, ro):
        """The recurrent launch under opponent-data reuse (``capi.Engine.rollout_steps_lstm_reuse``, ``ro`` a
        ``capi.RolloutLstmReuse``)."""
        self.engines[g].rollout_steps_lstm_reuse(ro, *self.env_ptrs(g), stream=self._stream())

    def rollout_steps_zoo_group(self, g, ro, zoo):
        """The same against policy-zoo MLP nets (``capi.Engine.rollout_steps_zoo``, ``zoo`` a ``capi.ZooMlp``)."""
        self.engines[g].rollout_steps_zoo(ro, zoo, *self.env_ptrs(g), stream=self._stream())

    def rollout_steps_zoo_lstm_group(self, g, ro, zoo):
        """The same against policy-zoo LSTM nets (``capi.Engine.rollout_steps_zoo_lstm``, ``zoo`` a ``capi.ZooLstm`` whose
        ``state`` holds agent 1's rows of the group's envs)."""
        self.engines[g].rollout_steps_zoo_lstm(ro, zoo, *self.env_ptrs(g), stream=self._stream())

    def rollout_steps_lstm_zoo_group(self, g, ro, zoo):
        """The recurrent launch against policy-zoo MLP nets (``capi.Engine.rollout_steps_lstm_zoo``, ``ro`` a ``capi.RolloutLstm``,
        ``zoo`` a ``capi.ZooMlp``)."""
        self.engines[g].rollout_steps_lstm_zoo(ro, zoo, *self.env_ptrs(g), stream=self._stream())

    def rollout_steps_lstm_zoo_lstm_group(self, g, ro, zoo):
        """The recurrent launch against policy-zoo LSTM nets (``capi.Engine.rollout_steps_lstm_zoo_lstm``, ``zoo`` a
        ``capi.ZooLstm`` whose ``state`` holds agent 1's rows of the group's envs)."""
        self.engines[g].rollout_steps_lstm_zoo_lstm(ro, zoo, *self.env_ptrs(g), stream=self._stream())

    def rollout_steps_zoo_league_group(self, g, ro, league):
        """The MLP learner's launch against a league of policy-zoo nets of both families (``capi.Engine.rollout_steps_zoo_league``,
        ``league`` a ``capi.ZooLeague`` whose LSTM table's ``state`` holds agent 1's rows of the group's envs)."""
        self.engines[g].rollout_steps_zoo_league(ro, league, *self.env_ptrs(g), stream=self._stream())

    def rollout_steps_lstm_zoo_league_group(self, g, ro, league):
        """The recurrent learner's launch against such a league (``capi.Engine.rollout_steps_lstm_zoo_league``, ``ro`` a
        ``capi.RolloutLstm``)."""
        self.engines[g].rollout_steps_lstm_zoo_league(ro, league, *self.env_ptrs(g), stream=self._stream())

    def rollout_steps_pair_group(self, g, ro):
        """K fused co-training steps of group ``g`` of a mixed match-up on the current stream (``capi.Engine.rollout_steps_pair``,
        ``ro`` a ``capi.RolloutPair`` whose ``env_offset`` is the group's first env)."""
        self.engines[g].rollout_steps_pair(ro, *self.env_ptrs(g), stream=self._stream())

    def step_device(self, actions):
        """actions: float32 CUDA tensor [N, 2, act_stride]. Returns (obs, info, done, ep_r, ep_dr, ep_l) tensors that
        are overwritten by the next call."""
        self._assert_not_closed()
        if actions.dtype != self._torch.float32 or not actions.is_cuda or not actions.is_contiguous() \
                or tuple(actions.shape) != tuple(self.act_dev.shape):
            raise ValueError("actions must be a contiguous float32 CUDA tensor of shape %s" % (tuple(self.act_dev.shape),))
        for g in range(self.groups):
            self.step_device_group(g, actions)
        return self.obs_dev, self.info_dev, self.done_dev, self.ep_r_dev, self.ep_dr_dev, self.ep_l_dev

    def set_adjust_z(self, adjust_z):
        """Counterpart of ``for agent in env.agents: agent._adjust_z = v`` (eval_robosumo_against_fix.py:110-112)."""
        self._assert_not_closed()
        self.adjust_z = float(adjust_z)
        for E_ in self.engines:
            E_.set_adjust_z(self.adjust_z)

    # ---- snapshots ---------------------------------------------------------------------------------------------------
    _SNAP_BUFFERS = ("obs_dev", "act_dev", "info_dev", "done_dev", "ep_r_dev", "ep_dr_dev", "ep_l_dev")

    def snapshot(self):
        """The whole env set as a dict: one engine blob per group (``capi.Engine.snapshot``), clones of the seven step buffers, the
        seeds and whether the next reset still uploads them, ``adjust_z`` / ``cfrc_mode``, and what :meth:`restore` checks (env id,
        ``num_envs``, ``groups``).  Synchronises.  A later :meth:`restore` -- on this env or on a freshly built one of the same shape --
        makes every following step, fused rollout launch and reset return what it returned after the snapshot, bit for bit."""
        self._assert_not_closed()
        self._torch.cuda.synchronize(self.device)
        snap = dict(env_id=self.spec.id, num_envs=int(self.num_envs), groups=int(self.groups), adjust_z=float(self.adjust_z),
                    cfrc_mode=self.cfrc_mode, seeds=np.array(self.seeds, copy=True), _needs_seed=bool(self._needs_seed),
                    blobs=[E.snapshot() for E in self.engines])
        for k in self._SNAP_BUFFERS:
            snap[k] = getattr(self, k).clone()
        return snap

    def restore(self, snap):
        """Put a :meth:`snapshot` back (its tensors may live on the host).  Another env id, ``num_envs`` or ``groups`` is refused here,
        another ``cfrc_mode`` or a damaged blob by the engine, which checks a blob before it writes anything; with several groups the groups
        already loaded are put back to what they held when a later group's blob is refused.  The engines' fault counters (:meth:`stats`) are not part of a snapshot."""
        self._assert_not_closed()
        for k, mine in (("env_id", self.spec.id), ("num_envs", int(self.num_envs)), ("groups", int(self.groups))):
            if snap[k] != mine:
                raise ValueError("snapshot of an env with %s=%r cannot be restored into one with %s=%r" % (k, snap[k], k, mine))
        if snap["cfrc_mode"] != self.cfrc_mode:
            raise ValueError("snapshot of an env with cfrc_mode=%r cannot be restored into one with cfrc_mode=%r" % (snap["cfrc_mode"], self.cfrc_mode))
        if len(snap["blobs"]) != len(self.engines):
            raise ValueError("snapshot holds %d engine blobs, this env has %d groups" % (len(snap["blobs"]), len(self.engines)))
        self._torch.cuda.synchronize(self.device)
        done = []
        try:
            for E, blob in zip(self.engines, snap["blobs"]):
                before = E.snapshot() if len(self.engines) > 1 else None      # several groups: a later group's refusal undoes the earlier ones
                E.restore(blob)
                done.append((E, before))
        except Exception:
            for E, before in done:
                E.restore(before)
            raise
        for k in self._SNAP_BUFFERS:
            getattr(self, k).copy_(snap[k])
        self.seeds = np.array(snap["seeds"], dtype=np.uint64, copy=True)
        self._needs_seed = bool(snap["_needs_seed"])
        self.adjust_z = float(snap["adjust_z"])
        self._torch.cuda.synchronize(self.device)

    def stats(self):
        """Solver / contact statistics summed over the groups' engines (maxima for the ``max_*`` entries)."""
        out = None
        for E in self.engines:
            st = E.stats()
            if out is None:
                out = dict(st)
            else:
                for k, v in st.items():
                    out[k] = max(out[k], v) if k.startswith("max_") else out[k] + v
        return out

    # ---- reference (host) API ------------------------------------------------------------------------------------
    def _obs_host(self):
        o = self.obs_dev.cpu().numpy()
        if self._same_dims:
            return o[:, :, :self.model.obs_dims[0]].copy()
        # heterogeneous match-ups: the reference's np.stack of ragged tuples yields an object array
        out = np.empty((self.num_envs, 2), dtype=object)
        for e in range(self.num_envs):
            for a in range(2):
                out[e, a] = o[e, a, :self.model.obs_dims[a]].copy()
        return out

    def reset(self):
        self._assert_not_closed()
        self.reset_device()
        return self._obs_host()

    def step_async(self, actions):
        self._assert_not_closed()
        a = np.zeros(tuple(self.act_dev.shape), np.float32)
        for e in range(self.num_envs) if not self._same_dims else ():
            for g in range(2):
                a[e, g, :self.model.act_dims[g]] = np.asarray(actions[e][g], np.float32)
        if self._same_dims:
            act = np.asarray(actions, dtype=np.float32)
            if act.shape != a.shape:
                raise ValueError("actions must have shape %s, got %s" % (a.shape, act.shape))
            a = act
        self.act_dev.copy_(self._torch.from_numpy(np.ascontiguousarray(a)))
        self.step_device(self.act_dev)
        self.waiting = True

    def step_wait(self):
        self._assert_not_closed()
        self.waiting = False
        info = self.info_dev.cpu().numpy()
        done = self.done_dev.cpu().numpy().astype(bool)
        ep_r, ep_l = self.ep_r_dev.cpu().numpy(), self.ep_l_dev.cpu().numpy()
        obs = self._obs_host()
        rews = info[:, :, 3] + info[:, :, 6]                                      # sumo.py:186
        now = round(time.time() - self.tstart, 6)
        infos = []
        for e in range(self.num_envs):
            per_agent = []
            for g in range(2):
                d = {k: float(info[e, g, i]) for i, k in enumerate(_INFO_KEYS)}
                flags = int(info[e, g, 7])
                if flags & 1:
                    d["winner"] = True                                             # sumo.py:159
                if flags & 2:
                    d["timeout"] = True                                            # sumo_env.py:62-65
                if flags & 4:
                    d["diverged"] = True       # bad-value guard (include/sumo_hip.h): the reference raises MujocoException there
                per_agent.append(d)
            if done[e, 0]:                                                         # monitor.py:63-78 (agent 0 only)
                per_agent[0]["episode"] = {"r": round(float(ep_r[e]), 6), "l": int(ep_l[e]), "t": now}
            infos.append(tuple(per_agent))
        return obs, rews, done, tuple(infos)

    # ---- pictures ------------------------------------------------------------------------------------------------
    def get_images(self, envs=None, width=320, height=240, camera="arena"):
        """RGB images uint8 [k][H][W][3] (host) of the chosen envs, default the first min(N, 16), rendered on the GPU from each
        group's ``get_state()`` qpos (render.py).  ``camera``: 'arena' (one fixed view), 'track' (follows the two torsos, one camera
        per env) or a ``render.Camera``.  The renderer is created on first use."""
        from . import render
        if getattr(self, "_renderer", None) is None:
            self._renderer = render.Renderer(self.model, device=self.device.index or 0)
        self._assert_not_closed()
        envs = np.arange(min(self.num_envs, 16)) if envs is None else np.atleast_1d(np.asarray(envs, np.int64))
        if envs.size == 0 or envs.min() < 0 or envs.max() >= self.num_envs:
            raise ValueError("envs must name some of the %d envs" % self.num_envs)
        self._torch.cuda.synchronize(self.device)
        qpos = np.concatenate([E.get_state()[0] for E in self.engines])[envs]
        if camera == "arena":
            cams = render.arena_camera()
        elif camera == "track":
            cams = render.track_camera(self.model, qpos)
        elif isinstance(camera, render.Camera):
            cams = camera
        else:
            raise ValueError("camera must be 'arena', 'track' or a render.Camera")
        return self._renderer.frames(qpos, cams, width, height)["rgb"].cpu().numpy()

    def render(self, mode="rgb_array", **kw):
        """``mode='rgb_array'``: the images of :meth:`get_images` (its keywords) tiled into one picture, as baselines'
        ``VecEnv.render`` returns it.  There is no window: ``mode='human'`` is not implemented."""
        if mode == "rgb_array":
            from . import render
            return render.tile_images(self.get_images(**kw))
        if mode == "human":
            raise NotImplementedError("render(mode='human'): there is no display path; use mode='rgb_array' or play.py")
        raise NotImplementedError("unknown render mode %r" % (mode,))

    def close_extras(self):
        if getattr(self, "_renderer", None) is not None:
            self._renderer.close()
            self._renderer = None
        for E in self.engines:
            E.close()

    def _assert_not_closed(self):
        assert not self.closed, "Trying to operate on a SumoVecEnv after calling close()"

    def __del__(self):
        if not self.closed:
            try:
                self.close()
            except Exception:
                pass


def make_vec_env(env_id, num_env, seed, device=0, **kw):
    """Counterpart of reference run.py:124-146 ``build_env``: ``num_env`` envs seeded ``seed + i``."""
    return SumoVecEnv(env_id, num_envs=num_env, seed=seed, device=device, **kw)
