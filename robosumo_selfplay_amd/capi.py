"""ctypes binding of the engine's C ABI (include/sumo_hip.h -> csrc/libsumo_hip.so).

This is the stub a maintainer of the reference would drop in next to subproc_vec_env.py.
There is NO CPU fallback: if the library is missing or no GPU is visible, construction raises.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

INFO_STRIDE = 8
NDIMS = 16
NSTATS = 13
_LIB = None


class SumoHipError(RuntimeError):
    pass


_I, _P = C.c_int, C.c_void_p
# the field tails the MLP and the LSTM struct of a launch share (include/sumo_hip.h)
_ROLLOUT_TAIL = [("T", _I), ("Ntot", _I), ("env_offset", _I), ("s0", _I), ("K", _I), ("alpha", C.c_double), ("noise0", _P), ("noise1", _P),
                 ("obs", _P), ("act", _P), ("rew", _P), ("val", _P), ("nlp", _P), ("onlp", _P),
                 ("done", _P), ("ep_done", _P), ("ep_r", _P), ("ep_l", _P)]
_MATCH_TAIL = [("T", _I), ("s0", _I), ("K", _I), ("quota", _I), ("noise0", _P), ("noise1", _P), ("score", _P)]


class Rollout(C.Structure):
    """``sumo_rollout`` of include/sumo_hip.h (device pointers as integers)."""
    _fields_ = [("learner_params", _P), ("opponent_params", _P), ("opponent_index", _P),
                ("npool", _I), ("ob_dim", _I), ("ac_dim", _I)] + _ROLLOUT_TAIL


class RolloutLstm(C.Structure):
    """``sumo_rollout_lstm`` of include/sumo_hip.h (``learner``: pointer to a host ``ppo_capi.LstmNet``; the rest device pointers)."""
    _fields_ = [("learner", _P), ("opponents_dev", _P), ("tile_net_dev", _P), ("npool", _I), ("state0", _P), ("state1", _P)] + _ROLLOUT_TAIL


class RolloutLstmReuse(C.Structure):
    """``sumo_rollout_lstm_reuse`` of include/sumo_hip.h: the fields of :class:`RolloutLstm` (the header nests that struct: same
    layout) and ``state2``, the learner's shadow state along agent 1's stream."""
    _fields_ = RolloutLstm._fields_ + [("state2", _P)]


class Match(C.Structure):
    """``sumo_match`` of include/sumo_hip.h (device pointers as integers)."""
    _fields_ = [("params", _P), ("idx0", _P), ("idx1", _P), ("nsnap", _I), ("ob_dim", _I), ("ac_dim", _I)] + _MATCH_TAIL


class MatchLstm(C.Structure):
    """``sumo_match_lstm`` of include/sumo_hip.h (``proto`` a host pointer to a ``ppo_capi.LstmNet``, the rest device pointers)."""
    _fields_ = [("proto", _P), ("nets_dev", _P), ("idx0", _P), ("idx1", _P), ("nsnap", _I), ("state0", _P), ("state1", _P)] + _MATCH_TAIL


class MatchCross(C.Structure):
    """``sumo_match_cross`` of include/sumo_hip.h: an MLP(64,64) table and an LSTM(128) table, one per agent (``proto`` a host pointer
    to a ``ppo_capi.LstmNet``, the rest device pointers; ``lstm_side``: the agent the LSTM table plays)."""
    _fields_ = [("params", _P), ("nsnap_mlp", _I), ("ob_dim", _I), ("ac_dim", _I), ("proto", _P), ("nets_dev", _P), ("nsnap_lstm", _I),
                ("state", _P), ("lstm_side", _I), ("idx0", _P), ("idx1", _P)] + _MATCH_TAIL


class ZooMlp(C.Structure):
    """``sumo_zoo_mlp`` of include/sumo_hip.h: a device table of frozen policy-zoo MLP nets (device pointers as integers)."""
    _fields_ = [("params", _P), ("filt", _P), ("obs_clip", C.c_float), ("nzoo", _I), ("ob_dim", _I)]


class ZooLstm(C.Structure):
    """``sumo_zoo_lstm`` of include/sumo_hip.h: a device table of frozen policy-zoo LSTM nets plus agent 1's recurrent state of the
    launch's envs (device pointers as integers)."""
    _fields_ = [("params", _P), ("filt", _P), ("state", _P), ("obs_clip", C.c_float), ("forget_bias", C.c_float), ("nzoo", _I),
                ("ob_dim", _I), ("emb_dim", _I), ("hidden", _I)]


class ZooLeague(C.Structure):
    """``sumo_zoo_league`` of include/sumo_hip.h: a zoo MLP table, a zoo LSTM table and the league entry of every 16-env tile of the
    whole env set (``tile_entry_dev``: device int32 [Ntot / 16]; [0, mlp.nzoo) = MLP row, then the LSTM rows)."""
    _fields_ = [("mlp", ZooMlp), ("lstm", ZooLstm), ("tile_entry_dev", _P)]


class PairSideRollout(C.Structure):
    """``sumo_pair_side`` of include/sumo_hip.h: one seat of the co-training launch (device pointers as integers)."""
    _fields_ = [("table", _P), ("tile_row", _P), ("nrows", _I), ("row_stride", _I), ("ob_dim", _I), ("ac_dim", _I), ("record_row", _I),
                ("noise", _P), ("obs", _P), ("act", _P), ("val", _P), ("nlp", _P), ("done", _P)]


class RolloutPair(C.Structure):
    """``sumo_rollout_pair`` of include/sumo_hip.h: the two seats and what the launch shares."""
    _fields_ = [("side", PairSideRollout * 2), ("T", _I), ("Ntot", _I), ("env_offset", _I), ("s0", _I), ("K", _I), ("alpha", C.c_double),
                ("rew", _P), ("ep_done", _P), ("ep_r", _P), ("ep_l", _P)]


# every fused launch of the C ABI: name -> (launch struct, the struct that follows it or None); their argtypes, their restype and
# their place in EXPORTS come from here
FUSED_ENTRIES = {
    "sumo_rollout_steps": (Rollout, None), "sumo_rollout_steps_lstm": (RolloutLstm, None),
    "sumo_match_steps": (Match, None), "sumo_match_steps_lstm": (MatchLstm, None),
    "sumo_rollout_steps_zoo": (Rollout, ZooMlp), "sumo_match_steps_zoo": (Match, ZooMlp),
    "sumo_match_steps_zoo_lstm": (Match, ZooLstm), "sumo_match_steps_lstm_zoo_lstm": (MatchLstm, ZooLstm),
    "sumo_rollout_steps_zoo_lstm": (Rollout, ZooLstm), "sumo_rollout_steps_lstm_zoo": (RolloutLstm, ZooMlp),
    "sumo_rollout_steps_lstm_zoo_lstm": (RolloutLstm, ZooLstm), "sumo_rollout_steps_zoo_league": (Rollout, ZooLeague),
    "sumo_rollout_steps_lstm_zoo_league": (RolloutLstm, ZooLeague), "sumo_match_steps_cross": (MatchCross, None),
    "sumo_match_steps_lstm_zoo": (MatchLstm, ZooMlp), "sumo_rollout_steps_lstm_reuse": (RolloutLstmReuse, None),
}
# the fused launches of mixed match-ups, bound like the ones above (a table of its own: FUSED_ENTRIES and EXPORTS list the launches of
# homogeneous scenes, which matches.py and the runner's rollout modes index)
PAIR_ENTRIES = {"sumo_rollout_steps_pair": (RolloutPair, None)}
# the env snapshot of Engine.snapshot / Engine.restore, a table of its own like the one above (EXPORTS is the tuple that the pairing
# tests pin entry by entry)
SNAPSHOT_EXPORTS = ("sumo_snapshot_bytes", "sumo_snapshot_save", "sumo_snapshot_load")
SNAPSHOT_HEADER_BYTES = 64


def lib():
    global _LIB
    if _LIB is None:
        path = os.environ.get("SUMO_HIP_LIB") or _build.lib_path("libsumo_hip.so")  # override: profiling builds
        if not os.path.exists(path):
            raise SumoHipError("%s not found: build it with `python -m robosumo_selfplay_amd.build` "
                               "(the HIP engine has no CPU fallback)" % path)
        L = C.CDLL(path)
        L.sumo_last_error.restype = C.c_char_p
        vp, i32 = C.c_void_p, C.c_int
        L.sumo_create.argtypes = [vp, C.c_size_t, i32, i32, C.POINTER(vp)]
        L.sumo_destroy.argtypes = [vp]
        L.sumo_dims.argtypes = [vp, vp]
        L.sumo_reset.argtypes = [vp, vp, vp, vp, vp]
        L.sumo_step.argtypes = [vp] * 9
        for n, (launch, second) in list(FUSED_ENTRIES.items()) + list(PAIR_ENTRIES.items()):
            getattr(L, n).argtypes = [vp] + [C.POINTER(t) for t in (launch, second) if t is not None] + [vp] * 8
            getattr(L, n).restype = i32
        L.sumo_get_state.argtypes = [vp] * 5
        L.sumo_set_cfrc_mode.argtypes = [vp, i32]
        L.sumo_get_cfrc_ext.argtypes = [vp, vp]
        L.sumo_set_adjust_z.argtypes = [vp, C.c_double]
        L.sumo_set_state.argtypes = [vp] * 5
        L.sumo_debug_forward.argtypes = [vp] * 4
        L.sumo_stats.argtypes = [vp, vp]
        L.sumo_profile.argtypes = [vp, vp]
        L.sumo_debug_trace.argtypes = [vp, vp]
        L.sumo_debug_trace.restype = i32
        L.sumo_rollout_status.argtypes = [vp, vp]
        L.sumo_rollout_status.restype = i32
        L.sumo_debug_fault.argtypes = [vp, i32]
        L.sumo_debug_fault.restype = i32
        L.sumo_static_layout.argtypes = [vp]
        L.sumo_static_layout.restype = i32
        L.sumo_profile.restype = i32
        if hasattr(L, "sumo_snapshot_bytes"):   # a SUMO_HIP_LIB build from before the snapshot exports runs everything but snapshot / restore
            L.sumo_snapshot_bytes.argtypes = [vp]
            L.sumo_snapshot_bytes.restype = C.c_size_t
            for n in SNAPSHOT_EXPORTS[1:]:
                getattr(L, n).argtypes = [vp, vp, C.c_size_t]
                getattr(L, n).restype = i32
        if hasattr(L, "sumo_debug_wave_ops"):   # a SUMO_HIP_LIB build from before these two debug exports still runs everything else (_debug_export)
            L.sumo_debug_grad_threshold.argtypes = [C.c_double, C.c_double, vp]
            L.sumo_debug_grad_threshold.restype = i32
            L.sumo_debug_wave_ops.argtypes = [vp] * 7 + [i32, C.c_double, C.c_double, vp]
            L.sumo_debug_wave_ops.restype = i32
        for n in ("sumo_create", "sumo_destroy", "sumo_dims", "sumo_reset", "sumo_step", "sumo_get_state", "sumo_set_cfrc_mode",
                  "sumo_get_cfrc_ext", "sumo_set_adjust_z", "sumo_set_state", "sumo_debug_forward", "sumo_stats"):
            getattr(L, n).restype = i32
        _LIB = L
    return _LIB


EXPORTS = (("sumo_last_error", "sumo_create", "sumo_destroy", "sumo_dims", "sumo_reset", "sumo_step") + tuple(FUSED_ENTRIES)
           + ("sumo_set_cfrc_mode", "sumo_get_cfrc_ext", "sumo_set_adjust_z", "sumo_get_state", "sumo_set_state", "sumo_debug_forward",
              "sumo_stats", "sumo_profile", "sumo_debug_trace", "sumo_rollout_status", "sumo_debug_fault", "sumo_static_layout",
              "sumo_debug_layout", "sumo_debug_model_ints", "sumo_debug_dump"))


def _np(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _chk(rc):
    if rc != 0:
        raise SumoHipError("sumo_hip error %d: %s" % (rc, lib().sumo_last_error().decode()))


def _debug_export(name):
    """One of the exports that an older SUMO_HIP_LIB build may lack (the two debug ones, the snapshot ones): a clear error instead of
    ctypes' AttributeError."""
    L = lib()
    if not hasattr(L, name):
        raise SumoHipError("%s is not exported by %s: rebuild the engine library" % (name, L._name))
    return getattr(L, name)


def grad_threshold(scale, tol):
    """Development / tests (host only): the largest float64 G with scale * sqrt(G) < tol -- the Newton loop's gradient test as a
    threshold on the squared gradient norm (sumo_debug_grad_threshold); -1 where no G >= 0 passes."""
    out = C.c_double()
    _chk(_debug_export("sumo_debug_grad_threshold")(float(scale), float(tol), C.byref(out)))
    return out.value


class Engine:
    """Thin owner of one ``sumo_handle_t``; device buffers are passed as raw pointers (ints)."""

    def __init__(self, model, num_envs, device=0):
        L = lib()
        blob = model.to_blob()
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        h = C.c_void_p()
        _chk(L.sumo_create(C.cast(buf, C.c_void_p), len(blob), int(num_envs), int(device), C.byref(h)))
        self.h = h
        self.N = int(num_envs)
        d = np.zeros(NDIMS, np.int32)
        _chk(L.sumo_dims(self.h, _np(d)))
        (self.nq, self.nv, self.nu, self.nbody, self.njnt, self.ngeom, self.npair, self.nagent, self.obs_stride,
         self.act_stride, self.maxcon, self.maxefc, self.lds_bytes, self.state_stride, self.jbcap) = [int(x) for x in d[:15]]

    def close(self):
        if getattr(self, "h", None):
            lib().sumo_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, obs_ptr, seeds=None, mask_ptr=None, stream=None):
        s = None if seeds is None else np.ascontiguousarray(seeds, np.uint64)
        if s is not None and s.shape != (self.N,):
            raise ValueError("seeds must have shape (%d,)" % self.N)
        _chk(lib().sumo_reset(self.h, _np(s), mask_ptr, obs_ptr, stream))

    def step(self, actions_ptr, obs_ptr, info_ptr, done_ptr, ep_r_ptr, ep_dr_ptr, ep_l_ptr, stream=None):
        _chk(lib().sumo_step(self.h, actions_ptr, obs_ptr, info_ptr, done_ptr, ep_r_ptr, ep_dr_ptr, ep_l_ptr, stream))

    def _fused(self, entry, launch, env_ptrs, stream, zoo=None):
        """One fused launch: ``env_ptrs`` are the seven env-side pointers of :meth:`step`, in its order; ``zoo``: the
        :class:`ZooMlp` / :class:`ZooLstm` table (or :class:`ZooLeague`) the ``*_zoo`` / ``*_zoo_lstm`` / ``*_zoo_league`` entry points take after
        the launch struct."""
        structs = (C.byref(launch),) if zoo is None else (C.byref(launch), C.byref(zoo))
        _chk(getattr(lib(), entry)(self.h, *structs, *env_ptrs, stream))

    def rollout_steps(self, ro, *env_ptrs, stream=None):
        """K fused self-play rollout steps (``sumo_rollout_steps``); ``ro`` is a filled :class:`Rollout`."""
        self._fused("sumo_rollout_steps", ro, env_ptrs, stream)

    def rollout_steps_lstm(self, ro, *env_ptrs, stream=None):
        """The same for recurrent policies (``sumo_rollout_steps_lstm``); ``ro`` is a filled :class:`RolloutLstm`."""
        self._fused("sumo_rollout_steps_lstm", ro, env_ptrs, stream)

    def rollout_steps_lstm_reuse(self, ro, *env_ptrs, stream=None):
        """The recurrent launch under opponent-data reuse (``sumo_rollout_steps_lstm_reuse``); ``ro`` is a filled
        :class:`RolloutLstmReuse` (``state2``: the learner's shadow state rows of the launch's envs, read and updated in place)."""
        self._fused("sumo_rollout_steps_lstm_reuse", ro, env_ptrs, stream)

    def match_steps(self, mo, *env_ptrs, stream=None):
        """K fused checkpoint-vs-checkpoint match steps (``sumo_match_steps``); ``mo`` is a filled :class:`Match`.  The outcome is
        read with :meth:`rollout_status`."""
        self._fused("sumo_match_steps", mo, env_ptrs, stream)

    def match_steps_lstm(self, mo, *env_ptrs, stream=None):
        """The same for recurrent checkpoints (``sumo_match_steps_lstm``); ``mo`` is a filled :class:`MatchLstm`."""
        self._fused("sumo_match_steps_lstm", mo, env_ptrs, stream)

    def rollout_steps_zoo(self, ro, zoo, *env_ptrs, stream=None):
        """K fused rollout steps against policy-zoo MLP nets (``sumo_rollout_steps_zoo``); ``ro`` is a filled :class:`Rollout`
        (``opponent_params`` None, ``npool`` = ``zoo.nzoo``), ``zoo`` a filled :class:`ZooMlp`."""
        self._fused("sumo_rollout_steps_zoo", ro, env_ptrs, stream, zoo)

    def match_steps_zoo(self, mo, zoo, *env_ptrs, stream=None):
        """K fused match steps of checkpoints (agent 0) against policy-zoo MLP nets (agent 1) (``sumo_match_steps_zoo``); ``mo`` is
        a filled :class:`Match` whose ``idx1`` indexes ``zoo``, a filled :class:`ZooMlp`."""
        self._fused("sumo_match_steps_zoo", mo, env_ptrs, stream, zoo)

    def match_steps_zoo_lstm(self, mo, zoo, *env_ptrs, stream=None):
        """K fused match steps of MLP checkpoints (agent 0) against policy-zoo LSTM nets (agent 1) (``sumo_match_steps_zoo_lstm``);
        ``mo`` is a filled :class:`Match` whose ``idx1`` indexes ``zoo``, a filled :class:`ZooLstm` (``state``: agent 1's rows)."""
        self._fused("sumo_match_steps_zoo_lstm", mo, env_ptrs, stream, zoo)

    def match_steps_lstm_zoo_lstm(self, mo, zoo, *env_ptrs, stream=None):
        """The same for LSTM(128) checkpoints (``sumo_match_steps_lstm_zoo_lstm``); ``mo`` is a filled :class:`MatchLstm` with
        ``state1`` left None (agent 1's state is ``zoo.state``)."""
        self._fused("sumo_match_steps_lstm_zoo_lstm", mo, env_ptrs, stream, zoo)

    def rollout_steps_zoo_lstm(self, ro, zoo, *env_ptrs, stream=None):
        """K fused rollout steps against policy-zoo LSTM nets (``sumo_rollout_steps_zoo_lstm``); ``ro`` is a filled :class:`Rollout`
        (``opponent_params`` None, ``npool`` = ``zoo.nzoo``), ``zoo`` a filled :class:`ZooLstm` (``state``: agent 1's rows of the
        launch's envs, read and updated in place)."""
        self._fused("sumo_rollout_steps_zoo_lstm", ro, env_ptrs, stream, zoo)

    def rollout_steps_lstm_zoo(self, ro, zoo, *env_ptrs, stream=None):
        """K fused rollout steps of a recurrent learner against policy-zoo MLP nets (``sumo_rollout_steps_lstm_zoo``); ``ro`` is a
        filled :class:`RolloutLstm` (``opponents_dev`` / ``state1`` None, ``npool`` = ``zoo.nzoo``, ``tile_net_dev`` the table row
        per 16-env tile or None), ``zoo`` a filled :class:`ZooMlp`."""
        self._fused("sumo_rollout_steps_lstm_zoo", ro, env_ptrs, stream, zoo)

    def rollout_steps_lstm_zoo_lstm(self, ro, zoo, *env_ptrs, stream=None):
        """The same against policy-zoo LSTM nets (``sumo_rollout_steps_lstm_zoo_lstm``); ``zoo`` a filled :class:`ZooLstm`
        (``state``: agent 1's rows of the launch's envs, read and updated in place)."""
        self._fused("sumo_rollout_steps_lstm_zoo_lstm", ro, env_ptrs, stream, zoo)

    def rollout_steps_zoo_league(self, ro, league, *env_ptrs, stream=None):
        """K fused rollout steps of an MLP learner against a league of policy-zoo nets of both families
        (``sumo_rollout_steps_zoo_league``); ``ro`` is a filled :class:`Rollout` (``opponent_params`` / ``opponent_index`` None,
        ``npool`` = the league's size), ``league`` a filled :class:`ZooLeague`."""
        self._fused("sumo_rollout_steps_zoo_league", ro, env_ptrs, stream, league)

    def rollout_steps_lstm_zoo_league(self, ro, league, *env_ptrs, stream=None):
        """The same for a recurrent learner (``sumo_rollout_steps_lstm_zoo_league``); ``ro`` is a filled :class:`RolloutLstm`
        (``opponents_dev`` / ``tile_net_dev`` / ``state1`` None, ``npool`` = the league's size)."""
        self._fused("sumo_rollout_steps_lstm_zoo_league", ro, env_ptrs, stream, league)

    def match_steps_cross(self, mo, *env_ptrs, stream=None):
        """K fused match steps of MLP(64,64) checkpoints against LSTM(128) checkpoints (``sumo_match_steps_cross``); ``mo`` is a
        filled :class:`MatchCross` (``lstm_side``: the agent the LSTM table plays, ``state``: that agent's rows)."""
        self._fused("sumo_match_steps_cross", mo, env_ptrs, stream)

    def match_steps_lstm_zoo(self, mo, zoo, *env_ptrs, stream=None):
        """K fused match steps of LSTM(128) checkpoints (agent 0) against policy-zoo MLP nets (agent 1)
        (``sumo_match_steps_lstm_zoo``); ``mo`` is a filled :class:`MatchLstm` with ``state1`` left None, ``zoo`` a filled
        :class:`ZooMlp` that ``idx1`` indexes."""
        self._fused("sumo_match_steps_lstm_zoo", mo, env_ptrs, stream, zoo)

    def rollout_steps_pair(self, ro, *env_ptrs, stream=None):
        """K fused co-training rollout steps of a match-up of two species (``sumo_rollout_steps_pair``); ``ro`` is a filled
        :class:`RolloutPair`: per side a table of MLP rows, the row of every 16-env tile, the row whose tiles record, and its own record."""
        self._fused("sumo_rollout_steps_pair", ro, env_ptrs, stream)

    def set_cfrc_mode(self, mode):
        """'zero' (default, the reference's behaviour) or 'rne_post' (include/sumo_hip.h: cfrc_mode)."""
        _chk(lib().sumo_set_cfrc_mode(self.h, {"zero": 0, "rne_post": 1}[mode]))

    def set_adjust_z(self, adjust_z):
        """``Agent._adjust_z`` of the reference (agents.py:33,155-161; include/sumo_hip.h: sumo_set_adjust_z)."""
        _chk(lib().sumo_set_adjust_z(self.h, float(adjust_z)))

    def get_cfrc_ext(self):
        out = np.zeros((self.N, self.nbody, 6))
        _chk(lib().sumo_get_cfrc_ext(self.h, _np(out)))
        return out

    def get_state(self):
        qpos = np.zeros((self.N, self.nq))
        qvel = np.zeros((self.N, self.nv))
        warm = np.zeros((self.N, self.nv))
        cnt = np.zeros((self.N, 2), np.int32)
        _chk(lib().sumo_get_state(self.h, _np(qpos), _np(qvel), _np(warm), _np(cnt)))
        return qpos, qvel, warm, cnt

    def set_state(self, qpos=None, qvel=None, warm=None, counters=None):
        def f(a, dt, shape):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dt)
            if a.shape != shape:
                raise ValueError("bad shape %s, expected %s" % (a.shape, shape))
            return a
        qpos = f(qpos, np.float64, (self.N, self.nq))
        qvel = f(qvel, np.float64, (self.N, self.nv))
        warm = f(warm, np.float64, (self.N, self.nv))
        counters = f(counters, np.int32, (self.N, 2))
        _chk(lib().sumo_set_state(self.h, _np(qpos), _np(qvel), _np(warm), _np(counters)))

    def snapshot(self):
        """Everything a later step's outputs depend on as one versioned blob (uint8 array; ``sumo_snapshot_save``): a 64-byte header,
        then the state rows whole, all four counter words, the seeds and, in cfrc_mode 'rne_post', the pre-step state and cfrc_ext."""
        n = int(_debug_export("sumo_snapshot_bytes")(self.h))
        blob = np.zeros(n, np.uint8)
        _chk(lib().sumo_snapshot_save(self.h, _np(blob), n))
        return blob

    def restore(self, blob):
        """Put a :meth:`snapshot` back (``sumo_snapshot_load``).  A blob of another engine shape, model, cfrc_mode or format raises
        before anything is written; the fault counters of :meth:`stats` stay this engine's own."""
        if hasattr(blob, "numpy"):
            blob = blob.numpy()
        blob = np.ascontiguousarray(np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray)) else blob, np.uint8).ravel()
        _chk(_debug_export("sumo_snapshot_load")(self.h, _np(blob), blob.size))

    def debug_forward(self, ctrl):
        ctrl = np.ascontiguousarray(ctrl, np.float64)
        if ctrl.shape != (self.N, self.nu):
            raise ValueError("ctrl must have shape (%d, %d)" % (self.N, self.nu))
        qacc = np.zeros((self.N, self.nv))
        counts = np.zeros((self.N, 4), np.int32)
        _chk(lib().sumo_debug_forward(self.h, _np(ctrl), _np(qacc), _np(counts)))
        return qacc, counts

    def debug_wave_ops(self, rows, ints, gn=(), scale=1.0, tol=0.0):
        """Development / tests: one wave through the kernels' in-wave primitives (sumo_debug_wave_ops).  rows float64 [8][64],
        ints int32 [64] -> (sums [20], row 0 pair-swapped [64], exclusive scan [64], its total, gradient test [len(gn)][2]: the
        sqrt form and the threshold form at `scale`, `tol`)."""
        rows = np.ascontiguousarray(rows, np.float64)
        ints = np.ascontiguousarray(ints, np.int32)
        gn = np.ascontiguousarray(gn, np.float64)
        if rows.shape != (8, 64) or ints.shape != (64,) or gn.ndim != 1:
            raise ValueError("rows must be [8][64], ints [64], gn one-dimensional")
        sums, swapped, scan = np.zeros(20), np.zeros(64), np.zeros(65, np.int32)
        grad = np.zeros((max(len(gn), 1), 2), np.uint8)
        _chk(_debug_export("sumo_debug_wave_ops")(self.h, _np(rows), _np(ints), _np(sums), _np(swapped), _np(scan), _np(gn) if len(gn) else None,
                                       len(gn), float(scale), float(tol), _np(grad)))
        return sums, swapped, scan[:64], int(scan[64]), grad[:len(gn)].astype(bool)

    def debug_trace(self, stamps_ptr):
        """Development: device uint64 [N][4] buffer that receives each env wave's start / end stamps and work counters (0 / None = off)."""
        _chk(lib().sumo_debug_trace(self.h, stamps_ptr or None))

    def profile(self):
        o = np.zeros(24)
        _chk(lib().sumo_profile(self.h, _np(o)))
        return o

    def stats(self):
        o = np.zeros(NSTATS)
        _chk(lib().sumo_stats(self.h, _np(o)))
        return dict(forward=o[0], newton=o[1], contacts=o[2], efc=o[3], max_ncon=o[4], max_nefc=o[5],
                    max_newton=o[6], dropped=o[7], diverged=o[8], rollout_aborts=o[9], handover_mismatches=o[10],
                    capsule_box_3=o[11], rod_endcap=o[12])

    def rollout_status(self):
        """Waits for the engine's most recent fused rollout launch and RAISES if it was cut short (``sumo_rollout_status``:
        expired hand-over wait or a hand-over tag / checksum mismatch).  Returns dict(aborted, tickets_drawn, tickets, mismatches)."""
        o = np.zeros(4, np.int64)
        _chk(lib().sumo_rollout_status(self.h, _np(o)))
        return dict(aborted=int(o[0]), tickets_drawn=int(o[1]), tickets=int(o[2]), mismatches=int(o[3]))

    def static_layout(self):
        """True if this engine runs static-Layout kernel variants (Ant-vs-Ant or Spider-vs-Spider at default settings; include/sumo_hip.h)."""
        return lib().sumo_static_layout(self.h) >= 1

    def debug_fault(self, env):
        """Tests: make the first hand-over of ``env`` in the following fused launches carry a wrong checksum (-1 = off)."""
        _chk(lib().sumo_debug_fault(self.h, int(env)))
