"""ctypes binding of include/sumo_ppo.h (csrc/libsumo_ppo.so).  No CPU fallback."""
import ctypes as C
import os

from . import build as _build

NSTATS = 8
FWD_PI, FWD_VF, FWD_TANH = 1, 2, 4
GRAD_TANH = 1
LSTM_GATES_IFOU, LSTM_GATES_IJFO = 0, 1
_LIB = None

EXPORTS = ("ppo_last_error", "ppo_param_count", "ppo_forward", "ppo_forward_filtered", "ppo_lstm_step", "ppo_lstm_step_pool", "ppo_lstm_step_save", "ppo_lstm_xproj", "ppo_lstm_step_save_z", "ppo_lstm_seq_forward", "ppo_lstm_seq_backward", "ppo_lstm_head_grad", "ppo_lstm_bwd_step", "ppo_lstm_wgrad_workspace_bytes", "ppo_lstm_wgrad", "ppo_selfplay_forward", "ppo_post_step", "ppo_reward_mix", "ppo_vtrace", "ppo_adv_moments", "ppo_adv_moments_ws", "ppo_adv_moments_workspace_bytes",
           "ppo_adv_normalize", "ppo_grad_workspace_bytes", "ppo_grad", "ppo_loss_stats", "ppo_clip_adam",
           "ppo_a2c_grad", "ppo_a2c_loss_stats", "ppo_selection_scores_workspace_bytes", "ppo_selection_scores",
           "ppo_adv_moments_masked_ws", "ppo_adv_normalize_masked", "ppo_lstm_head_grad_masked", "ppo_zoo_seat_act", "ppo_mixed_step",
           "ppo_mixed_pair_step", "ppo_grad_act", "ppo_obs_filter")


class PpoHipError(RuntimeError):
    pass


class LstmNet(C.Structure):
    """``ppo_lstm_net`` of include/sumo_ppo.h (device pointers as integers; 0 / None = absent)."""
    _fields_ = [("ob_dim", C.c_int), ("emb_dim", C.c_int), ("hidden", C.c_int), ("ac_dim", C.c_int), ("gate_order", C.c_int),
                ("forget_bias", C.c_float), ("obs_mean", C.c_void_p), ("obs_invstd", C.c_void_p), ("obs_clip", C.c_float),
                ("emb_w", C.c_void_p), ("emb_b", C.c_void_p), ("wx", C.c_void_p), ("wh", C.c_void_p), ("b", C.c_void_p),
                ("head_w", C.c_void_p), ("head_b", C.c_void_p), ("logstd", C.c_void_p), ("vf_w", C.c_void_p), ("vf_b", C.c_void_p)]


class ZooSeat(C.Structure):
    """``ppo_zoo_seat`` of include/sumo_ppo.h: the zoo nets of one seat of a zoo-vs-zoo match (device pointers as integers)."""
    _fields_ = [("mlp_params", C.c_void_p), ("mlp_filt", C.c_void_p), ("lstm_params", C.c_void_p), ("lstm_filt", C.c_void_p),
                ("tile_entry", C.c_void_p), ("state", C.c_void_p), ("n_mlp", C.c_int), ("n_lstm", C.c_int), ("ob_dim", C.c_int),
                ("ac_dim", C.c_int), ("obs_clip", C.c_float), ("forget_bias", C.c_float)]


class LearnerSeat(C.Structure):
    """``ppo_learner_seat`` of include/sumo_ppo.h: the parameter rows that may play agent 0 of a mixed match-up."""
    _fields_ = [("table", C.c_void_p), ("tile_row", C.c_void_p), ("nrows", C.c_int), ("row_stride", C.c_int), ("ob_dim", C.c_int),
                ("ac_dim", C.c_int)]


class MixedRecord(C.Structure):
    """``ppo_mixed_record`` of include/sumo_ppo.h: where ``ppo_mixed_step`` writes agent 0's rollout record (0 / None = skip)."""
    _fields_ = [("obs", C.c_void_p), ("action", C.c_void_p), ("neglogp", C.c_void_p), ("value", C.c_void_p), ("done", C.c_void_p)]


class PairSide(C.Structure):
    """``ppo_pair_side`` of include/sumo_ppo.h: one learner seat of ``ppo_mixed_pair_step`` with its buffers and record."""
    _fields_ = [("seat", LearnerSeat), ("obs", C.c_void_p), ("noise", C.c_void_p), ("done", C.c_void_p), ("action", C.c_void_p),
                ("record", MixedRecord)]


def mixed_status(tile, side):
    """The status word ``ppo_mixed_step`` leaves for a tile whose side names no table row."""
    return 1 + 2 * int(tile) + int(side)


def mixed_status_decode(status):
    """(tile, side) of a non-zero ``ppo_mixed_step`` status word."""
    status = int(status)
    if status < 1:
        raise ValueError("status %d reports no tile" % status)
    return (status - 1) >> 1, (status - 1) & 1


def fill_lstm_net_ifou(n, ob_dim, ac_dim, nlstm, addrs):
    """Fill ``n`` for a net of the layout ``learn(network='lstm')`` trains -- gate order i,f,o,u, no forget-bias offset, no embedding /
    observation filter -- from the device addresses of its eight tensors in ``policies.lstm_param_shapes`` order."""
    n.ob_dim, n.emb_dim, n.hidden, n.ac_dim = int(ob_dim), 0, int(nlstm), int(ac_dim)
    n.gate_order, n.forget_bias = LSTM_GATES_IFOU, 0.0
    n.wx, n.wh, n.b, n.head_w, n.head_b, n.logstd, n.vf_w, n.vf_b = (int(a) for a in addrs)
    return n


def lib():
    global _LIB
    if _LIB is None:
        path = os.environ.get("SUMO_PPO_LIB") or _build.lib_path("libsumo_ppo.so")
        if not os.path.exists(path):
            raise PpoHipError("%s not found: build it with `python -m robosumo_selfplay_amd.build`" % path)
        L = C.CDLL(path)
        vp, i32, f64, f32 = C.c_void_p, C.c_int, C.c_double, C.c_float
        L.ppo_last_error.restype = C.c_char_p
        L.ppo_param_count.argtypes = [i32, i32]
        L.ppo_forward.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]
        L.ppo_forward_filtered.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, f32, vp, vp, vp, vp, vp, vp, vp]
        L.ppo_lstm_step.argtypes = [C.POINTER(LstmNet), vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
        L.ppo_lstm_step_pool.argtypes = [C.POINTER(LstmNet), vp, vp, vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
        L.ppo_lstm_step_save.argtypes = [C.POINTER(LstmNet), vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp]
        L.ppo_lstm_xproj.argtypes = [C.POINTER(LstmNet), vp, i32, i32, vp, vp]
        L.ppo_lstm_step_save_z.argtypes = [C.POINTER(LstmNet), vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]
        L.ppo_lstm_seq_forward.argtypes = [C.POINTER(LstmNet), vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]
        L.ppo_lstm_seq_backward.argtypes = [C.POINTER(LstmNet), i32, i32, vp, vp, vp, vp, vp, vp, vp]
        L.ppo_lstm_head_grad.argtypes = [C.POINTER(LstmNet), vp, i32, vp, vp, vp, vp, vp, f64, f32, f32, vp, vp, vp, vp, vp, vp]
        L.ppo_lstm_head_grad_masked.argtypes = [C.POINTER(LstmNet), vp, i32, vp, vp, vp, vp, vp, vp, vp, f32, f32, vp, vp, vp, vp, vp, vp]
        L.ppo_lstm_bwd_step.argtypes = [C.POINTER(LstmNet), i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.ppo_lstm_wgrad_workspace_bytes.argtypes = [i32, i32, i32]
        L.ppo_lstm_wgrad_workspace_bytes.restype = C.c_size_t
        L.ppo_lstm_wgrad.argtypes = [C.POINTER(LstmNet), i32, vp, vp, vp, vp, vp, vp, vp, f32, vp, vp, vp]
        L.ppo_zoo_seat_act.argtypes = [C.POINTER(ZooSeat), vp, i32, i32, vp, i32, vp, vp, i32, vp, vp]
        L.ppo_mixed_step.argtypes = [C.POINTER(LearnerSeat), C.POINTER(ZooSeat), vp, vp, i32, i32, vp, i32, vp, vp, vp, vp, i32,
                                     C.POINTER(MixedRecord), vp, vp]
        L.ppo_mixed_pair_step.argtypes = [C.POINTER(PairSide), i32, i32, i32, i32, vp, vp]
        L.ppo_reward_mix.argtypes = [vp, i32, f64, vp, i32, vp]
        L.ppo_selfplay_forward.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, C.POINTER(vp), C.POINTER(vp), vp]
        L.ppo_post_step.argtypes = [vp, i32, f64, vp, i32, vp, vp, vp, vp, vp, vp, vp]
        L.ppo_vtrace.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, f64, f64, f64, f64, vp, vp, vp, vp, vp]
        L.ppo_adv_moments.argtypes = [vp, vp, vp, i32, vp, vp]
        L.ppo_adv_moments_ws.argtypes = [vp, vp, vp, i32, vp, vp, vp]
        L.ppo_adv_moments_workspace_bytes.argtypes = []
        L.ppo_adv_moments_workspace_bytes.restype = C.c_size_t
        L.ppo_adv_normalize.argtypes = [vp, vp, vp, i32, vp, vp, vp]
        L.ppo_adv_moments_masked_ws.argtypes = [vp, vp, vp, i32, vp, vp, vp]
        L.ppo_adv_normalize_masked.argtypes = [vp, vp, vp, i32, vp, vp, vp]
        L.ppo_grad_workspace_bytes.argtypes = [i32, i32]
        L.ppo_grad_workspace_bytes.restype = C.c_size_t
        L.ppo_grad.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, f64, f32, f32, f32, vp, vp, vp, vp, vp]
        L.ppo_grad_act.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, f64, f32, f32, f32, i32, f32, f32, vp, vp, vp, vp, vp]
        L.ppo_obs_filter.argtypes = [vp, i32, i32, i32, vp, vp, f32, vp, i32, vp]
        L.ppo_loss_stats.argtypes = [vp, vp, i32, vp, vp]
        L.ppo_a2c_grad.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, i32, f64, f32, f32, vp, vp, vp, vp]
        L.ppo_a2c_loss_stats.argtypes = [vp, vp, i32, vp, vp]
        L.ppo_selection_scores_workspace_bytes.argtypes = []
        L.ppo_selection_scores_workspace_bytes.restype = C.c_size_t
        L.ppo_selection_scores.argtypes = [vp, vp, i32, vp, i32, vp, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp]
        L.ppo_clip_adam.argtypes = [vp, vp, vp, vp, i32, i32, f64, f64, f64, f64, f64, vp, vp]
        for n in EXPORTS:
            if n not in ("ppo_last_error", "ppo_grad_workspace_bytes", "ppo_lstm_wgrad_workspace_bytes", "ppo_adv_moments_workspace_bytes",
                         "ppo_selection_scores_workspace_bytes"):
                getattr(L, n).restype = i32
        _LIB = L
    return _LIB


def chk(rc):
    if rc != 0:
        raise PpoHipError("sumo_ppo error %d: %s" % (rc, lib().ppo_last_error().decode()))


def ptr(t):
    return None if t is None else t.data_ptr()
