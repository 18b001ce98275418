"""Fixed opponents from the OpenAI RoboSumo policy zoo + the win/draw/lose evaluator, on the HIP forward kernel.

Reference:
  * robosumo/robosumo/policy_zoo/policy.py:23-91   ``MLPPolicy`` (tanh 64-64 value and policy trunks, state-independent
    logstd, running-mean observation filter clipped to +-5, value de-normalised by the return filter)
  * robosumo/robosumo/policy_zoo/utils.py:9-33     ``RunningMeanStd`` (sum / sumsq / count, std = sqrt(max(var, 1e-2)))
  * robosumo/robosumo/policy_zoo/utils.py:66-83    flat ``.npy`` parameter vector in TF variable-creation order
  * eval_robosumo_against_fix.py:150-230           evaluation loop (learner deterministic on obs[:,0], zoo opponent
    deterministic on obs[:,1,:-1], 'winner' bookkeeping)
  * alg_ppo.py:194-206                             ``opponent_mode='fix'``

MLP and LSTM zoo nets are built (policy.py:23-91 and :94-199); the LSTM one keeps a per-env recurrent state on the device.
Both families also play inside the fused rollout and match launches from device tables: :class:`ZooTable` (MLP nets) and
:class:`ZooLstmTable` (LSTM nets, policy branch only).  :class:`ZooLeague` deals several nets of either family over the 16-env
tiles of a training run.
The ``.npy`` files are loaded with ``numpy.load(allow_pickle=False)``.
"""
import numpy as np

from . import ppo_capi
from .policies import HIDDEN, flatten_params

# TF variable-creation order of MLPPolicy(normalize=True) -- policy.py:38-70
_ZOO_MLP_ORDER = ["retfilter/sum", "retfilter/sumsq", "retfilter/count", "obsfilter/sum", "obsfilter/sumsq", "obsfilter/count",
                  "vffc1/w", "vffc1/b", "vffc2/w", "vffc2/b", "vffinal/w", "vffinal/b",
                  "polfc1/w", "polfc1/b", "polfc2/w", "polfc2/b", "polfinal/w", "polfinal/b", "logstd"]


def zoo_mlp_shapes(ob_dim, ac_dim, hidden=HIDDEN):
    h = hidden
    return {"retfilter/sum": (), "retfilter/sumsq": (), "retfilter/count": (),
            "obsfilter/sum": (ob_dim,), "obsfilter/sumsq": (ob_dim,), "obsfilter/count": (),
            "vffc1/w": (ob_dim, h), "vffc1/b": (h,), "vffc2/w": (h, h), "vffc2/b": (h,), "vffinal/w": (h, 1), "vffinal/b": (1,),
            "polfc1/w": (ob_dim, h), "polfc1/b": (h,), "polfc2/w": (h, h), "polfc2/b": (h,), "polfinal/w": (h, ac_dim),
            "polfinal/b": (ac_dim,), "logstd": (1, ac_dim)}


def zoo_mlp_param_count(ob_dim, ac_dim, hidden=HIDDEN):
    return int(sum(int(np.prod(s)) for s in zoo_mlp_shapes(ob_dim, ac_dim, hidden).values()))


def infer_ob_dim(nparams, ac_dim, hidden=HIDDEN):
    """Observation width of a flat zoo MLP vector (the count is affine in ob_dim)."""
    c0, c1 = zoo_mlp_param_count(0, ac_dim, hidden), zoo_mlp_param_count(1, ac_dim, hidden)
    d, r = divmod(nparams - c0, c1 - c0)
    if r != 0 or d <= 0:
        raise ValueError("%d parameters do not fit a zoo MLP policy with %d actions" % (nparams, ac_dim))
    return int(d)


def split_zoo_mlp(flat, ac_dim, hidden=HIDDEN):
    """utils.py:70-83 ``set_from_flat``: consecutive slices in variable order."""
    flat = np.asarray(flat, np.float32).ravel()
    ob_dim = infer_ob_dim(flat.size, ac_dim, hidden)
    shapes = zoo_mlp_shapes(ob_dim, ac_dim, hidden)
    out, o = {}, 0
    for k in _ZOO_MLP_ORDER:
        n = int(np.prod(shapes[k]))
        out[k] = flat[o:o + n].reshape(shapes[k]).copy()
        o += n
    return ob_dim, out


def filter_stats(p, prefix):
    """RunningMeanStd.mean / .std (utils.py:30-32), float32 like the TF graph."""
    cnt = np.float32(p[prefix + "/count"])
    mean = (p[prefix + "/sum"] / cnt).astype(np.float32)
    var = (p[prefix + "/sumsq"] / cnt).astype(np.float32) - np.square(mean)
    std = np.sqrt(np.maximum(var, np.float32(1e-2))).astype(np.float32)
    return mean, std


def zoo_kernel_flat(p):
    """The kernel's flat layout (sumo_ppo.h) of a split zoo MLP net: pi trunk, vf trunk, pi head, logstd, vf head."""
    return flatten_params([p["polfc1/w"], p["polfc1/b"], p["polfc2/w"], p["polfc2/b"], p["vffc1/w"], p["vffc1/b"],
                           p["vffc2/w"], p["vffc2/b"], p["polfinal/w"], p["polfinal/b"], p["logstd"], p["vffinal/w"],
                           p["vffinal/b"]])


def zoo_table_rows(flats, ac_dim):
    """Host rows of a device table of zoo MLP nets (include/sumo_hip.h ``sumo_zoo_mlp``) from flat ``.npy`` vectors:
    ``(params [n][Pz], filt [n][2][Dz])`` float32 -- each net in the kernel's flat layout, and its observation filter's
    mean | 1 / std.  Zoo LSTM vectors and vectors of different ``ob_dim`` raise ``ValueError``."""
    flats = [np.asarray(f, np.float32).ravel() for f in flats]
    if not flats:
        raise ValueError("a zoo table needs at least one net")
    params, filt, dims = [], [], []
    for k, f in enumerate(flats):
        try:
            ob_dim, p = split_zoo_mlp(f, ac_dim)
        except ValueError:
            try:
                split_zoo_lstm(f, ac_dim)
            except ValueError:
                raise ValueError("net %d: %d parameters fit neither zoo policy with %d actions" % (k, f.size, ac_dim))
            raise ValueError("net %d is a zoo LSTM policy: a ZooTable holds zoo MLP nets only (zoo LSTM nets play from a "
                             "ZooLstmTable, or step by step as ZooLSTMPolicy)" % k)
        mean, std = filter_stats(p, "obsfilter")
        params.append(zoo_kernel_flat(p))
        filt.append(np.stack([mean, (np.float32(1.0) / std).astype(np.float32)]))
        dims.append(ob_dim)
    if len(set(dims)) != 1:
        raise ValueError("the nets of one zoo table share ob_dim; got %s" % sorted(set(dims)))
    return np.stack(params).astype(np.float32), np.stack(filt).astype(np.float32)


class ZooTable(object):
    """Device table of frozen zoo MLP nets for the fused launches (``sumo_rollout_steps_zoo`` / ``sumo_match_steps_zoo``):
    ``params [n][Pz]`` and ``filt [n][2][ob_dim]`` CUDA tensors.  ``sources``: ``.npy`` paths, flat vectors or
    :class:`ZooMLPPolicy` objects (a :class:`ZooLSTMPolicy` or an LSTM-shaped vector is refused)."""

    obs_clip = 5.0

    def __init__(self, sources, ac_dim, device=0):
        import os
        import torch
        self.device = torch.device("cuda", int(device)) if not isinstance(device, torch.device) else device
        self.ac_dim = int(ac_dim)
        flats, self.labels = [], []
        for src in sources:
            if isinstance(src, ZooLSTMPolicy):
                raise ValueError("a ZooLSTMPolicy does not play in a ZooTable (zoo MLP nets only): use ZooLstmTable")
            self.labels.append(str(src) if isinstance(src, (str, os.PathLike)) else None)
            if isinstance(src, ZooMLPPolicy):
                if src.ac_dim != self.ac_dim:
                    raise ValueError("zoo policy has %d actions, the table %d" % (src.ac_dim, self.ac_dim))
                flats.append(src.flat)
            elif isinstance(src, (str, os.PathLike)):
                flats.append(np.load(os.path.expanduser(str(src)), allow_pickle=False))
            else:
                flats.append(src)
        params, filt = zoo_table_rows(flats, self.ac_dim)
        self.capacity, self.ob_dim = int(params.shape[0]), int(filt.shape[2])
        self.params = torch.from_numpy(params).to(self.device)
        self.filt = torch.from_numpy(filt).to(self.device)

    def struct(self):
        """The ``capi.ZooMlp`` launch struct of this table (the tensors stay owned by the table)."""
        from . import capi
        z = capi.ZooMlp()
        z.params, z.filt, z.obs_clip, z.nzoo, z.ob_dim = self.params.data_ptr(), self.filt.data_ptr(), self.obs_clip, self.capacity, self.ob_dim
        return z


# order of a zoo LSTM net's row in the fused launches' table (include/sumo_hip.h ``sumo_zoo_lstm``): the policy branch only
_ZOO_LSTM_ROW = ("p/emb/w", "p/emb/b", "lstmp/kernel", "lstmp/bias", "p/out/w", "p/out/b", "logstd")


def zoo_lstm_table_rows(flats, ac_dim):
    """Host rows of a device table of zoo LSTM nets (include/sumo_hip.h ``sumo_zoo_lstm``) from flat ``.npy`` vectors:
    ``(params [n][Pz], filt [n][2][Dz])`` float32 -- each net's policy branch in the order ``p/emb/w | p/emb/b | lstmp/kernel |
    lstmp/bias | p/out/w | p/out/b | logstd`` (row-major slices of :func:`split_zoo_lstm`), and its observation filter's
    mean | 1 / std.  Zoo MLP vectors, vectors that fit neither family and vectors of different ``ob_dim`` raise ``ValueError``."""
    flats = [np.asarray(f, np.float32).ravel() for f in flats]
    if not flats:
        raise ValueError("a zoo table needs at least one net")
    params, filt, dims = [], [], []
    for k, f in enumerate(flats):
        try:
            ob_dim, p = split_zoo_lstm(f, ac_dim)
        except ValueError:
            try:
                infer_ob_dim(f.size, ac_dim)
            except ValueError:
                raise ValueError("net %d: %d parameters fit neither zoo policy with %d actions" % (k, f.size, ac_dim))
            raise ValueError("net %d is a zoo MLP policy: a ZooLstmTable holds zoo LSTM nets only (zoo MLP nets play from a "
                             "ZooTable)" % k)
        mean, std = filter_stats(p, "obsfilter")
        params.append(np.concatenate([np.asarray(p[n], np.float32).ravel() for n in _ZOO_LSTM_ROW]))
        filt.append(np.stack([mean, (np.float32(1.0) / std).astype(np.float32)]))
        dims.append(ob_dim)
    if len(set(dims)) != 1:
        raise ValueError("the nets of one zoo table share ob_dim; got %s" % sorted(set(dims)))
    return np.stack(params).astype(np.float32), np.stack(filt).astype(np.float32)


def zoo_file_kind(nparams, ac_dim):
    """'mlp' or 'lstm': the zoo family whose layout a flat vector of ``nparams`` entries fits; ``ValueError`` if it fits neither.
    Both counts grow by 130 per observation column (two filter sums plus two 64-wide input layers) and their offsets differ by 8
    modulo 130 for every ``ac_dim``, so no length fits both families; should other widths ever make one fit both, it is refused
    rather than guessed."""
    def fits(c0, c1):
        d, r = divmod(int(nparams) - c0, c1 - c0)
        return r == 0 and d > 0

    mlp = fits(zoo_mlp_param_count(0, ac_dim), zoo_mlp_param_count(1, ac_dim))
    lstm = fits(zoo_lstm_param_count(0, ac_dim), zoo_lstm_param_count(1, ac_dim))
    if mlp and lstm:
        raise ValueError("%d parameters fit a zoo MLP and a zoo LSTM policy with %d actions: the family cannot be read from the "
                         "length" % (nparams, ac_dim))
    if not mlp and not lstm:
        raise ValueError("%d parameters fit neither zoo policy with %d actions" % (nparams, ac_dim))
    return "mlp" if mlp else "lstm"


class ZooLstmTable(object):
    """Device table of frozen zoo LSTM nets for the fused launches (``sumo_match_steps_zoo_lstm`` /
    ``sumo_match_steps_lstm_zoo_lstm`` / ``sumo_rollout_steps_zoo_lstm``): ``params [n][Pz]`` and ``filt [n][2][ob_dim]`` CUDA tensors, plus one ``ppo_lstm_net``
    per row (``nets``, filled as ``ZooLSTMPolicy._nets["p"]``) for the step-by-step path.  ``sources``: ``.npy`` paths, flat
    vectors or :class:`ZooLSTMPolicy` objects (a :class:`ZooMLPPolicy` or an MLP-shaped vector is refused)."""

    recurrent = True
    obs_clip = 5.0
    forget_bias = 1.0        # tf BasicLSTMCell
    emb = hidden = HIDDEN

    def __init__(self, sources, ac_dim, device=0):
        import os
        import torch
        self.device = torch.device("cuda", int(device)) if not isinstance(device, torch.device) else device
        self.ac_dim = int(ac_dim)
        flats, self.labels = [], []
        for src in sources:
            if isinstance(src, ZooMLPPolicy):
                raise ValueError("a ZooMLPPolicy does not play in a ZooLstmTable (zoo LSTM nets only): use ZooTable")
            self.labels.append(str(src) if isinstance(src, (str, os.PathLike)) else None)
            if isinstance(src, ZooLSTMPolicy):
                if src.ac_dim != self.ac_dim:
                    raise ValueError("zoo policy has %d actions, the table %d" % (src.ac_dim, self.ac_dim))
                flats.append(src.flat)
            elif isinstance(src, (str, os.PathLike)):
                flats.append(np.load(os.path.expanduser(str(src)), allow_pickle=False))
            else:
                flats.append(src)
        params, filt = zoo_lstm_table_rows(flats, self.ac_dim)
        self.capacity, self.ob_dim = int(params.shape[0]), int(filt.shape[2])
        self.params = torch.from_numpy(params).to(self.device)
        self.filt = torch.from_numpy(filt).to(self.device)
        D, E, H, A = self.ob_dim, self.emb, self.hidden, self.ac_dim
        self.nets = (ppo_capi.LstmNet * self.capacity)()
        for k in range(self.capacity):
            n, base = self.nets[k], self.params[k].data_ptr()
            n.ob_dim, n.emb_dim, n.hidden, n.ac_dim = D, E, H, A
            n.gate_order, n.forget_bias = ppo_capi.LSTM_GATES_IJFO, self.forget_bias
            n.obs_mean, n.obs_invstd, n.obs_clip = self.filt[k, 0].data_ptr(), self.filt[k, 1].data_ptr(), self.obs_clip
            o = 0
            for name, size in (("emb_w", D * E), ("emb_b", E), ("wx", E * 4 * H), ("wh", H * 4 * H), ("b", 4 * H), ("head_w", H * A),
                               ("head_b", A), ("logstd", A)):
                setattr(n, name, base + 4 * o)
                o += size
            assert o == self.params.shape[1]

    def struct(self, state):
        """The ``capi.ZooLstm`` launch struct of this table with agent 1's state rows ``state`` (contiguous float32 CUDA
        [n][2 * 64], c | h); the tensors stay owned by their holders."""
        from . import capi
        z = capi.ZooLstm()
        z.params, z.filt, z.state = self.params.data_ptr(), self.filt.data_ptr(), state.data_ptr()
        z.obs_clip, z.forget_bias, z.nzoo, z.ob_dim, z.emb_dim, z.hidden = self.obs_clip, self.forget_bias, self.capacity, self.ob_dim, self.emb, self.hidden
        return z


class ZooMLPPolicy(object):
    """One zoo MLP net resident on the GPU.  ``act`` follows policy.py:72-79; ``step`` / ``value`` /
    ``action_probability`` follow the PolicyWithValue surface so the object can sit in ``Runner.models[1]``
    (``opponent_mode='fix'``).  Observations may carry extra trailing columns (the time feature): only the first
    ``ob_dim`` are read, which is the ``obs[:, 1, :-1]`` of eval_robosumo_against_fix.py:206."""

    initial_state = None
    recurrent = False

    def __init__(self, flat_params, ac_dim, device=0):
        import torch
        self._t = torch
        self.device = torch.device("cuda", int(device)) if not isinstance(device, torch.device) else device
        self.ac_dim = int(ac_dim)
        self.flat = np.asarray(flat_params, np.float32).ravel().copy()     # the zoo's own vector (ZooTable reads it)
        self.ob_dim, p = split_zoo_mlp(self.flat, ac_dim)
        self.tensors = p
        mean, std = filter_stats(p, "obsfilter")
        self.ret_mean, self.ret_std = [float(x) for x in filter_stats(p, "retfilter")]
        flat = zoo_kernel_flat(p)
        self.params = torch.from_numpy(flat).to(self.device)
        self.obs_mean = torch.from_numpy(mean).to(self.device)
        self.obs_invstd = torch.from_numpy((np.float32(1.0) / std).astype(np.float32)).to(self.device)
        self.gen = torch.Generator(device=self.device)

    def seed(self, s):
        self.gen.manual_seed(int(s))

    def reset(self, **kwargs):   # policy.py:13-15
        pass

    def _prep(self, x, min_cols):
        t = self._t
        np_in = isinstance(x, np.ndarray) or not t.is_tensor(x)
        if np_in:
            x = np.asarray(x, np.float32)
            if x.ndim == 1:
                x = x[None]
            x = t.from_numpy(np.ascontiguousarray(x)).to(self.device)
        if x.dtype != t.float32 or not x.is_cuda or x.dim() != 2 or x.stride(1) != 1 or x.shape[1] < min_cols:
            raise ValueError("expected float32 [n, >=%d] observations with unit inner stride" % min_cols)
        return x, np_in

    def evaluate(self, obs, flags, given_action=None, deterministic=False, out=None, noise=None):
        """Same contract as ``PolicyWithValue.evaluate`` (device tensors in, dict of device tensors out; ``out`` may hold
        preallocated outputs), so the device-mode Runner can drive a zoo opponent.  ``noise``: explicit standard-normal rows
        (contiguous float32 CUDA [n, ac_dim]) for the sampled action instead of a draw from ``self.gen``."""
        t = self._t
        ob, _ = self._prep(obs, self.ob_dim)
        n, A = ob.shape[0], self.ac_dim
        out = out or {}
        action = neglogp = value = given = None
        if flags & ppo_capi.FWD_PI:
            action = out.get("action")
            if action is None:
                action = t.empty((n, A), dtype=t.float32, device=self.device)
            neglogp = out.get("neglogp")
            if neglogp is None:
                neglogp = t.empty(n, dtype=t.float32, device=self.device)
            if given_action is not None:
                given, _ = self._prep(given_action, A)
                given = given.contiguous()
                noise = None
            elif deterministic:
                noise = None
            elif noise is None:
                noise = t.randn((n, A), generator=self.gen, device=self.device, dtype=t.float32)
            elif tuple(noise.shape) != (n, A) or noise.dtype != t.float32 or not noise.is_cuda or not noise.is_contiguous():
                raise ValueError("noise must be a contiguous float32 CUDA tensor of shape (%d, %d)" % (n, A))
        else:
            noise = None
        if flags & ppo_capi.FWD_VF:
            value = out.get("value")
            if value is None:
                value = t.empty(n, dtype=t.float32, device=self.device)
        st = t.cuda.current_stream(self.device).cuda_stream
        ppo_capi.chk(ppo_capi.lib().ppo_forward_filtered(
            self.params.data_ptr(), ob.data_ptr(), n, ob.stride(0) if n > 1 else ob.shape[1], self.ob_dim, A, flags | ppo_capi.FWD_TANH,
            self.obs_mean.data_ptr(), self.obs_invstd.data_ptr(), 5.0, ppo_capi.ptr(noise), ppo_capi.ptr(given),
            ppo_capi.ptr(action), ppo_capi.ptr(neglogp), ppo_capi.ptr(value), None, st))
        if value is not None:
            value.mul_(self.ret_std).add_(self.ret_mean)          # policy.py:58-60
        return dict(action=action, neglogp=neglogp, value=value)

    @staticmethod
    def _np(x):
        return isinstance(x, np.ndarray) or not hasattr(x, "is_cuda")

    def _ret(self, x, np_in):
        return x.cpu().numpy() if np_in else x

    # ---- zoo surface (policy.py:72-79) ----------------------------------------------------------------------------
    def act(self, observation, stochastic=True):
        np_in = self._np(observation)
        single = np_in and np.asarray(observation).ndim == 1
        r = self.evaluate(observation, ppo_capi.FWD_PI | ppo_capi.FWD_VF, deterministic=not stochastic)
        a, v = self._ret(r["action"], np_in), self._ret(r["value"], np_in)
        return (a[0], {"vpred": v[0]}) if single else (a, {"vpred": v})

    # ---- PolicyWithValue surface (policies.py:84-128 of the reference) -------------------------------------------
    def step(self, observation, deterministic=False, **extra_feed):
        np_in = self._np(observation)
        r = self.evaluate(observation, ppo_capi.FWD_PI | ppo_capi.FWD_VF, deterministic=deterministic)
        return self._ret(r["action"], np_in), self._ret(r["value"], np_in), None, self._ret(r["neglogp"], np_in)

    def value(self, ob, *args, **kwargs):
        return self._ret(self.evaluate(ob, ppo_capi.FWD_VF)["value"], self._np(ob))

    def action_probability(self, observation, given_action=None, **extra_feed):
        return self._ret(self.evaluate(observation, ppo_capi.FWD_PI, given_action=given_action)["neglogp"], self._np(observation))


# TF variable-creation order of LSTMPolicy(hiddens=[E, H], normalize=True) -- policy.py:106-183
_ZOO_LSTM_ORDER = ["retfilter/sum", "retfilter/sumsq", "retfilter/count", "obsfilter/sum", "obsfilter/sumsq", "obsfilter/count",
                   "v/emb/w", "v/emb/b", "lstmv/kernel", "lstmv/bias", "v/out/w", "v/out/b",
                   "p/emb/w", "p/emb/b", "lstmp/kernel", "lstmp/bias", "p/out/w", "p/out/b", "logstd"]


def zoo_lstm_shapes(ob_dim, ac_dim, emb=HIDDEN, hidden=HIDDEN):
    e, h = emb, hidden
    return {"retfilter/sum": (), "retfilter/sumsq": (), "retfilter/count": (),
            "obsfilter/sum": (ob_dim,), "obsfilter/sumsq": (ob_dim,), "obsfilter/count": (),
            "v/emb/w": (ob_dim, e), "v/emb/b": (e,), "lstmv/kernel": (e + h, 4 * h), "lstmv/bias": (4 * h,), "v/out/w": (h, 1), "v/out/b": (1,),
            "p/emb/w": (ob_dim, e), "p/emb/b": (e,), "lstmp/kernel": (e + h, 4 * h), "lstmp/bias": (4 * h,), "p/out/w": (h, ac_dim),
            "p/out/b": (ac_dim,), "logstd": (1, ac_dim)}


def zoo_lstm_param_count(ob_dim, ac_dim, emb=HIDDEN, hidden=HIDDEN):
    return int(sum(int(np.prod(s)) for s in zoo_lstm_shapes(ob_dim, ac_dim, emb, hidden).values()))


def split_zoo_lstm(flat, ac_dim, emb=HIDDEN, hidden=HIDDEN):
    flat = np.asarray(flat, np.float32).ravel()
    c0, c1 = zoo_lstm_param_count(0, ac_dim, emb, hidden), zoo_lstm_param_count(1, ac_dim, emb, hidden)
    ob_dim, r = divmod(flat.size - c0, c1 - c0)
    if r != 0 or ob_dim <= 0:
        raise ValueError("%d parameters do not fit a zoo LSTM policy with %d actions" % (flat.size, ac_dim))
    shapes = zoo_lstm_shapes(int(ob_dim), ac_dim, emb, hidden)
    out, o = {}, 0
    for k in _ZOO_LSTM_ORDER:
        n = int(np.prod(shapes[k]))
        out[k] = flat[o:o + n].reshape(shapes[k]).copy()
        o += n
    return int(ob_dim), out


class ZooLSTMPolicy(object):
    """policy.py:94-199 on the device: observation filter -> relu embedding (64) -> BasicLSTMCell(64) -> head, separately
    for the value and the policy (two cells).  The recurrent state of every env lives in ``self.state`` ([4][n][64]:
    value c, value h, policy c, policy h -- the reference's ``zero_state`` order); ``reset(mask)`` zeroes the rows of
    finished episodes (the reference calls ``policy.reset()`` when an episode starts).

    ``step`` / ``value`` / ``action_probability`` are the surface ``FixedOpponentModel`` and the ``Runner`` call
    (``opponent_mode='fix'``), with the Runner's rules for recurrent opponents: the acting call masks the state rows by the done
    flags ``M`` of the previous step and advances them, the scoring call (``given_action``) is one cell evaluation from a zero
    state that writes no state.  :meth:`evaluate` is the same on explicit noise rows and an explicit state.  All of them are
    ``ppo_lstm_step`` launches on the policy branch (``value``: on the value branch)."""

    recurrent = True
    initial_state = None     # the acting state lives in the policy (``S=None``) or in the caller's tensor

    def __init__(self, flat_params, ac_dim, device=0, emb=HIDDEN, hidden=HIDDEN):
        import torch
        self._t = torch
        self.device = torch.device("cuda", int(device)) if not isinstance(device, torch.device) else device
        self.ac_dim, self.emb, self.hidden = int(ac_dim), int(emb), int(hidden)
        self.flat = np.asarray(flat_params, np.float32).ravel().copy()     # the zoo's own vector (ZooLstmTable reads it)
        self.ob_dim, p = split_zoo_lstm(self.flat, ac_dim, emb, hidden)
        self.tensors = p
        mean, std = filter_stats(p, "obsfilter")
        self.ret_mean, self.ret_std = [float(x) for x in filter_stats(p, "retfilter")]
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.device)
        self.dev = {k: dev(v) for k, v in p.items() if "/" in k and not k.startswith(("retfilter", "obsfilter"))}
        self.dev["logstd"] = dev(p["logstd"])
        self.obs_mean, self.obs_invstd = dev(mean), dev(np.float32(1.0) / std)
        self.gen = torch.Generator(device=self.device)
        self.state = None
        self._nets = {}
        for br, cell, head in (("v", "lstmv", None), ("p", "lstmp", "p/out")):
            n = ppo_capi.LstmNet()
            n.ob_dim, n.emb_dim, n.hidden, n.ac_dim = self.ob_dim, self.emb, self.hidden, self.ac_dim
            n.gate_order, n.forget_bias = ppo_capi.LSTM_GATES_IJFO, 1.0          # tf BasicLSTMCell: (i, j, f, o), forget_bias 1
            n.obs_mean, n.obs_invstd, n.obs_clip = self.obs_mean.data_ptr(), self.obs_invstd.data_ptr(), 5.0
            n.emb_w, n.emb_b = self.dev[br + "/emb/w"].data_ptr(), self.dev[br + "/emb/b"].data_ptr()
            k = self.dev[cell + "/kernel"]
            n.wx, n.wh, n.b = k.data_ptr(), k.data_ptr() + 4 * self.emb * 4 * self.hidden, self.dev[cell + "/bias"].data_ptr()
            if head:
                n.head_w, n.head_b, n.logstd = self.dev["p/out/w"].data_ptr(), self.dev["p/out/b"].data_ptr(), self.dev["logstd"].data_ptr()
            else:
                n.vf_w, n.vf_b = self.dev["v/out/w"].data_ptr(), self.dev["v/out/b"].data_ptr()
            self._nets[br] = n

    def seed(self, s):
        self.gen.manual_seed(int(s))

    def reset(self, mask=None, **kwargs):
        """policy.py:198-199; ``mask`` (bool / uint8 [n], host or device) restricts the reset to those rows."""
        if self.state is None:
            return
        if mask is None:
            self.state.zero_()
        else:
            m = self._t.as_tensor(mask, device=self.device).to(self._t.bool)
            self.state[:, m, :] = 0.0

    def act(self, observation, stochastic=True, want_value=False):
        t = self._t
        np_in = isinstance(observation, np.ndarray) or not t.is_tensor(observation)
        x = observation
        single = False
        if np_in:
            x = np.asarray(x, np.float32)
            single = x.ndim == 1
            x = t.from_numpy(np.ascontiguousarray(x[None] if single else x)).to(self.device)
        if x.dtype != t.float32 or x.dim() != 2 or x.stride(1) != 1 or x.shape[1] < self.ob_dim:
            raise ValueError("expected float32 [n, >=%d] observations with unit inner stride" % self.ob_dim)
        n, A, H = x.shape[0], self.ac_dim, self.hidden
        if self.state is None or self.state.shape[1] != n:
            self.state = t.zeros((4, n, H), dtype=t.float32, device=self.device)
        action = t.empty((n, A), dtype=t.float32, device=self.device)
        noise = t.randn((n, A), generator=self.gen, device=self.device, dtype=t.float32) if stochastic else None
        st = t.cuda.current_stream(self.device).cuda_stream
        stride = x.stride(0) if n > 1 else x.shape[1]
        L = ppo_capi.lib()
        import ctypes as C
        ppo_capi.chk(L.ppo_lstm_step(C.byref(self._nets["p"]), x.data_ptr(), n, stride, None, self.state[2].data_ptr(),
                                     self.state[3].data_ptr(), H, ppo_capi.ptr(noise), None, action.data_ptr(), None, None, None, st))
        info = {"state": self.state}
        if want_value:
            value = t.empty(n, dtype=t.float32, device=self.device)
            ppo_capi.chk(L.ppo_lstm_step(C.byref(self._nets["v"]), x.data_ptr(), n, stride, None, self.state[0].data_ptr(),
                                         self.state[1].data_ptr(), H, None, None, None, None, value.data_ptr(), None, st))
            value = value * self.ret_std + self.ret_mean
            info["vpred"] = value.cpu().numpy() if np_in else value
            if single:
                info["vpred"] = info["vpred"][0]
        a = action.cpu().numpy() if np_in else action
        return (a[0] if single else a), info


    # ---- PolicyWithValue surface (policies.py:84-128 of the reference) with the S / M feeds of models.py:163-170 ---------------
    def _obs(self, x):
        t = self._t
        np_in = isinstance(x, np.ndarray) or not t.is_tensor(x)
        if np_in:
            x = np.asarray(x, np.float32)
            x = t.from_numpy(np.ascontiguousarray(x[None] if x.ndim == 1 else x)).to(self.device)
        if x.dtype != t.float32 or not x.is_cuda or x.dim() != 2 or x.stride(1) != 1 or x.shape[1] < self.ob_dim:
            raise ValueError("expected float32 [n, >=%d] observations with unit inner stride" % self.ob_dim)
        return x, np_in

    def _own_state(self, n):
        if self.state is None or self.state.shape[1] != n:
            self.state = self._t.zeros((4, n, self.hidden), dtype=self._t.float32, device=self.device)
        return self.state

    def _mask(self, M, n):
        t = self._t
        if M is None:
            return None
        m = (M if t.is_tensor(M) else t.from_numpy(np.ascontiguousarray(np.asarray(M).reshape(-1), np.float32))).to(self.device, t.float32)
        if tuple(m.shape) != (n,):
            raise ValueError("the done mask must have shape (%d,)" % n)
        return m.contiguous()

    def evaluate(self, obs, state=None, mask=None, given_action=None, deterministic=False, noise=None, out=None):
        """One ``ppo_lstm_step`` launch of the policy branch on device tensors.  ``given_action`` None: the net ACTS -- ``state`` is
        a contiguous float32 CUDA [n, 2 * hidden] tensor (c | h), or None for the policy's own state; its rows are zeroed where
        ``mask`` (the done flags of the previous step) is set and then advanced IN PLACE; the action is the mean
        (``deterministic``) or mean + exp(logstd) * ``noise`` (explicit contiguous float32 CUDA [n, ac_dim] rows; None: drawn from
        ``self.gen``).  With ``given_action`` the net SCORES it: one cell evaluation from a zero state (a scratch buffer zeroed
        for every call), no state is written, ``state`` / ``mask`` / ``noise`` are not read.  Returns dict(action, neglogp);
        ``out`` may hold preallocated outputs."""
        import ctypes as C
        t = self._t
        x, _ = self._obs(obs)
        n, A, H = x.shape[0], self.ac_dim, self.hidden
        out = out or {}
        action, neglogp = out.get("action"), out.get("neglogp")
        if action is None:
            action = t.empty((n, A), dtype=t.float32, device=self.device)
        if neglogp is None:
            neglogp = t.empty(n, dtype=t.float32, device=self.device)
        given = None
        if given_action is not None:
            given = given_action if t.is_tensor(given_action) else t.from_numpy(np.ascontiguousarray(given_action, np.float32))
            given = given.to(self.device, t.float32).reshape(n, A).contiguous()
            # a fresh zero state per call, allocated on the current stream: the kernel writes its new state there, and the env
            # groups of a Runner score on streams of their own (one cached buffer would be shared between them)
            zero = t.zeros((n, 2 * H), dtype=t.float32, device=self.device)
            cptr, hptr, stride, mask, noise = zero.data_ptr(), zero.data_ptr() + 4 * H, 2 * H, None, None
        else:
            if state is None:
                st = self._own_state(n)
                cptr, hptr, stride = st[2].data_ptr(), st[3].data_ptr(), H
            else:
                if tuple(state.shape) != (n, 2 * H) or state.dtype != t.float32 or not state.is_cuda or not state.is_contiguous():
                    raise ValueError("state must be a contiguous float32 CUDA tensor of shape (%d, %d)" % (n, 2 * H))
                cptr, hptr, stride = state.data_ptr(), state.data_ptr() + 4 * H, 2 * H
            mask = self._mask(mask, n)
            if deterministic:
                noise = None
            elif noise is None:
                noise = t.randn((n, A), generator=self.gen, device=self.device, dtype=t.float32)
            elif tuple(noise.shape) != (n, A) or noise.dtype != t.float32 or not noise.is_cuda or not noise.is_contiguous():
                raise ValueError("noise must be a contiguous float32 CUDA tensor of shape (%d, %d)" % (n, A))
        ppo_capi.chk(ppo_capi.lib().ppo_lstm_step(C.byref(self._nets["p"]), x.data_ptr(), n, x.stride(0) if n > 1 else x.shape[1],
                                                  ppo_capi.ptr(mask), cptr, hptr, stride, ppo_capi.ptr(noise), ppo_capi.ptr(given),
                                                  action.data_ptr(), neglogp.data_ptr(), None, None,
                                                  t.cuda.current_stream(self.device).cuda_stream))
        return dict(action=action, neglogp=neglogp)

    def step(self, observation, S=None, M=None, deterministic=False, noise=None, **extra_feed):
        """(action, None, S, neglogp): the net acts on ``observation`` from the state ``S`` (None: its own) masked by ``M``.  The value
        slot is None -- fix mode values agent 1 with the learner, and the value branch is a second cell (:meth:`value`)."""
        x, np_in = self._obs(observation)
        r = self.evaluate(x, state=S, mask=M, deterministic=deterministic, noise=noise)
        ret = (lambda z: z.cpu().numpy()) if np_in else (lambda z: z)
        return ret(r["action"]), None, S, ret(r["neglogp"])

    def value(self, ob, S=None, M=None, **kwargs):
        """The value branch on the policy's own value state (masked by ``M``, advanced), de-normalised with the return filter, as
        ``act(want_value=True)`` computes it.  Kept for the model interface: fix mode never reads it."""
        import ctypes as C
        t = self._t
        x, np_in = self._obs(ob)
        n, H = x.shape[0], self.hidden
        st = self._own_state(n)
        value = t.empty(n, dtype=t.float32, device=self.device)
        ppo_capi.chk(ppo_capi.lib().ppo_lstm_step(C.byref(self._nets["v"]), x.data_ptr(), n, x.stride(0) if n > 1 else x.shape[1],
                                                  ppo_capi.ptr(self._mask(M, n)), st[0].data_ptr(), st[1].data_ptr(), H, None, None, None,
                                                  None, value.data_ptr(), None, t.cuda.current_stream(self.device).cuda_stream))
        value = value * self.ret_std + self.ret_mean
        return value.cpu().numpy() if np_in else value

    def action_probability(self, observation, given_action=None, **extra_feed):
        """-log pi(given_action | observation) from a zero state (the Runner's scoring calls feed no state)."""
        x, np_in = self._obs(observation)
        nlp = self.evaluate(x, given_action=given_action)["neglogp"]
        return nlp.cpu().numpy() if np_in else nlp


def load_zoo_policy(path, ac_dim, device=0, kind=None):
    """utils.py:66-67 ``load_params`` + policy construction; ``kind`` 'mlp' / 'lstm' (default: whichever layout fits the
    vector length)."""
    return load_zoo_policy_from_flat(np.load(path, allow_pickle=False), ac_dim, device=device, kind=kind)


def load_zoo_policy_from_flat(flat, ac_dim, device=0, kind=None):
    """The policy for a flat parameter vector already in memory (utils.py:70-83 ``set_from_flat``)."""
    if kind is None:
        try:
            infer_ob_dim(flat.size, ac_dim)
            kind = "mlp"
        except ValueError:
            kind = "lstm"
    if kind == "lstm":
        return ZooLSTMPolicy(flat, ac_dim, device=device)
    return ZooMLPPolicy(flat, ac_dim, device=device)


# ---- leagues of zoo nets (learn(opponent_mode='fix', fix_opponent_path=[files])) ------------------------------------------------
LEAGUE_TILE = 16    # envs per tile: the granularity at which the fused launches select a table row (tile_net_dev / tile_entry_dev)


def league_plan(nmembers, nenvs, offset=0):
    """The member every 16-env tile of ``nenvs`` envs faces: int32 [nenvs / 16], tile t -> member (t + offset) % nmembers -- round
    robin over the tiles, ``offset`` the rotation (``learn`` passes update - 1: every member meets every env region over time).
    ``ValueError`` for an empty league, ``nenvs`` off the tile grid and fewer tiles than members (some member would not play)."""
    nmembers, nenvs = int(nmembers), int(nenvs)
    if nmembers < 1:
        raise ValueError("a league needs at least one zoo net (got %d)" % nmembers)
    if nenvs < LEAGUE_TILE or nenvs % LEAGUE_TILE:
        raise ValueError("a league deals its %d members over tiles of %d envs: nenvs = %d is not a multiple of %d"
                         % (nmembers, LEAGUE_TILE, nenvs, LEAGUE_TILE))
    ntiles = nenvs // LEAGUE_TILE
    if ntiles < nmembers:
        raise ValueError("a league of %d members needs at least as many 16-env tiles: nenvs = %d gives %d" % (nmembers, nenvs, ntiles))
    return ((np.arange(ntiles, dtype=np.int64) + int(offset)) % nmembers).astype(np.int32)


def league_entries(kinds):
    """Table entry of every member of a league whose families are ``kinds`` ('mlp' / 'lstm', in file order), in the encoding of
    include/sumo_hip.h ``sumo_zoo_league``: the MLP members take [0, nmlp) in their order, the LSTM members [nmlp, nmlp + nlstm) in
    theirs.  Returns (entries int32 [n], nmlp, nlstm)."""
    kinds = list(kinds)
    if any(k not in ("mlp", "lstm") for k in kinds):
        raise ValueError("league families are 'mlp' / 'lstm', got %r" % (kinds,))
    nmlp = sum(k == "mlp" for k in kinds)
    seen = {"mlp": 0, "lstm": 0}
    out = []
    for k in kinds:
        out.append(seen[k] + (nmlp if k == "lstm" else 0))
        seen[k] += 1
    return np.asarray(out, np.int32), nmlp, len(kinds) - nmlp


def league_scores(ep_done, ep_r, ep_l, tile_member, nmembers, timestep_limit=500):
    """Per-member tally of agent 0's finished episodes of one rollout, from the episode records ``Runner.run`` reads back
    (``ep_done`` bool / ``ep_r`` / ``ep_l`` [T][N], numpy) and the update's tile assignment (``tile_member`` [N / 16]): int64
    [nmembers][4] = episodes, learner wins, losses, draws -- an ESTIMATE, a training diagnostic and no evaluator (eval_against_fix.py
    reads the winner flags).  The record carries no winner flag, so the outcome is read from the
    episode itself (sumo.py:147-186): longer than ``timestep_limit`` steps = the -1000 timeout, a draw; otherwise the return holds
    the +2000 / -2000 main reward next to the dense shaping sum (about -1 to -5 per step), and the episode counts as a win if the
    return is above -1000 and as a loss otherwise.  Known misreadings: a double fall or a diverged episode (main reward 0) counts as
    a win, a win after hundreds of steps of strongly negative shaping can fall below -1000 and count as a loss, a fall in the very
    step after the time limit counts as a draw."""
    d = np.asarray(ep_done).astype(bool)
    r, l = np.asarray(ep_r, np.float64), np.asarray(ep_l)
    member = np.repeat(np.asarray(tile_member, np.int64), LEAGUE_TILE)
    if d.ndim != 2 or member.shape[0] != d.shape[1]:
        raise ValueError("episode records [T][N] and %d tiles of %d envs do not match" % (len(tile_member), LEAGUE_TILE))
    out = np.zeros((int(nmembers), 4), np.int64)
    _, env = np.nonzero(d)
    m = member[env]
    draw = l[d] > timestep_limit
    win = ~draw & (r[d] > -1000.0)
    for k, sel in enumerate((np.ones_like(draw), win, ~draw & ~win, draw)):
        np.add.at(out[:, k], m[sel], 1)
    return out


class ZooLeague(object):
    """A league of zoo nets, MLP and LSTM mixed, as agent 1 of a device-mode ``Runner`` (inside a :class:`FixedOpponentModel`):
    every 16-env tile of the whole env set faces one member (:func:`league_plan`, re-dealt by :meth:`assign`).  Holds the members
    (:class:`ZooMLPPolicy` / :class:`ZooLSTMPolicy`, file order), a :class:`ZooTable` of the MLP members and a
    :class:`ZooLstmTable` of the LSTM members (None where the league has none of that family), each member's table entry
    (:func:`league_entries`), the per-tile entries on the device (``tile_entry`` int32 [N / 16], and ``env_entry`` [N], the same
    per env), ONE noise generator for agent 1's action noise of the whole league and the zoo LSTM state ``state`` [N][128] (c | h;
    only envs on LSTM tiles use their rows; a row is zeroed when its tile changes member).

    :meth:`act` / :meth:`score` are the step-by-step definition of what the fused league launches compute: each member's rows are
    gathered, evaluated exactly as a single zoo net is, and scattered back."""

    recurrent = False
    initial_state = None

    def __init__(self, members, nenvs, device=0):
        import torch
        self._t = torch
        self.device = torch.device("cuda", int(device)) if not isinstance(device, torch.device) else device
        self.members = list(members)
        if any(type(m) not in (ZooMLPPolicy, ZooLSTMPolicy) for m in self.members):
            raise ValueError("league members are ZooMLPPolicy / ZooLSTMPolicy objects")
        if any(type(m) is ZooLSTMPolicy and not (m.emb == m.hidden == HIDDEN) for m in self.members):
            raise ValueError("the LSTM members of a league have embedding and cell of %d (the league keeps one [N][%d] state for all of them)"
                             % (HIDDEN, 2 * HIDDEN))
        self.num_envs = int(nenvs)
        league_plan(len(self.members), self.num_envs)                 # the size checks, before anything is uploaded
        self.kinds = ["lstm" if type(m) is ZooLSTMPolicy else "mlp" for m in self.members]
        self.entries, self.nmlp, self.nlstm = league_entries(self.kinds)
        self.ac_dim = self.members[0].ac_dim
        if len({m.ac_dim for m in self.members}) != 1 or len({m.ob_dim for m in self.members}) != 1:
            raise ValueError("the members of a league share ob_dim and ac_dim")
        self.ob_dim = self.members[0].ob_dim
        mlp = [m for m in self.members if type(m) is ZooMLPPolicy]
        lstm = [m for m in self.members if type(m) is ZooLSTMPolicy]
        self.mlp_table = ZooTable(mlp, self.ac_dim, self.device) if mlp else None
        self.lstm_table = ZooLstmTable(lstm, self.ac_dim, self.device) if lstm else None
        self.gen = torch.Generator(device=self.device)
        self.state = torch.zeros((self.num_envs, 2 * HIDDEN), dtype=torch.float32, device=self.device)
        self.tile_member = None
        self.assign(0)

    def seed(self, s):
        self.gen.manual_seed(int(s))

    def reset(self, **kwargs):
        self.state.zero_()

    def assign(self, offset):
        """Deal the members over the tiles with rotation ``offset`` (:func:`league_plan`); the state rows of tiles that change
        member are zeroed."""
        t = self._t
        plan = league_plan(len(self.members), self.num_envs, offset)
        if self.tile_member is not None:
            changed = np.repeat(plan != self.tile_member, LEAGUE_TILE)
            if changed.any():
                self.state[t.from_numpy(changed).to(self.device)] = 0.0
        self.tile_member = plan
        self.tile_entry = t.from_numpy(self.entries[plan]).to(self.device)
        self.env_entry = self.tile_entry.repeat_interleave(LEAGUE_TILE).contiguous()
        env_member = np.repeat(plan, LEAGUE_TILE)
        self._member_envs = [np.nonzero(env_member == k)[0] for k in range(len(self.members))]
        self._rows = {}

    def member_rows(self, first_env, n):
        """[(member, device int64 rows relative to ``first_env``)] for the members that play envs [first_env, first_env + n)."""
        key = (int(first_env), int(n))
        if key not in self._rows:
            out = []
            for k, envs in enumerate(self._member_envs):
                sel = envs[(envs >= key[0]) & (envs < key[0] + key[1])] - key[0]
                if sel.size:
                    out.append((self.members[k], self._t.from_numpy(sel.astype(np.int64)).to(self.device)))
            self._rows[key] = out
        return self._rows[key]

    def struct(self, state):
        """The ``capi.ZooLeague`` launch struct of a mixed league with the state rows ``state`` of the launch's envs."""
        from . import capi
        if self.mlp_table is None or self.lstm_table is None:
            raise ValueError("the league launch plays MLP and LSTM members side by side; a league of one family plays through that "
                             "family's launch")
        z = capi.ZooLeague()
        z.mlp, z.lstm, z.tile_entry_dev = self.mlp_table.struct(), self.lstm_table.struct(state), self.tile_entry.data_ptr()
        return z

    def act(self, obs, done, first_env, noise, action, neglogp):
        """Agent 1's step of envs [first_env, first_env + n): every member acts on its rows of ``obs`` [n, >= ob_dim] with its rows
        of ``noise`` [n, A] -- an MLP member through ``ppo_forward_filtered`` with the tanh trunk, an LSTM member from its rows of
        ``self.state``, masked by ``done`` [n] (agent 1's flags of the previous step) and advanced -- into ``action`` / ``neglogp``."""
        n = obs.shape[0]
        for m, rows in self.member_rows(first_env, n):
            o, nz = obs[rows], noise[rows].contiguous()
            if type(m) is ZooLSTMPolicy:
                st = self.state[first_env + rows]
                r = m.evaluate(o, state=st, mask=done[rows], noise=nz)
                self.state[first_env + rows] = st
            else:
                r = m.evaluate(o, ppo_capi.FWD_PI, noise=nz)
            action[rows] = r["action"]
            neglogp[rows] = r["neglogp"]

    def score(self, obs, given_action, first_env, neglogp):
        """Every member's -log pi(given_action | obs) on its rows (an LSTM member: from a zero state, nothing written)."""
        n = obs.shape[0]
        for m, rows in self.member_rows(first_env, n):
            if type(m) is ZooLSTMPolicy:
                r = m.evaluate(obs[rows], given_action=given_action[rows])
            else:
                r = m.evaluate(obs[rows], ppo_capi.FWD_PI, given_action=given_action[rows])
            neglogp[rows] = r["neglogp"]

    def evaluate(self, obs, flags=None, given_action=None, noise=None, out=None, first_env=0, mask=None):
        """The policies' ``evaluate`` on device rows of envs [first_env, first_env + n) (what makes a device-mode ``Runner`` of an MLP
        learner accept the league): :meth:`score` with ``given_action``, else :meth:`act` (``noise`` None: drawn from ``self.gen``;
        ``mask`` None: no state row is zeroed).  Returns dict(action, neglogp); ``out`` may hold preallocated outputs."""
        t = self._t
        n, out = obs.shape[0], out or {}
        neglogp = out.get("neglogp")
        if neglogp is None:
            neglogp = t.empty(n, dtype=t.float32, device=self.device)
        if given_action is not None:
            self.score(obs, given_action, first_env, neglogp)
            return dict(action=given_action, neglogp=neglogp)
        action = out.get("action")
        if action is None:
            action = t.empty((n, self.ac_dim), dtype=t.float32, device=self.device)
        if noise is None:
            noise = t.randn((n, self.ac_dim), generator=self.gen, device=self.device, dtype=t.float32)
        if mask is None:
            mask = t.zeros(n, dtype=t.uint8, device=self.device)
        self.act(obs, mask, first_env, noise, action, neglogp)
        return dict(action=action, neglogp=neglogp)

    # ---- model surface (FixedOpponentModel): whole env set, host or device arrays -----------------------------------------------
    def _dev(self, x):
        t = self._t
        np_in = not t.is_tensor(x)
        if np_in:
            x = t.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(self.device)
        return x, np_in

    def step(self, observation, S=None, M=None, **extra_feed):
        """(action, None, None, neglogp) for the whole env set: every member acts on its tiles (host arrays in, host arrays out)."""
        t = self._t
        x, np_in = self._dev(observation)
        if x.shape[0] != self.num_envs:
            raise ValueError("a league steps its whole env set (%d envs), got %d rows" % (self.num_envs, x.shape[0]))
        mask = None if M is None else (M if t.is_tensor(M) else t.from_numpy(np.ascontiguousarray(np.asarray(M).reshape(-1), np.uint8)).to(self.device))
        r = self.evaluate(x, mask=mask)
        ret = (lambda z: z.cpu().numpy()) if np_in else (lambda z: z)
        return ret(r["action"]), None, None, ret(r["neglogp"])

    def value(self, ob, *args, **kwargs):
        raise NotImplementedError("fix mode values agent 1 with the learner; a league has no value of its own")

    def action_probability(self, observation, given_action=None, **extra_feed):
        x, np_in = self._dev(observation)
        nlp = self.evaluate(x, given_action=self._dev(given_action)[0].reshape(x.shape[0], self.ac_dim))["neglogp"]
        return nlp.cpu().numpy() if np_in else nlp


def load_zoo_league(paths, ac_dim, nenvs, device=0):
    """A :class:`ZooLeague` from a sequence of ``.npy`` files (the family of each is read from its length, as :func:`load_zoo_policy`
    reads it)."""
    paths = list(paths)
    if not paths:
        raise ValueError("a league needs at least one zoo net (got 0 files)")
    league_plan(len(paths), nenvs)
    return ZooLeague([load_zoo_policy(p, ac_dim, device=device) for p in paths], nenvs, device=device)


class FixedOpponentModel(object):
    """What alg_ppo.py:194-206 puts into ``runner.models[1]`` in ``opponent_mode='fix'``: a non-trainable model whose
    ``step`` / ``value`` / ``act_model.action_probability`` come from the zoo net (either family)."""

    trainable = False

    def __init__(self, policy):
        self.act_model = self.train_model = policy
        self.initial_state = None
        self.step = policy.step
        self.value = policy.value

    def load(self, path):
        raise RuntimeError("the fixed opponent is not replaced by checkpoints")


EVAL_ADJUST_Z = -0.5   # eval_robosumo_against_fix.py:108-115, play_fixed.py:23, compare_history_version.py:74


def evaluate_against(model, opponent, env, rounds, deterministic=True, adjust_z=EVAL_ADJUST_Z):
    """eval_robosumo_against_fix.py:196-230 on the device: ``model`` acts for agent 0 on obs[:, 0], ``opponent`` (zoo
    policy) for agent 1 on obs[:, 1, :ob_dim]; an episode counts as a win if agent 0 carries the 'winner' flag when it
    ends, a loss if agent 1 does, a draw otherwise.  Returns dict(win, draw, lose, rounds, steps).

    The reference's evaluator builds its envs with ``agent._adjust_z = -0.5`` on every agent (:108-115): observed heights
    and the lose test (sumo.py:147-160: ``z + adjust_z < 0.29``) are relative to a tatami surface at z = 0, which is what
    the zoo nets were trained on.  ``adjust_z`` is imposed on ``env`` for the evaluation and the env's own value restored
    afterwards (None: leave the env as it is)."""
    import torch
    prev_adjust = getattr(env, "adjust_z", 0.0)
    if adjust_z is not None and float(adjust_z) != prev_adjust:
        env.set_adjust_z(adjust_z)
    try:
        return _evaluate_against(model, opponent, env, rounds, deterministic)
    finally:
        if adjust_z is not None and float(adjust_z) != prev_adjust:
            torch.cuda.synchronize()
            env.set_adjust_z(prev_adjust)


def _evaluate_against(model, opponent, env, rounds, deterministic):
    import torch
    obs = env.reset_device()
    A0, A1 = env.model.act_dims
    D0 = env.model.obs_dims[0]
    acts = torch.zeros_like(env.act_dev)
    win = draw = lose = done_rounds = steps = 0
    while done_rounds < rounds:
        a0 = model.step(obs[:, 0, :D0], deterministic=deterministic)[0]
        a1 = opponent.act(obs[:, 1, :], stochastic=not deterministic)[0]
        acts[:, 0, :A0] = a0
        acts[:, 1, :A1] = a1
        obs, info, done, _, _, _ = env.step_device(acts)
        steps += 1
        fin = done[:, 0] != 0
        nfin = int(fin.sum())
        if nfin and getattr(opponent, "recurrent", False):
            opponent.reset(fin)
        if nfin:
            flags = info[:, :, 7].to(torch.int64)
            w0 = ((flags[:, 0] & 1) != 0) & fin
            w1 = ((flags[:, 1] & 1) != 0) & fin & ~w0
            nw, nl = int(w0.sum()), int(w1.sum())
            win += nw; lose += nl; draw += nfin - nw - nl
            done_rounds += nfin
    return dict(win=win / done_rounds, draw=draw / done_rounds, lose=lose / done_rounds, rounds=done_rounds, steps=steps)
