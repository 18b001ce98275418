"""Fine-tune a policy-zoo MLP net with PPO: ``learn(network='zoo_mlp', zoo_init=<file>)``.

The learner IS a zoo net (robosumo/robosumo/policy_zoo/policy.py:23-91): tanh 64-64 policy and value trunks, state-independent
logstd, the running-mean observation filter clipped to +-5 and the value de-normalised by the return filter.  Its kernel layout
(``policy_zoo.zoo_kernel_flat``) is the flat layout of ``PPOModel``, so the slab reduction, ``ppo_clip_adam``, the HIP-graph step and
the loss statistics are inherited; what differs is the gradient launch (``ppo_grad_act`` with ``PPO_GRAD_TANH`` and the value affine)
and the observation filter, applied once per update to the batch copy the model owns (``ppo_obs_filter``).

Both filters are FROZEN, like the reference's zoo nets at play time: a checkpoint is the zoo's flat ``.npy`` vector with the six
filter entries of the source file byte for byte and the thirteen trained tensors from ``params`` -- every zoo path (``ZooMLPPolicy``,
``ZooTable``, ``ppo_capi.ZooSeat``, leagues, ``zoo_tournament.py``, the reference's ``demos/play.py``) plays it unchanged.
"""
import os

import numpy as np

from . import mixed, policy_zoo, ppo_capi
from .model import PPOModel
from .policies import PARAM_NAMES, param_shapes, unflatten_params

OBS_CLIP = 5.0            # policy.py:47
_FILTER_KEYS = policy_zoo._ZOO_MLP_ORDER[:6]
# the 13 tensors of PARAM_NAMES (the kernel's flat order) under their zoo names
_TRAINED_KEYS = ["polfc1/w", "polfc1/b", "polfc2/w", "polfc2/b", "vffc1/w", "vffc1/b", "vffc2/w", "vffc2/b", "polfinal/w", "polfinal/b",
                 "logstd", "vffinal/w", "vffinal/b"]
assert sorted(_FILTER_KEYS + _TRAINED_KEYS) == sorted(policy_zoo._ZOO_MLP_ORDER) and len(_TRAINED_KEYS) == len(PARAM_NAMES)


def read_zoo_vector(src):
    """The flat float32 vector of ``src``: a ``.npy`` path (``allow_pickle=False``) or a vector."""
    if isinstance(src, (str, os.PathLike)):
        with open(os.path.expanduser(str(src)), "rb") as f:
            src = np.load(f, allow_pickle=False)
    return np.asarray(src, np.float32).ravel().copy()


def zoo_vector(tensors):
    """The zoo's flat vector (``_ZOO_MLP_ORDER``) of a dict of its tensors: the inverse of ``policy_zoo.split_zoo_mlp``."""
    return np.concatenate([np.asarray(tensors[k], np.float32).ravel() for k in policy_zoo._ZOO_MLP_ORDER])


def write_zoo_vector(path, flat):
    """``numpy.save`` to an open file: the name is kept as given (a checkpoint is ``00007``, not ``00007.npy``)."""
    dirname = os.path.dirname(path)
    if dirname:
        os.makedirs(dirname, exist_ok=True)
    with open(path, "wb") as f:
        np.save(f, np.asarray(flat, np.float32), allow_pickle=False)


class ZooMlpSpec(object):
    """What ``build_policy(env, 'zoo_mlp', zoo_init=...)`` returns: the source net split by ``split_zoo_mlp`` (``tensors``), its widths
    (``ob_dim``: the env's observation width without the trailing time feature, 120 / 164 / 208), the observation filter's
    mean / std and the return filter's mean / std (float32, as ``policy_zoo.filter_stats`` gives them)."""

    network = "zoo_mlp"

    def __init__(self, env_ob_dim, ac_dim, zoo_init):
        if zoo_init is None:
            raise ValueError("network='zoo_mlp' needs zoo_init=<policy_zoo .npy file or flat vector>: the net to fine-tune")
        self.env_ob_dim, self.ac_dim = int(env_ob_dim), int(ac_dim)
        self.source = str(zoo_init) if isinstance(zoo_init, (str, os.PathLike)) else None
        flat = read_zoo_vector(zoo_init)
        name = self.source or "the zoo_init vector"
        try:
            kind = policy_zoo.zoo_file_kind(flat.size, self.ac_dim)
        except ValueError:
            raise ValueError("zoo_init: %s (%d parameters) fits no policy-zoo net with %d actions: a net of another species?"
                             % (name, flat.size, self.ac_dim))
        if kind == "lstm":
            raise NotImplementedError("zoo_init: %s is a zoo LSTM policy; network='zoo_mlp' fine-tunes zoo MLP nets only (zoo LSTM learners "
                                      "are not built)" % name)
        self.ob_dim, self.tensors = policy_zoo.split_zoo_mlp(flat, self.ac_dim)
        if self.ob_dim != self.env_ob_dim - 1:
            raise ValueError("zoo_init: %s reads %d observation columns, this env gives %d plus the time feature: a net of another "
                             "species" % (name, self.ob_dim, self.env_ob_dim - 1))
        self.flat = flat
        self.obs_mean, self.obs_std = policy_zoo.filter_stats(self.tensors, "obsfilter")
        self.ret_mean, self.ret_std = [float(x) for x in policy_zoo.filter_stats(self.tensors, "retfilter")]

    def filter_bytes(self):
        return b"".join(np.asarray(self.tensors[k], np.float32).tobytes() for k in _FILTER_KEYS)


class ZooActPolicy(policy_zoo.ZooMLPPolicy):
    """A ``ZooMLPPolicy`` whose kernel parameters are the learner's own ``params`` tensor: the evaluation is
    ``ZooMLPPolicy.evaluate`` itself (the ``ppo_forward_filtered`` launch and the value de-normalisation), on weights that train."""

    def __init__(self, spec, params, device):
        super().__init__(spec.flat, spec.ac_dim, device=device)
        assert params.numel() == self.params.numel()
        self.spec = spec
        self.params = params


def check_learn(env, *, opponent_mode, opponent_pool, fused_selector, fused_fix_opponent, eval_interval, eval_opponents, comm, resume,
                resume_interval, load_path, zoo_init):
    """What ``alg_ppo.learn(network='zoo_mlp')`` refuses, each with its own message, before anything touches the device."""
    pre = "network='zoo_mlp': "
    if opponent_mode == "ours":
        raise NotImplementedError(pre + "opponent_mode='ours' is not available (its selector scores relu MLP(64,64) checkpoints); use "
                                  "'latest', 'random' or 'fix'")
    if int(opponent_pool) > 1:
        raise NotImplementedError(pre + "opponent_pool > 1 is not available (the pool plays inside the fused rollout launch, which holds "
                                  "no zoo-architecture learner)")
    if fused_selector:
        raise NotImplementedError(pre + "fused_selector serves opponent_mode='ours', which this learner does not run")
    if fused_fix_opponent:
        raise NotImplementedError(pre + "fused_fix_opponent is not available: the zoo-architecture learner plays step by step, not inside "
                                  "the engine's fused launches")
    if eval_interval or eval_opponents:
        raise NotImplementedError(pre + "eval_interval / eval_opponents are not available (the evaluator's fused matches take relu MLP and "
                                  "LSTM learners); the checkpoints are zoo files, play them with zoo_tournament.py")
    if comm is not None:
        raise NotImplementedError(pre + "runs on a single GPU (no comm)")
    if resume or resume_interval:
        raise NotImplementedError(pre + "resume / resume_interval are not available (the resume state knows joblib checkpoints)")
    if mixed.is_mixed(env):
        D, A = env.model.obs_dims, env.model.act_dims
        raise NotImplementedError(pre + "not available on a mixed match-up (observations %d / %d, actions %d / %d): homogeneous scenes only"
                                  % (D[0], D[1], A[0], A[1]))
    if zoo_init is None:
        raise ValueError("network='zoo_mlp' needs zoo_init=<policy_zoo .npy file or flat vector>: the net to fine-tune")
    if load_path is not None:
        a, b = read_zoo_vector(load_path).size, read_zoo_vector(zoo_init).size
        if a != b:
            raise ValueError(pre + "load_path %s holds %d parameters, zoo_init %d: a net of another species" % (load_path, a, b))


class ZooPPOModel(PPOModel):
    """``PPOModel`` for a zoo-architecture net (``policy`` is a :class:`ZooMlpSpec`).  ``params`` starts as the kernel layout of the
    source file and nothing is drawn from numpy's stream."""

    recurrent = False
    graph_noun = "zoo PPO"

    def __init__(self, *, policy, ob_space=None, ac_space=None, nbatch_act=None, nbatch_train=None, nsteps=None, ent_coef=0.0,
                 vf_coef=0.5, max_grad_norm=0.5, microbatch_size=None, trainable=True, model_scope="", device=0, comm=None):
        if comm is not None:
            raise NotImplementedError("network='zoo_mlp': runs on a single GPU (no comm)")
        if not isinstance(policy, ZooMlpSpec):
            raise TypeError("ZooPPOModel needs a ZooMlpSpec (build_policy(env, 'zoo_mlp', zoo_init=...))")
        rng_state = np.random.get_state()
        super().__init__(policy=policy, ob_space=ob_space, ac_space=ac_space, nbatch_act=nbatch_act, nbatch_train=nbatch_train,
                         nsteps=nsteps, ent_coef=ent_coef, vf_coef=vf_coef, max_grad_norm=max_grad_norm, microbatch_size=microbatch_size,
                         trainable=trainable, model_scope=model_scope, device=device, comm=None)
        np.random.set_state(rng_state)                                   # the base constructor's orthogonal init is not this net's
        t = self._t
        self.params.copy_(t.from_numpy(policy_zoo.zoo_kernel_flat(policy.tensors)))
        self.act_model = ZooActPolicy(policy, self.params, self.device)
        self.train_model = self.act_model
        self.step, self.value = self.act_model.step, self.act_model.value
        self.obs_mean, self.obs_invstd = self.act_model.obs_mean, self.act_model.obs_invstd

    # ---- the observation filter: once per update on the model's own copy, or on what the eager path is given ----------------
    def _filter(self, src, dst):
        st = self._t.cuda.current_stream(self.device).cuda_stream
        ppo_capi.chk(ppo_capi.lib().ppo_obs_filter(src.data_ptr(), src.shape[0], src.stride(0), self.spec.ob_dim, self.obs_mean.data_ptr(),
                                                   self.obs_invstd.data_ptr(), OBS_CLIP, dst.data_ptr(), dst.stride(0), st))
        return dst

    def _check_obs(self, obs):
        if obs.dim() != 2 or obs.shape[1] < self.spec.ob_dim or obs.stride(1) != 1:
            raise ValueError("expected [n, >=%d] observations with unit inner stride" % self.spec.ob_dim)

    def begin_update(self, obs, returns, actions, values, neglogpacs, weights):
        self._check_obs(obs)
        super().begin_update(obs, returns, actions, values, neglogpacs, weights)
        buf = self._static["bufs"][0]
        self._filter(buf, buf)

    def train(self, lr, cliprange, obs, returns, masks, actions, values, neglogpacs, rewards, IS_weight, states=None):
        t = self._t
        np_in = not t.is_tensor(obs)
        obs = self._dev(obs, np.float32)
        self._check_obs(obs)
        obs = self._filter(obs, t.empty((obs.shape[0], self.spec.ob_dim), dtype=t.float32, device=self.device))
        ret, val = self._dev(returns, np.float32), self._dev(values, np.float32)
        act, old, w = self._dev(actions, np.float32), self._dev(neglogpacs, np.float32), self._dev(IS_weight, np.float32)
        out = PPOModel.train_indexed(self, lr, cliprange, obs, ret, act, val, old, w, None, obs.shape[0])
        stats = out[:5]
        if np_in:
            return [np.float32(s) for s in stats] + [out[5].cpu().numpy(), None]
        return list(stats) + [out[5], None]

    def train_indexed(self, lr, cliprange, obs, returns, actions, values, neglogpacs, weights, idx, n, sync=True, mb_index=None):
        """Rows of the ``begin_update`` batch (filtered there).  Without an open update the rows given would reach the gradient kernel
        unfiltered: that is ``train``'s job."""
        if self._static is None or not self._static["open"]:
            raise RuntimeError("ZooPPOModel.train_indexed needs begin_update() (it filters the batch); train() takes raw observations")
        obs = self._static["bufs"][0]
        return super().train_indexed(lr, cliprange, obs, returns, actions, values, neglogpacs, weights, idx, n, sync=sync, mb_index=mb_index)

    def _launch_loss_grad(self, obs, returns, actions, values, neglogpacs, weights, idx, n, cliprange, adv, log_ratio, st, mom=None):
        """``PPOModel._launch_loss_grad`` with the gradient launch swapped; ``obs`` rows are already filtered."""
        L = ppo_capi.lib()
        ip = ppo_capi.ptr(idx)
        mom = self.moments
        ppo_capi.chk(L.ppo_adv_moments_ws(returns.data_ptr(), values.data_ptr(), ip, n, mom.data_ptr(), self.adv_ws.data_ptr(), st))
        ppo_capi.chk(L.ppo_adv_normalize(returns.data_ptr(), values.data_ptr(), ip, n, mom.data_ptr(), adv.data_ptr(), st))
        self.stats.zero_()
        ppo_capi.chk(L.ppo_grad_act(self.params.data_ptr(), obs.data_ptr(), obs.stride(0), self.spec.ob_dim, self.spec.ac_dim,
                                    actions.data_ptr(), adv.data_ptr(), returns.data_ptr(), neglogpacs.data_ptr(), weights.data_ptr(), ip, n,
                                    1.0 / float(n), float(cliprange), self.ent_coef, self.vf_coef, ppo_capi.GRAD_TANH, self.spec.ret_std,
                                    self.spec.ret_mean, self.grads.data_ptr(), self.stats.data_ptr(), log_ratio.data_ptr(),
                                    self.workspace.data_ptr(), st))

    # ---- checkpoints are zoo files ---------------------------------------------------------------------------------------------
    def get_param_list(self):
        return unflatten_params(self.params.cpu().numpy(), self.spec.ob_dim, self.spec.ac_dim)

    def set_param_list(self, plist):
        shapes = param_shapes(self.spec.ob_dim, self.spec.ac_dim)
        assert len(plist) == len(shapes), "number of variables loaded mismatches len(variables)"
        for p, s in zip(plist, shapes):
            if tuple(np.shape(p)) != tuple(s):
                raise ValueError("checkpoint tensor shape %s does not match %s" % (np.shape(p), s))
        self.params.copy_(self._t.from_numpy(np.concatenate([np.asarray(p, np.float32).ravel() for p in plist])))

    def zoo_flat(self):
        """The model as the zoo's flat vector: the source file's filter entries, the trained tensors from ``params``."""
        tensors = dict((k, self.spec.tensors[k]) for k in _FILTER_KEYS)
        tensors.update(zip(_TRAINED_KEYS, self.get_param_list()))
        return zoo_vector(tensors)

    def save(self, save_path):
        write_zoo_vector(save_path, self.zoo_flat())

    def load(self, load_path):
        flat = read_zoo_vector(load_path)
        if flat.size != self.spec.flat.size:
            raise ValueError("%s holds %d parameters, this model %d: a net of another species or family" % (load_path, flat.size, self.spec.flat.size))
        _, p = policy_zoo.split_zoo_mlp(flat, self.spec.ac_dim)
        if b"".join(np.asarray(p[k], np.float32).tobytes() for k in _FILTER_KEYS) != self.spec.filter_bytes():
            raise ValueError("%s carries other filter statistics than this model's zoo_init: the filters are frozen, and the opponent copy "
                             "and the scratch model share the learner's" % load_path)
        self.set_param_list([p[k] for k in _TRAINED_KEYS])
