"""``ActorCriticModel`` on the HIP kernels: the reference's A2C learner (model.py:216-372) with the same constructor keywords,
``train`` signature and ``loss_names``.

Parameters, ``act_model`` (the rollout policy), checkpoints and the Adam state are ``PPOModel``'s: the two learners share the network
(MLP(64, 64) trunks, copy value network) and the on-disk format, so PPO and A2C checkpoints load into each other.  Only the loss
differs (model.py:257-310): pg = mean(w * adv * neglogp), vf = 0.5 * mean(w * (v - R)^2), no ratio, no clipping, the IS weight on
both terms.  One ``train`` call is one optimiser step on the whole batch:

    ppo_adv_moments_ws -> ppo_adv_normalize -> ppo_a2c_grad -> ppo_a2c_loss_stats   (one HIP graph, no host read-back)
    ppo_clip_adam                                                                    (outside: its step count is a host scalar)

Out of scope: recurrent policies and multi-GPU (``comm``) -- both raise ``NotImplementedError``."""
import numpy as np

from . import policies, ppo_capi
from .model import PPOModel


class ActorCriticModel(PPOModel):
    loss_names = ["policy_loss", "value_loss", "policy_entropy"]   # model.py:296
    graph_noun = "A2C"

    def __init__(self, *, policy, ob_space=None, ac_space=None, nbatch_act=None, nbatch_train=None, nsteps=None,
                 ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, microbatch_size=None, trainable=True, model_scope="",
                 device=0, comm=None):
        if not isinstance(policy, policies.PolicySpec):
            raise NotImplementedError("ActorCriticModel: only MLP policies; recurrent (lstm) policies are not supported with the A2C learner")
        if comm is not None and trainable:
            raise NotImplementedError("ActorCriticModel: multi-GPU training (comm) is not supported with the A2C learner")
        super().__init__(policy=policy, ob_space=ob_space, ac_space=ac_space, nbatch_act=nbatch_act, nbatch_train=nbatch_train,
                         nsteps=nsteps, ent_coef=ent_coef, vf_coef=vf_coef, max_grad_norm=max_grad_norm,
                         microbatch_size=microbatch_size, trainable=trainable, model_scope=model_scope, device=device, comm=None)
        if trainable:
            self._last_n = None       # batch size of the previous step (a size is captured the second time in a row it is seen)

    # ---- one optimiser step (model.py:348-372) -----------------------------------------------------------------
    def train(self, lr, obs, returns, masks, actions, values, neglogpacs, rewards, IS_weight, states=None):
        """``masks``, ``neglogpacs`` and ``rewards`` are accepted for the reference's signature; the loss does not use them
        (neglogp is re-evaluated by the gradient kernel; rewards only fed a TF summary).  Returns [pg_loss, vf_loss, entropy]
        (np.float32 for numpy inputs, floats otherwise)."""
        if states is not None:
            raise NotImplementedError("ActorCriticModel: recurrent states are not supported with the A2C learner")
        t = self._t
        np_in = not t.is_tensor(obs)
        obs = self._dev(obs, np.float32)
        ret, val = self._dev(returns, np.float32), self._dev(values, np.float32)
        act, w = self._dev(actions, np.float32), self._dev(IS_weight, np.float32)
        o = self.train_device(lr, obs, ret, act, val, w).cpu().numpy()
        return [np.float32(x) for x in o] if np_in else [float(x) for x in o]

    def train_device(self, lr, obs, returns, actions, values, IS_weight):
        """``train`` on device tensors without host read-back: returns the device float64 [3] tensor of the step's
        [pg_loss, vf_loss, entropy] (a fresh tensor per call)."""
        if not self.trainable:
            raise RuntimeError("model built with trainable=False")
        t = self._t
        if obs.dim() != 2 or obs.stride(1) != 1:
            raise ValueError("obs must be [n, ob_dim] with unit inner stride")
        n = int(obs.shape[0])
        for x in (returns, actions, values, IS_weight):
            if x.shape[0] != n or not x.is_contiguous() or x.dtype != t.float32 or x.device != self.device:
                raise ValueError("batch arrays must be contiguous float32 device tensors of %d rows" % n)
        if n == 0:
            raise ValueError("empty batch")
        st = t.cuda.current_stream(self.device).cuda_stream
        out3 = None
        if self.use_graph:
            out3 = self._graph_step(obs, returns, actions, values, IS_weight, n)
        if out3 is None:
            out3 = t.empty(3, dtype=t.float64, device=self.device)
            adv = t.empty(n, dtype=t.float32, device=self.device)
            self._launch_chain(obs, returns, actions, values, IS_weight, n, adv, out3, st)
        self._adam_step(lr, st)
        return out3.clone()

    def _launch_chain(self, obs, returns, actions, values, weights, n, adv, out3, st):
        """Advantages normalised over the whole batch (model.py:351-355), the A2C gradient, the loss statistics."""
        L = ppo_capi.lib()
        D, A = self.spec.ob_dim, self.spec.ac_dim
        self.stats.zero_()
        ppo_capi.chk(L.ppo_adv_moments_ws(returns.data_ptr(), values.data_ptr(), None, n, self.moments.data_ptr(), self.adv_ws.data_ptr(), st))
        ppo_capi.chk(L.ppo_adv_normalize(returns.data_ptr(), values.data_ptr(), None, n, self.moments.data_ptr(), adv.data_ptr(), st))
        ppo_capi.chk(L.ppo_a2c_grad(self.params.data_ptr(), obs.data_ptr(), obs.stride(0), D, A, actions.data_ptr(), adv.data_ptr(),
                                    returns.data_ptr(), weights.data_ptr(), None, n, 1.0 / float(n), self.ent_coef, self.vf_coef,
                                    self.grads.data_ptr(), self.stats.data_ptr(), self.workspace.data_ptr(), st))
        off = self.P - 1 - policies.HIDDEN - A                       # pi/logstd inside the flat parameter vector (checkpoint order)
        ppo_capi.chk(L.ppo_a2c_loss_stats(self.stats.data_ptr(), self.params.data_ptr() + 4 * off, A, out3.data_ptr(), st))

    def _graph_step(self, obs, returns, actions, values, weights, n):
        """The chain replayed from a HIP graph over batch buffers this model owns (the batch is copied in: five device copies per
        update).  A graph is captured for a batch size the second time in a row it is seen, so a run whose batch size changes every
        update (opponent-data reuse) stays on the eager launches instead of capturing per update.  Returns None = use the eager
        path."""
        t = self._t
        seen_before, self._last_n = self._last_n == n, n
        g = self._graphs.get(n)
        if g is None:
            if not seen_before:
                return None

            def make_record():
                bufs = [t.empty((n, obs.shape[1]), dtype=t.float32, device=self.device)] + [t.empty_like(x) for x in (returns, actions, values, weights)]
                for dst, x in zip(bufs, (obs, returns, actions, values, weights)):
                    dst.copy_(x)
                return dict(bufs=bufs, adv=t.empty(n, dtype=t.float32, device=self.device), out3=t.zeros(3, dtype=t.float64, device=self.device))

            def body(g):
                self._launch_chain(*g["bufs"], n, g["adv"], g["out3"], t.cuda.current_stream(self.device).cuda_stream)
            g = self._graphs.capture(n, make_record, body, lambda: setattr(type(self), "use_graph", False))
            if g is None:
                return None
        for dst, x in zip(g["bufs"], (obs, returns, actions, values, weights)):
            dst.copy_(x)
        g["graph"].replay()
        return g["out3"]
