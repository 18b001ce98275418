"""Recurrent PPO model: baselines ``lstm(nlstm)`` policy (shared latent, two heads) trained by back-propagation through
time on the HIP kernels.

Reference surfaces mirrored: ``PPOModel`` (model.py:9-213: ``step`` / ``value`` / ``train(..., states)`` / ``save`` /
``load``), the recurrent network builder baselines/baselines/common/models.py:131-183 + a2c/utils.py:82-103 and the
recurrent minibatch convention of baselines ppo2 (whole env sequences per minibatch, env-major flattening; the reference
fork's own copy of that loop, alg_ppo.py:408-421, passes the states as ``IS_weight`` and cannot run -- SURVEY.md App. C.3).

Kernels (include/sumo_ppo.h): ``ppo_lstm_step`` (acting), ``ppo_lstm_step_save`` (unrolled forward that records gates),
``ppo_lstm_head_grad`` (loss + head gradients on the stored latents), ``ppo_lstm_bwd_step`` (one BPTT step; nlstm = 128: the whole
sequence in one launch each way, ``ppo_lstm_seq_forward`` / ``ppo_lstm_seq_backward``), the weight gradients by the hand-written
split-K MFMA kernel ``ppo_lstm_wgrad`` (``SUMO_LSTM_WGRAD=blas`` keeps ``torch.matmul`` = hipBLASLt as a cross-check only) and
``ppo_clip_adam``.
"""
import ctypes as C
import os

import numpy as np

from . import dist as sdist, hostcfg, policies, ppo_capi
from .learner import Learner


class LstmSpec(object):
    def __init__(self, ob_dim, ac_dim, nlstm=128):
        if nlstm not in (64, 128):
            raise NotImplementedError("nlstm must be 64 or 128")
        self.ob_dim, self.ac_dim, self.nlstm = int(ob_dim), int(ac_dim), int(nlstm)


class LstmPPOModel(Learner):
    loss_names = ["policy_loss", "value_loss", "policy_entropy", "approxkl", "clipfrac"]
    recurrent = True
    accepts_noise = True  # step(..., noise=rows) takes the action noise from the caller (device-mode Runner: one draw per rollout)
    use_graph = True      # single-GPU training on device tensors: the ~2T+12 launches of a minibatch step replay from a HIP graph

    def __init__(self, *, policy, ob_space=None, ac_space=None, nbatch_act=None, nbatch_train=None, nsteps=None, ent_coef=0.0,
                 vf_coef=0.5, max_grad_norm=0.5, microbatch_size=None, trainable=True, model_scope="", device=0, comm=None):
        import torch
        if not torch.cuda.is_available():
            raise ppo_capi.PpoHipError("LstmPPOModel needs a HIP device (no CPU fallback in the product path)")
        self.comm = comm if trainable else None      # torch.distributed group: every rank trains on its own env sequences
        self._t = torch
        self.spec, self.scope, self.sess = policy, model_scope, None
        self.device = torch.device("cuda", int(device))
        self.ent_coef, self.vf_coef, self.max_grad_norm = float(ent_coef), float(vf_coef), max_grad_norm
        self.trainable, self.nsteps, self.nenv = trainable, nsteps, nbatch_act
        D, A, H = policy.ob_dim, policy.ac_dim, policy.nlstm
        self.shapes = policies.lstm_param_shapes(D, A, H)
        self.sizes = [int(np.prod(s)) for s in self.shapes]
        self.P = int(sum(self.sizes))
        flat = np.concatenate([np.asarray(p, np.float32).ravel() for p in policies.init_lstm_param_list(D, A, H)])
        self.params = torch.from_numpy(flat).to(self.device)
        self.views = self._split(self.params)
        self._net = ppo_capi.fill_lstm_net_ifou(ppo_capi.LstmNet(), D, A, H, [v.data_ptr() for v in self.views])
        self.gen = torch.Generator(device=self.device)
        self.act_model = self.train_model = self
        self.initial_state = None if nbatch_act is None else np.zeros((int(nbatch_act), 2 * H), np.float32)   # models.py:176
        if trainable:
            self.m = torch.zeros(self.P, dtype=torch.float32, device=self.device)
            self.v = torch.zeros(self.P, dtype=torch.float32, device=self.device)
            self.t = 0
            self.grads = torch.zeros(self.P + ppo_capi.NSTATS, dtype=torch.float32, device=self.device)   # [flat grad | loss sums]
            self.gviews = self._split(self.grads)
            self.stats = torch.zeros(ppo_capi.NSTATS, dtype=torch.float64, device=self.device)
            self.moments = torch.zeros(3, dtype=torch.float64, device=self.device)
            self._graphs = hostcfg.GraphCache("recurrent PPO", self.device)
            self.wgrad_native = os.environ.get("SUMO_LSTM_WGRAD", "native") != "blas"
            self.seq_kernels = os.environ.get("SUMO_LSTM_SEQ", "1") != "0"    # whole-sequence forward / BPTT launches (nlstm 128)
            self.xproj = os.environ.get("SUMO_LSTM_XPROJ", "1") != "0"      # input block of the training forward hoisted out of the recurrence
            self.adv_ws = torch.zeros(ppo_capi.lib().ppo_adv_moments_workspace_bytes(), dtype=torch.uint8, device=self.device)
            self.wg_workspace = torch.empty(ppo_capi.lib().ppo_lstm_wgrad_workspace_bytes(D, H, A), dtype=torch.uint8, device=self.device)

    class _X:
        class dtype:
            name = "float32"
    X = _X()

    def _split(self, flat):
        out, o = [], 0
        for s, n in zip(self.shapes, self.sizes):
            out.append(flat[o:o + n].view(*s))
            o += n
        return out

    def seed(self, s):
        self.gen.manual_seed(int(s))

    # ---- checkpoints: list of the 8 tensors in TF variable order ---------------------------------------------------
    def get_param_list(self):
        return [v.cpu().numpy().copy() for v in self.views]

    def set_param_list(self, plist):
        assert len(plist) == len(self.shapes), "number of variables loaded mismatches len(variables)"
        for p, s in zip(plist, self.shapes):
            if tuple(np.shape(p)) != tuple(s):
                raise ValueError("parameter shape %s does not match %s" % (np.shape(p), s))
        self.params.copy_(self._t.from_numpy(np.concatenate([np.asarray(p, np.float32).ravel() for p in plist])))

    # ---- acting (policies.py:84-128 with the S / M feeds of models.py:163-170) --------------------------------------
    def net_dev(self):
        """Device copy of this model's ``ppo_lstm_net`` (its pointers address ``self.params``, whose storage never moves): what the
        fused recurrent rollout reads when this model is the opponent."""
        if getattr(self, "_net_dev", None) is None:
            self._net_dev = self._t.from_numpy(np.frombuffer(bytes(self._net), dtype=np.uint8).copy()).to(self.device)
        return self._net_dev

    def _run(self, obs, S, M, given_action=None, deterministic=False, noise=None):
        t = self._t
        np_in = not t.is_tensor(obs)
        D, A, H = self.spec.ob_dim, self.spec.ac_dim, self.spec.nlstm
        x = self._dev(obs).reshape(-1, D)
        n = x.shape[0]
        st = t.zeros((n, 2 * H), dtype=t.float32, device=self.device) if S is None else self._dev(S).clone()
        mask = None if M is None else self._dev(np.asarray(M, np.float32) if not t.is_tensor(M) else M.to(t.float32))
        action = t.empty((n, A), dtype=t.float32, device=self.device)
        neglogp = t.empty(n, dtype=t.float32, device=self.device)
        value = t.empty(n, dtype=t.float32, device=self.device)
        given = None if given_action is None else self._dev(given_action).reshape(n, A).contiguous()
        if deterministic or given is not None:
            noise = None
        elif noise is None:                       # (the device-mode Runner hands in the rows of a per-rollout draw instead)
            noise = t.randn((n, A), generator=self.gen, device=self.device, dtype=t.float32)
        ppo_capi.chk(ppo_capi.lib().ppo_lstm_step(C.byref(self._net), x.data_ptr(), n, x.stride(0) if n > 1 else D, ppo_capi.ptr(mask),
                                                  st.data_ptr(), st.data_ptr() + 4 * H, 2 * H, ppo_capi.ptr(noise), ppo_capi.ptr(given),
                                                  action.data_ptr(), neglogp.data_ptr(), value.data_ptr(), None,
                                                  t.cuda.current_stream(self.device).cuda_stream))
        out = (lambda z: z.cpu().numpy()) if np_in else (lambda z: z)
        return out(action), out(value), out(st), out(neglogp)

    def step(self, observation, S=None, M=None, deterministic=False, noise=None, **extra_feed):
        return self._run(observation, S, M, deterministic=deterministic, noise=noise)

    def value(self, ob, S=None, M=None, **kwargs):
        return self._run(ob, S, M, deterministic=True)[1]

    def action_probability(self, observation, given_action=None, S=None, M=None, **extra_feed):
        """Without ``S`` the sequence start state (zeros) is used -- what the reference's Runner does for the opponent's
        likelihood of the learner's action (runner.py:85 passes no state)."""
        return self._run(observation, S, M, given_action=given_action)[3]

    def score_and_value(self, observation, given_action):
        """(value, neglogp) of ``given_action`` from the sequence start state (zeros) in ONE evaluation: how the Runner scores and
        values agent 1's action when a policy-zoo net plays it (its state is not this net's)."""
        r = self._run(observation, None, None, given_action=given_action)
        return r[1], r[3]

    def score_value_advance(self, observation, S, M, given_action):
        """(value, neglogp of ``given_action``, new state) from the state ``S`` masked by ``M`` in ONE evaluation: how the Runner
        scores and values agent 1's action along the learner's shadow state under opponent-data reuse (``Runner.reuse_opponent``)."""
        r = self._run(observation, S, M, given_action=given_action)
        return r[1], r[3], r[2]

    # ---- training ---------------------------------------------------------------------------------------------------
    def loss_and_grads(self, cliprange, obs, returns, masks, actions, advs, neglogpacs, IS_weight, states, nsteps, world=1, valid=None):
        """Forward over ``nsteps`` + BPTT for a minibatch of whole env sequences.  Flat inputs are env-major
        ([nenv_mb * nsteps, ...], baselines' ``sf01`` order); ``states`` [nenv_mb, 2H] is the state at the start of the
        sequences.  Leaves d(mean loss)/d(theta) in ``self.grads``, the un-normalised loss sums in ``self.stats``.
        ``valid`` (0 / 1 per row, opponent-data reuse): rows with 0 stay in the recurrence and leave the loss
        (``ppo_lstm_head_grad_masked``); the mean is then over the valid rows, whose number the kernel reads from ``self.moments[2]``
        -- the caller (``_loss_step``) has run ``ppo_adv_moments_masked_ws`` on the same ``valid``."""
        t = self._t
        L = ppo_capi.lib()
        D, A, H = self.spec.ob_dim, self.spec.ac_dim, self.spec.nlstm
        T = int(nsteps)
        f32 = t.float32
        tm = lambda x, *tail: self._dev(x).reshape(-1, T, *tail).transpose(0, 1).contiguous()     # env-major flat -> [T, n, ...]
        X, Mk, Ac = tm(obs, D), tm(np.asarray(masks, np.float32) if not t.is_tensor(masks) else masks.to(f32)), tm(actions, A)
        Ad, R, Old, W = tm(advs), tm(returns), tm(neglogpacs), tm(IS_weight)
        n = X.shape[1]
        rows = T * n
        st = t.cuda.current_stream(self.device).cuda_stream
        state = self._dev(states).reshape(n, 2 * H).clone()
        dev = self.device
        gates = t.empty((T, n, 4 * H), dtype=f32, device=dev)
        cprev, hprev, tanhc, lat = (t.empty((T, n, H), dtype=f32, device=dev) for _ in range(4))
        net = C.byref(self._net)
        # the input block x * wx of all T steps in one launch; the T sequential steps then only run the recurrent block on top of it
        # (same sums bit for bit, half the dependent chain per step).  The buffer is the one the backward sweep fills with dz later.
        dz = t.empty((T, n, 4 * H), dtype=f32, device=dev)
        if self.xproj:
            ppo_capi.chk(L.ppo_lstm_xproj(net, X.data_ptr(), rows, D, dz.data_ptr(), st))
        seq = self.xproj and self.seq_kernels and H == 128      # all T steps in one launch, recurrent weights resident in registers
        if seq:
            ppo_capi.chk(L.ppo_lstm_seq_forward(net, dz.data_ptr(), T, n, Mk.data_ptr(), state.data_ptr(), state.data_ptr() + 4 * H, 2 * H,
                                                gates.data_ptr(), cprev.data_ptr(), hprev.data_ptr(), tanhc.data_ptr(), lat.data_ptr(), st))
        for k in range(0 if seq else T):
            if self.xproj:
                ppo_capi.chk(L.ppo_lstm_step_save_z(net, dz[k].data_ptr(), n, Mk[k].data_ptr(), state.data_ptr(), state.data_ptr() + 4 * H, 2 * H,
                                                    gates[k].data_ptr(), cprev[k].data_ptr(), hprev[k].data_ptr(), tanhc[k].data_ptr(),
                                                    lat[k].data_ptr(), st))
            else:
                ppo_capi.chk(L.ppo_lstm_step_save(net, X[k].data_ptr(), n, D, Mk[k].data_ptr(), state.data_ptr(), state.data_ptr() + 4 * H,
                                                  2 * H, gates[k].data_ptr(), cprev[k].data_ptr(), hprev[k].data_ptr(), tanhc[k].data_ptr(), st))
                lat[k].copy_(state[:, H:])
        dlat = t.empty((T, n, H), dtype=f32, device=dev)
        dmean = t.empty((rows, A), dtype=f32, device=dev)
        dvalue = t.empty(rows, dtype=f32, device=dev)
        dls = t.empty((rows, A), dtype=f32, device=dev)
        self.stats.zero_()
        if valid is None:
            ppo_capi.chk(L.ppo_lstm_head_grad(net, lat.data_ptr(), rows, Ac.data_ptr(), Ad.data_ptr(), R.data_ptr(), Old.data_ptr(), W.data_ptr(),
                                              1.0 / (rows * world), float(cliprange), self.vf_coef, dlat.data_ptr(), dmean.data_ptr(), dvalue.data_ptr(),
                                              dls.data_ptr(), self.stats.data_ptr(), st))
        else:
            Vd = tm(valid)
            ppo_capi.chk(L.ppo_lstm_head_grad_masked(net, lat.data_ptr(), rows, Ac.data_ptr(), Ad.data_ptr(), R.data_ptr(), Old.data_ptr(),
                                                     W.data_ptr(), Vd.data_ptr(), self.moments.data_ptr() + 16, float(cliprange), self.vf_coef,
                                                     dlat.data_ptr(), dmean.data_ptr(), dvalue.data_ptr(), dls.data_ptr(), self.stats.data_ptr(), st))
        if seq:
            ppo_capi.chk(L.ppo_lstm_seq_backward(net, T, n, dlat.data_ptr(), Mk.data_ptr(), gates.data_ptr(), cprev.data_ptr(), tanhc.data_ptr(),
                                                 dz.data_ptr(), st))
        dh = t.zeros((n, H), dtype=f32, device=dev)
        dc = t.zeros((n, H), dtype=f32, device=dev)
        for k in range(-1 if seq else T - 1, -1, -1):
            ppo_capi.chk(L.ppo_lstm_bwd_step(net, n, dlat[k].data_ptr(), Mk[k].data_ptr(), gates[k].data_ptr(), cprev[k].data_ptr(),
                                             tanhc[k].data_ptr(), dh.data_ptr(), dc.data_ptr(), dz[k].data_ptr(), st))
        # weight gradients: [x | h_prev | 1]^T dz and [latent | 1]^T [dmean | dvalue | dlogstd rows] over all (time, env) rows, on the
        # split-K MFMA kernel (ppo_lstm_wgrad; SUMO_LSTM_WGRAD=blas keeps the library GEMMs for cross-checks)
        if self.wgrad_native:
            ppo_capi.chk(L.ppo_lstm_wgrad(net, rows, X.data_ptr(), hprev.data_ptr(), dz.data_ptr(), lat.data_ptr(), dmean.data_ptr(),
                                          dvalue.data_ptr(), dls.data_ptr(), -self.ent_coef / world, self.grads.data_ptr(),
                                          self.wg_workspace.data_ptr(), st))
        else:
            Z2, X2, H2, L2 = dz.view(rows, 4 * H), X.view(rows, D), hprev.view(rows, H), lat.view(rows, H)
            g = self.gviews
            t.matmul(X2.t(), Z2, out=g[0])
            t.matmul(H2.t(), Z2, out=g[1])
            t.sum(Z2, dim=0, out=g[2])
            t.matmul(L2.t(), dmean, out=g[3])
            t.sum(dmean, dim=0, out=g[4])
            g[5].copy_((dls.sum(dim=0) - self.ent_coef / world).view(1, A))     # the entropy term once in the global sum
            t.matmul(L2.t(), dvalue.view(rows, 1), out=g[6])
            g[7].copy_(dvalue.sum().view(1))
        return state

    def _loss_step(self, cliprange, obs, ret, val, masks, actions, neglogpacs, IS_weight, states, T, world, valid=None):
        """Advantage normalisation (model.py:180-185) + loss_and_grads: everything of a minibatch step before the optimiser.
        ``valid``: the masked entries (moments and normalisation over the valid rows, 0 elsewhere; single-GPU)."""
        t = self._t
        L = ppo_capi.lib()
        nrow = ret.numel()
        st = t.cuda.current_stream(self.device).cuda_stream
        adv = t.empty(nrow, dtype=t.float32, device=self.device)
        if valid is not None:
            if self.comm is not None:
                raise NotImplementedError("a row mask (opponent-data reuse for recurrent learners) is single-GPU")
            vd = self._dev(valid).to(t.float32).contiguous()
            ppo_capi.chk(L.ppo_adv_moments_masked_ws(ret.data_ptr(), val.data_ptr(), vd.data_ptr(), nrow, self.moments.data_ptr(), self.adv_ws.data_ptr(), st))
            ppo_capi.chk(L.ppo_adv_normalize_masked(ret.data_ptr(), val.data_ptr(), vd.data_ptr(), nrow, self.moments.data_ptr(), adv.data_ptr(), st))
            self.loss_and_grads(cliprange, obs, ret, masks, actions, adv, neglogpacs, IS_weight, states, T, world=world, valid=vd)
            return
        ppo_capi.chk(L.ppo_adv_moments_ws(ret.data_ptr(), val.data_ptr(), None, nrow, self.moments.data_ptr(), self.adv_ws.data_ptr(), st))
        sdist.allreduce_moments(self.moments, self.comm)                                # global advantage normalisation
        ppo_capi.chk(L.ppo_adv_normalize(ret.data_ptr(), val.data_ptr(), None, nrow, self.moments.data_ptr(), adv.data_ptr(), st))
        self.loss_and_grads(cliprange, obs, ret, masks, actions, adv, neglogpacs, IS_weight, states, T, world=world)

    def _graph_step(self, cliprange, tensors, T):
        """Replay ``_loss_step`` from a HIP graph captured once per (minibatch shape, cliprange): the inputs are copied into
        buffers owned by the graph, the 2T+12 kernel launches and GEMMs of the step then cost one launch on the host.
        A ninth tensor is the row mask ``valid``: one more static buffer, and (through the shapes) part of the key; the number of
        valid rows is read on the device, so one graph serves every mask.
        Returns False (after switching the graph path off) if capture is not possible here."""
        t = self._t
        key = (tuple(tuple(x.shape) for x in tensors), tuple(x.dtype for x in tensors), int(T), float(cliprange))
        ent = self._graphs.get(key)
        if ent is None:
            def make_record():
                static = [t.empty(x.shape, dtype=x.dtype, device=self.device) for x in tensors]
                for d, x in zip(static, tensors):
                    d.copy_(x)
                return dict(static=static)

            def body(ent):
                obs, returns, masks, actions, values, neglogpacs, IS_weight, states = ent["static"][:8]
                self._loss_step(cliprange, obs, returns.contiguous(), values.contiguous(), masks, actions, neglogpacs, IS_weight, states, T, 1,
                                valid=ent["static"][8] if len(ent["static"]) > 8 else None)
            ent = self._graphs.capture(key, make_record, body, lambda: setattr(type(self), "use_graph", False))
            if ent is None:
                return False
        else:
            for d, x in zip(ent["static"], tensors):
                d.copy_(x)
        ent["graph"].replay()
        return True

    def train(self, lr, cliprange, obs, returns, masks, actions, values, neglogpacs, rewards, IS_weight, states=None, nsteps=None, valid=None):
        """``valid`` (0 / 1 per row; None: every row counts, the unmasked entries call for call): rows with 0 stay in the recurrence and
        leave the loss, the advantage moments and the statistics, which are means over the valid rows.  A minibatch without a valid
        row (possible when only agent-1 sequences are drawn) has a zero gradient (but for the entropy term's constant on logstd,
        which no row carries): the optimiser still takes its step on it -- Adam's moments decay, the step counter advances -- and
        the statistics come back as 0."""
        if not self.trainable:
            raise RuntimeError("model built with trainable=False")
        if states is None:
            raise ValueError("a recurrent model trains on whole sequences: pass the start states of the minibatch envs")
        t = self._t
        np_in = not t.is_tensor(obs)
        T = int(nsteps or self.nsteps)
        world = 1 if self.comm is None else t.distributed.get_world_size(self.comm)
        tensors = (obs, returns, masks, actions, values, neglogpacs, IS_weight, states)
        if valid is not None:
            tensors += (valid.to(t.float32) if t.is_tensor(valid) else valid,)
        if not (self.use_graph and self.comm is None and all(t.is_tensor(x) for x in tensors)
                and self._graph_step(cliprange, tensors, T)):
            ret, val = self._dev(returns).contiguous(), self._dev(values).contiguous()
            self._loss_step(cliprange, obs, ret, val, masks, actions, neglogpacs, IS_weight, states, T, world, valid=valid)
        st = t.cuda.current_stream(self.device).cuda_stream
        if self.comm is not None:            # equal shards per rank
            self._allreduce_grad_and_stats()
        entropy = float((self.views[5].double() + 0.5 * np.log(2.0 * np.pi * np.e)).sum().item())
        self._adam_step(lr, st)
        s = self.stats.cpu().numpy()
        cnt = s[6] if valid is None else max(s[6], 1.0)
        out = [s[0] / cnt, s[1] / cnt, entropy, s[3] / cnt, s[4] / cnt]
        return [np.float32(x) for x in out] + [None, None] if np_in else out + [None, None]
