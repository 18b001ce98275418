"""What the learners (``PPOModel`` and with it ``ActorCriticModel``, ``LstmPPOModel``) share on the host: checkpoint files, host-to-device
staging, the Adam launch and the fused gradient all-reduce.  A learner provides ``params`` / ``grads`` / ``m`` / ``v`` (flat float32),
``stats`` (float64 [NSTATS]), ``P``, ``t``, ``max_grad_norm``, ``comm``, ``device``, ``_t`` (torch) and its own ``get_param_list`` /
``set_param_list`` (the parameter layouts differ)."""
import os

import numpy as np

from . import dist as sdist, ppo_capi


class Learner(object):
    def save(self, save_path):
        dirname = os.path.dirname(save_path)
        if dirname:
            os.makedirs(dirname, exist_ok=True)
        import joblib
        joblib.dump(self.get_param_list(), save_path)                  # same on-disk format as the reference's model.py:161

    def load(self, load_path):
        import joblib
        self.set_param_list(joblib.load(os.path.expanduser(load_path)))   # only files written by save()

    def _dev(self, x, dtype=np.float32):
        t = self._t
        return x if t.is_tensor(x) else t.from_numpy(np.ascontiguousarray(x, dtype)).to(self.device)

    def _adam_step(self, lr, st):
        """Global-norm clip + Adam on ``self.grads``.  The step count is a host scalar, which is why this launch stays outside the
        captured graphs."""
        self.t += 1
        ppo_capi.chk(ppo_capi.lib().ppo_clip_adam(self.params.data_ptr(), self.grads.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.P,
                                                   self.t, float(lr), 0.9, 0.999, 1e-5,
                                                   float(self.max_grad_norm) if self.max_grad_norm is not None else 0.0,
                                                   self.stats.data_ptr(), st))

    def _allreduce_grad_and_stats(self):
        """ONE fused collective per optimiser step: [flat grad | NSTATS loss sums], the sums riding in ``grads[P : P + NSTATS]``
        (the reference's only gradient collective, mpi_adam_optimizer.py:39, all-reduces the flat gradient alone)."""
        t, sl = self._t, slice(self.P, self.P + ppo_capi.NSTATS)
        self.grads[sl] = self.stats.to(t.float32)
        sdist.allreduce_fused(self.grads, self.comm)
        self.stats.copy_(self.grads[sl].to(t.float64))
