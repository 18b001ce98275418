"""The 'ours' opponent selector (ratio-divergence sampling, reference alg_ppo.py:227-244) on a device table of checkpoints.

``alg_ppo.learn`` scores up to 30 saved checkpoints per update: for each one a file read, 13 host-to-device copies, a
``ppo_forward`` launch over the opponent's whole sample batch and a host read-back.  :class:`FusedSelector` keeps the checkpoints as
rows of a ``matches.SnapshotTable`` and scores every candidate in ONE ``ppo_selection_scores`` launch (include/sumo_ppo.h) that
stages each 16-row tile of the batch once, followed by one device-to-host copy of the per-candidate sums and counts.

Two table modes, chosen at construction from the run length:

* **history** -- one row per checkpoint of the run (``capacity_rows`` rows fit ``table_mb``): ``note_saved`` copies the learner's
  parameters into the row device to device right after the checkpoint is written, so no file is read again.  The whole table,
  ``capacity_rows`` x P x 4 bytes (98 KB per row on Ant, at most ``table_mb``), is allocated and zero-filled at construction.
* **staging** -- the run is too long for that, or ``table_mb`` was set lower: a 32-row table (3 MB on Ant) is refilled from the
  sampled checkpoint files each update (the file reads stay, the per-candidate launches still become one).

Opt-in (``learn(fused_selector=True)``, ``run.py --fused_selector``); MLP(64,64) policies only.
"""
import os

import numpy as np

from . import matches, ppo_capi

MAX_CANDIDATES = 32      # SEL_MAX_CAND of csrc/ppo_kernels.hip


def selection_probs_from_scores(scores):
    """Sampling probabilities from the candidates' scores (alg_ppo.py:241-242): normalised, or uniform where the total is not
    finite or not positive (every candidate equals the current opponent)."""
    rd = np.asarray(scores, dtype=np.float64)
    tot = rd.sum()
    return rd / tot if np.isfinite(tot) and tot > 0 else np.full(len(rd), 1.0 / len(rd))


def _stamp(path):
    """What identifies the content a row was filled from: the file and its modification time (a run started in a directory that
    already holds checkpoints overwrites them one by one)."""
    return (str(path), os.stat(path).st_mtime_ns)


class FusedSelector(object):
    def __init__(self, spec, device, capacity_rows, table_mb=1024):
        import torch
        self._t = torch
        self.spec = spec
        P = matches.param_count(spec.ob_dim, spec.ac_dim)
        self.staging = int(capacity_rows) * P * 4 > float(table_mb) * 2 ** 20
        self.table = matches.SnapshotTable(spec, MAX_CANDIDATES if self.staging else int(capacity_rows), device)
        self.device, self.capacity = self.table.device, self.table.capacity
        self.stamps = [None] * self.capacity          # per row: _stamp of the file it holds (None: never filled)
        self._staged = None                           # staging mode: the rows the table holds now, in slot order
        self.rows_dev = torch.zeros(MAX_CANDIDATES, dtype=torch.int32, device=self.device)
        # sums (float64) and counts (int32) side by side, so that one copy brings both to the host
        self.out = torch.zeros(MAX_CANDIDATES * 12, dtype=torch.uint8, device=self.device)
        self.score_sum = self.out[:MAX_CANDIDATES * 8].view(torch.float64)
        self.finite_count = self.out[MAX_CANDIDATES * 8:].view(torch.int32)
        self.workspace = torch.zeros(ppo_capi.lib().ppo_selection_scores_workspace_bytes(), dtype=torch.uint8, device=self.device)   # zeroed once: sumo_ppo.h

    @property
    def filled(self):
        return self.table.filled

    def note_saved(self, k, model, path=None):
        """Checkpoint ``k`` of the run (its position in the sorted checkpoint directory) was just written from ``model``: copy
        ``model.params`` into row ``k``, device to device.  Nothing to do in staging mode or past the table's end (``ensure`` reads
        such a row from its file when it is sampled)."""
        if self.staging or not 0 <= k < self.capacity:
            return False
        if tuple(model.params.shape) != (self.table.P,):
            raise ValueError("model has %s parameters, the table's rows %d" % (tuple(model.params.shape), self.table.P))
        self.table.params[k].copy_(model.params)
        self.table.filled[k] = True
        self.table.labels[k] = None if path is None else str(path)
        self.stamps[k] = None if path is None else _stamp(path)
        return True

    def ensure(self, paths, rows):
        """Make the checkpoints ``paths[r]`` for r in ``rows`` resident.  History mode: a row that is not filled yet, or was filled
        from another file (content), is read from its file; the others are left alone.  Staging mode: the files are loaded into
        slots 0 .. len(rows) - 1.  Returns the number of files read."""
        rows = [int(r) for r in rows]
        if not 1 <= len(rows) <= MAX_CANDIDATES:
            raise ValueError("%d candidates: the selector scores 1 to %d per launch" % (len(rows), MAX_CANDIDATES))
        if self.staging:
            self._staged = None
            for j, r in enumerate(rows):
                self.table.set(j, paths[r])
            self._staged = rows
            return len(rows)
        nread = 0
        for r in rows:
            if not 0 <= r < self.capacity:
                raise IndexError("checkpoint %d outside the selector's table of %d rows" % (r, self.capacity))
            if self.table.filled[r] and (self.stamps[r] is None or self.stamps[r] == _stamp(paths[r])):
                continue
            self.table.set(r, paths[r])
            self.stamps[r] = _stamp(paths[r])
            nread += 1
        return nread

    def _slots(self, rows):
        rows = [int(r) for r in rows]
        if not 1 <= len(rows) <= MAX_CANDIDATES:
            raise ValueError("%d candidates: the selector scores 1 to %d per launch" % (len(rows), MAX_CANDIDATES))
        if self.staging:
            if rows != self._staged:
                raise ValueError("staging mode: ensure(paths, rows) loads the rows that scores() then reads")
            return list(range(len(rows)))
        for r in rows:
            if not 0 <= r < self.capacity or not self.table.filled[r]:
                raise ValueError("row %d of the selector's table is not filled" % r)
        return rows

    def launch(self, ref_params, rows, obs, actions, max_blocks=0, neglogp_dbg=None):
        """The one launch behind :meth:`scores`; the sums and counts stay on the device (``score_sum`` / ``finite_count`` [:len(rows)])."""
        t = self._t
        slots = self._slots(rows)
        D, A = self.spec.ob_dim, self.spec.ac_dim
        for x, cols in ((obs, D), (actions, A)):
            if not t.is_tensor(x) or x.dtype != t.float32 or not x.is_cuda or x.dim() != 2 or x.shape[1] != cols or x.stride(1) != 1:
                raise ValueError("expected a float32 CUDA matrix with %d columns and unit inner stride" % cols)
        n = int(obs.shape[0])
        if actions.shape[0] != n:
            raise ValueError("%d observation rows, %d action rows" % (n, actions.shape[0]))
        if not actions.is_contiguous():
            actions = actions.contiguous()
        if tuple(ref_params.shape) != (self.table.P,) or ref_params.dtype != t.float32 or not ref_params.is_cuda:
            raise ValueError("ref_params must be the flat float32 CUDA parameter vector of the policy (%d entries)" % self.table.P)
        if neglogp_dbg is not None and (tuple(neglogp_dbg.shape) != (len(slots) + 1, n) or neglogp_dbg.dtype != t.float32
                                        or not neglogp_dbg.is_cuda or not neglogp_dbg.is_contiguous()):
            raise ValueError("neglogp_dbg must be a contiguous float32 CUDA tensor of shape (%d, %d)" % (len(slots) + 1, n))
        self.rows_dev[:len(slots)].copy_(t.tensor(slots, dtype=t.int32))
        st = t.cuda.current_stream(self.device).cuda_stream
        ppo_capi.chk(ppo_capi.lib().ppo_selection_scores(
            ref_params.data_ptr(), self.table.params.data_ptr(), self.table.params.stride(0), self.rows_dev.data_ptr(), len(slots),
            obs.data_ptr(), n, obs.stride(0), D, A, actions.data_ptr(), self.score_sum.data_ptr(), self.finite_count.data_ptr(),
            ppo_capi.ptr(neglogp_dbg), int(max_blocks), self.workspace.data_ptr(), st))
        return len(slots)

    def scores(self, ref_params, rows, obs, actions, max_blocks=0, neglogp_dbg=None):
        """Mean |nap / ap - 1| over the finite rows per candidate (0 where none is finite: ``alg_ppo.selection_probs``' rule), float64
        numpy [len(rows)].  One launch, one device-to-host copy."""
        k = self.launch(ref_params, rows, obs, actions, max_blocks, neglogp_dbg)
        host = self.out.cpu().numpy()
        sums = host[:MAX_CANDIDATES * 8].view(np.float64)[:k]
        counts = host[MAX_CANDIDATES * 8:].view(np.int32)[:k]
        return np.where(counts > 0, sums / np.maximum(counts, 1), 0.0)
