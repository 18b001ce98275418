"""Checkpoint-vs-checkpoint matches on the GPU: the reference's compare_history_version.py / play_evaluation.py, plus a
round-robin over the versions of one run.

The reference loads version *i* of run P1 and version *i* of run P2 into two models and plays ``--trials`` games between them
on one env (stochastic ``model.step`` for both sides, ``agent._adjust_z = -0.5`` on every agent, compare_history_version.py:16-47,
:73-74), writing P1's win rate per version.  Here the snapshots of every match-up live as rows of one device table
(:class:`SnapshotTable`), each env plays one match-up (``idx0[e]`` for agent 0, ``idx1[e]`` for agent 1), and the fused match
launch (include/sumo_hip.h ``sumo_match_steps``) runs ``chunk`` whole env steps of every env with both policies evaluated inside
the owning wave, keeping each env's score {agent-0 wins, agent-1 wins, draws} on the device.  The host reads that small counter
tensor once per launch.

An episode is a win if agent 0 carries the 'winner' flag when it ends, a loss if only agent 1 does, a draw otherwise
(compare_history_version.py:33-41; policy_zoo._evaluate_against).  ``fused=False`` plays the same games step by step: two
``ppo_forward`` launches (what ``PPOModel.step`` runs) per match-up and side, then ``step_device``; with the same seed it draws
the same noise and yields bit-identical envs and scores.

Recurrent checkpoints (``LstmPPOModel.save``, ``learn(network='lstm')``) go into an :class:`LstmSnapshotTable` instead: the
same drivers detect the kind from the checkpoint files (:func:`checkpoint_kind`), and each side carries its own recurrent state
per env, zeroed where a batch starts and masked by that side's done flag of the previous step (``LstmPPOModel.step(obs, S, M)``).
The fused path is ``sumo_match_steps_lstm`` (LSTM(128)); ``fused=False`` makes one ``ppo_lstm_step`` launch per side and run of
envs sharing a snapshot, bit-identical again.

An MLP(64,64) run against an LSTM run plays through :func:`play_cross_matches` (one table per agent, either seating;
``sumo_match_steps_cross`` for LSTM(128), any width step by step); the version drivers take it with ``cross_family=True`` and
refuse it otherwise.

Policy-zoo opponents sit in a :class:`policy_zoo.ZooTable` (MLP nets) or a :class:`policy_zoo.ZooLstmTable` (LSTM nets) and play
agent 1 (:func:`play_against_zoo`, :func:`evaluate_history_against_zoo`): MLP checkpoints face either family, LSTM(128)
checkpoints face zoo LSTM nets (``sumo_match_steps_zoo`` / ``sumo_match_steps_zoo_lstm`` / ``sumo_match_steps_lstm_zoo_lstm``);
LSTM checkpoints against zoo MLP nets play with ``cross_family=True`` (``sumo_match_steps_lstm_zoo``) and are refused otherwise.
"""
import collections
import ctypes as C
import os
import warnings

import numpy as np

from . import capi, policies

EVAL_ADJUST_Z = -0.5      # compare_history_version.py:73-74


# ---- checkpoints ---------------------------------------------------------------------------------------------------------
def param_count(ob_dim, ac_dim):
    return sum(int(np.prod(s)) for s in policies.param_shapes(ob_dim, ac_dim))


def _source_vector(src, check_model, dict_hint, from_list, P, policy_name):
    """The source-type ladder behind :func:`snapshot_vector` / :func:`lstm_snapshot_vector`: a checkpoint path is loaded into
    its array list, a model yields its flat ``params`` (after ``check_model(src)``, which raises on the wrong kind or shape), a
    tensor becomes an array, dicts are refused, an array list goes through ``from_list(list, label)``, anything else must be a
    flat vector of ``P`` entries."""
    label = None
    if isinstance(src, (str, os.PathLike)):
        import joblib
        label = str(src)
        src = joblib.load(os.path.expanduser(str(src)))            # only files written by the models' save()
    if hasattr(src, "params") and hasattr(src, "spec"):            # PPOModel / ActorCriticModel / LstmPPOModel
        check_model(src)
        return src.params.detach().cpu().numpy().astype(np.float32).reshape(-1)
    if hasattr(src, "detach"):                                     # torch tensor
        src = src.detach().cpu().numpy()
    if isinstance(src, dict):
        raise ValueError("dict checkpoints are not supported here; load them into %s first" % dict_hint)
    if isinstance(src, (list, tuple)):
        return from_list(src, label or "checkpoint")
    v = np.ascontiguousarray(src, np.float32).reshape(-1)
    if v.size != P:
        raise ValueError("snapshot has %d parameters, the %s %d" % (v.size, policy_name, P))
    return v


def snapshot_vector(spec, src):
    """Flat float32 parameter vector (numpy) of an MLP(64,64) policy of ``spec`` from a ``PPOModel`` / ``ActorCriticModel``, a
    flat vector, the 13-array list of a checkpoint (model.py:153-177) or a checkpoint path written by ``PPOModel.save``.
    LSTM models and checkpoints are refused here: they play in an :class:`LstmSnapshotTable`."""
    D, A = spec.ob_dim, spec.ac_dim
    if getattr(src, "recurrent", False):
        raise ValueError("recurrent (LSTM) models do not play in a SnapshotTable (MLP(64,64) policies): use LstmSnapshotTable")

    def check_model(m):
        if (m.spec.ob_dim, m.spec.ac_dim) != (D, A):
            raise ValueError("model's policy (%d, %d) does not match the table's (%d, %d)" % (m.spec.ob_dim, m.spec.ac_dim, D, A))

    def from_list(plist, name):
        got = [tuple(np.shape(p)) for p in plist]
        if got == [tuple(x) for x in policies.lstm_param_shapes(D, A)]:
            raise ValueError("%s is an LSTM checkpoint: it plays in an LstmSnapshotTable, not in a SnapshotTable" % name)
        if got != [tuple(x) for x in policies.param_shapes(D, A)]:
            raise ValueError("%s does not match the MLP(64,64) policy of ob_dim %d / ac_dim %d" % (name, D, A))
        return policies.flatten_params(list(plist))

    return _source_vector(src, check_model, "a PPOModel", from_list, param_count(D, A), "policy")


def checkpoint_kind(path):
    """('mlp', None) for a checkpoint written by ``PPOModel.save`` (the 13 arrays of MLP(64,64)), ('lstm', nlstm) for one written by
    ``LstmPPOModel.save`` (the 8 arrays of ``lstm_param_shapes``), read from the array shapes."""
    import joblib
    plist = joblib.load(os.path.expanduser(str(path)))            # only files written by PPOModel.save() / LstmPPOModel.save()
    return _list_kind(plist, str(path))


def _list_kind(plist, label):
    if isinstance(plist, (list, tuple)):
        sh = [tuple(np.shape(p)) for p in plist]
        if len(sh) == 13 and len(sh[0]) == 2:
            D, A = sh[0][0], sh[8][1] if len(sh[8]) == 2 else -1
            if sh == [tuple(x) for x in policies.param_shapes(D, A)]:
                return "mlp", None
        if len(sh) == 8 and len(sh[0]) == 2 and len(sh[3]) == 2:
            D, H, A = sh[0][0], sh[3][0], sh[3][1]
            if sh == [tuple(x) for x in policies.lstm_param_shapes(D, A, H)]:
                return "lstm", H
    raise ValueError("%s is neither an MLP(64,64) nor an LSTM checkpoint" % label)


def _lstm_param_count(spec):
    return sum(int(np.prod(x)) for x in policies.lstm_param_shapes(spec.ob_dim, spec.ac_dim, spec.nlstm))


def lstm_snapshot_vector(spec, src):
    """Flat float32 parameter vector (numpy) of an LSTM policy of ``spec`` (``LstmSpec``) from an ``LstmPPOModel``, a flat vector,
    the 8-array list of ``lstm_param_shapes`` or a checkpoint path written by ``LstmPPOModel.save``.  MLP models and checkpoints,
    and LSTM policies of another width, are refused."""
    D, A, H = spec.ob_dim, spec.ac_dim, spec.nlstm

    def check_model(m):
        if not getattr(m, "recurrent", False):
            raise ValueError("MLP models cannot play in an LSTM snapshot table: use SnapshotTable")
        got = (m.spec.ob_dim, m.spec.ac_dim, m.spec.nlstm)
        if got != (D, A, H):
            raise ValueError("model's policy (%d, %d, LSTM(%d)) does not match the table's (%d, %d, LSTM(%d))" % (got + (D, A, H)))

    def from_list(plist, name):
        try:
            kind, h = _list_kind(plist, name)
        except ValueError:
            kind, h = None, None
        if kind == "mlp":
            raise ValueError("%s is an MLP(64,64) checkpoint: it plays in a SnapshotTable, not in an LSTM table" % name)
        if kind == "lstm" and h != H:
            raise ValueError("%s is an LSTM(%d) checkpoint, the table holds LSTM(%d) policies" % (name, h, H))
        if [tuple(np.shape(p)) for p in plist] != [tuple(x) for x in policies.lstm_param_shapes(D, A, H)]:
            raise ValueError("%s does not match the LSTM(%d) policy of ob_dim %d / ac_dim %d" % (name, H, D, A))
        return np.concatenate([np.asarray(p, np.float32).ravel() for p in plist])

    return _source_vector(src, check_model, "an LstmPPOModel", from_list, _lstm_param_count(spec), "LSTM policy")


class _SnapshotTableBase(object):
    """Device table ``params [capacity][P]`` of frozen policies of one ``spec``, with the rows' fill state and labels.  A
    subclass names its parameter count (``param_count_of``) and its vector loader (``vector_of``)."""
    recurrent = False

    def __init__(self, spec, capacity, device=0):
        import torch
        self.spec = spec
        self.capacity = int(capacity)
        if self.capacity < 1:
            raise ValueError("capacity must be >= 1")
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.P = self.param_count_of(spec)
        self.params = torch.zeros((self.capacity, self.P), dtype=torch.float32, device=self.device)
        self.filled = np.zeros(self.capacity, bool)
        self.labels = [None] * self.capacity

    def set(self, k, src, label=None):
        """Fill row ``k`` (see the table's ``vector_of`` for what ``src`` may be)."""
        import torch
        if not 0 <= k < self.capacity:
            raise IndexError("row %d outside the table of %d" % (k, self.capacity))
        v = self.vector_of(self.spec, src)
        self.params[k].copy_(torch.from_numpy(v).to(self.device))
        self.filled[k] = True
        self.labels[k] = label if label is not None else (str(src) if isinstance(src, (str, os.PathLike)) else None)

    @classmethod
    def from_checkpoints(cls, spec, paths, device=0):
        t = cls(spec, len(paths), device)
        for k, p in enumerate(paths):
            t.set(k, p)
        return t


class SnapshotTable(_SnapshotTableBase):
    """Device table ``params [capacity][P]`` of frozen MLP(64,64) policies in checkpoint order (the layout of sumo_ppo.h); rows
    are filled from what :func:`snapshot_vector` accepts."""
    param_count_of = staticmethod(lambda spec: param_count(spec.ob_dim, spec.ac_dim))
    vector_of = staticmethod(snapshot_vector)


class LstmSnapshotTable(_SnapshotTableBase):
    """Device table ``params [capacity][P]`` of frozen LSTM policies (``lstm_param_shapes`` order, what ``LstmPPOModel.save``
    writes; rows are filled from what :func:`lstm_snapshot_vector` accepts) plus the device array of their ``ppo_lstm_net``
    structs (``nets_dev``) and a host prototype (``proto``)."""
    recurrent = True
    param_count_of = staticmethod(_lstm_param_count)
    vector_of = staticmethod(lstm_snapshot_vector)

    def __init__(self, spec, capacity, device=0):
        from . import ppo_capi
        from .opponent_pool import fill_lstm_net
        super(LstmSnapshotTable, self).__init__(spec, capacity, device)
        import torch
        self.nets = (ppo_capi.LstmNet * self.capacity)()
        for k in range(self.capacity):
            fill_lstm_net(self.nets[k], self.params[k].data_ptr(), spec)
        self.proto = fill_lstm_net(ppo_capi.LstmNet(), self.params[0].data_ptr(), spec)
        self.nets_dev = torch.from_numpy(np.frombuffer(bytes(self.nets), dtype=np.uint8).copy()).to(self.device)


def checkpoint_dir(path):
    """``path`` may be a run directory (holding ``checkpoints/``) or the checkpoint directory itself."""
    ck = os.path.join(path, "checkpoints")
    return ck if os.path.isdir(ck) else path


def list_checkpoints(path):
    """Checkpoint ids of a run, sorted, ``00000`` (the untrained initial version) excluded (compare_history_version.py:63-69)."""
    ck = checkpoint_dir(path)
    ids = [f for f in os.listdir(ck) if f.isdigit() and f != "00000" and os.path.isfile(os.path.join(ck, f))]
    return sorted(ids, key=lambda f: (int(f), f))


def pair_versions(ids1, ids2):
    """Version i of P1 with version i of P2, up to the shorter list (the reference indexes P2 with P1's positions and fails
    where P2 is shorter; here the extra versions are dropped with a warning)."""
    n = min(len(ids1), len(ids2))
    if len(ids1) != len(ids2):
        warnings.warn("P1 has %d versions and P2 %d: comparing the first %d" % (len(ids1), len(ids2), n))
    return list(zip(ids1[:n], ids2[:n]))


def split_trials(trials, num_env):
    """(envs_per_pair, rounds_per_env) with envs_per_pair * rounds_per_env == trials: the largest divisor of ``trials`` that
    fits ``num_env`` envs, so a match-up's ``trials`` games run on as many envs in parallel as possible."""
    trials, num_env = int(trials), int(num_env)
    if trials < 1 or num_env < 1:
        raise ValueError("trials and num_env must be >= 1")
    epp = max(d for d in range(1, min(trials, num_env) + 1) if trials % d == 0)
    return epp, trials // epp


def plan_batches(npairs, envs_per_pair, num_envs):
    """Match-ups per launch batch: each batch gives pair b of the batch the CONTIGUOUS env block [b * envs_per_pair,
    (b + 1) * envs_per_pair), so waves running at the same time mostly read the same snapshots (L2 reuse)."""
    if envs_per_pair < 1 or envs_per_pair > num_envs:
        raise ValueError("envs_per_pair %d must be in [1, %d]" % (envs_per_pair, num_envs))
    per = num_envs // envs_per_pair
    return [list(range(b, min(b + per, npairs))) for b in range(0, npairs, per)]


def env_assignment(pairs, batch, envs_per_pair, num_envs):
    """Host arrays (idx0, idx1, active) of one batch: env e of block b plays pairs[batch[b]]; envs past the last block play
    snapshot 0 against itself and are not counted (active False)."""
    idx0 = np.zeros(num_envs, np.int32)
    idx1 = np.zeros(num_envs, np.int32)
    active = np.zeros(num_envs, bool)
    for b, p in enumerate(batch):
        sl = slice(b * envs_per_pair, (b + 1) * envs_per_pair)
        idx0[sl], idx1[sl] = pairs[p]
        active[sl] = True
    return idx0, idx1, active


# ---- one chunk of steps ----------------------------------------------------------------------------------------------------
def _check_env(env, table):
    D0, D1 = env.model.obs_dims
    A0, A1 = env.model.act_dims
    if D0 != D1 or A0 != A1:
        raise ValueError("matches need a homogeneous match-up (one observation / action space for both sides); got ob_dim %d / %d, "
                         "ac_dim %d / %d" % (D0, D1, A0, A1))
    if (table.spec.ob_dim, table.spec.ac_dim) != (D0, A0):
        raise ValueError("snapshot table's policy (%d, %d) does not match the env (%d, %d)" % (table.spec.ob_dim, table.spec.ac_dim, D0, A0))
    _check_cfrc_mode(getattr(env, "cfrc_mode", "zero"))


def _check_cfrc_mode(cfrc_mode):
    if cfrc_mode != "zero":
        raise ValueError("matches run on the fused launch, which refuses cfrc_mode 'rne_post'")


def _refuse_fused_width(nlstm):
    """The fused match launches hold LSTM(128) checkpoints only; ``nlstm`` None: no recurrent checkpoint plays."""
    if nlstm is not None and nlstm != 128:
        raise ValueError("the fused match launch plays LSTM(128) policies only (got LSTM(%d)): use fused=False" % nlstm)


# What plays one agent: ``family`` 'ckpt_mlp' (SnapshotTable), 'ckpt_lstm' (LstmSnapshotTable), 'zoo_mlp' (policy_zoo.ZooTable) or
# 'zoo_lstm' (policy_zoo.ZooLstmTable), its ``table`` and ``width``, the columns of its recurrent state per env (c | h) or None.
Seat = collections.namedtuple("Seat", "family table width")

# Two seats resolved to their fused launch: the ``capi.Engine`` method ``entry``, its launch struct, the
# class of the struct that follows it (agent 1's zoo table) or None, the agent the LSTM table of a cross-family pairing plays
# (else None) and the width of the LSTM checkpoints that play (else None).
Pairing = collections.namedtuple("Pairing", "seats entry struct second lstm_side nlstm")

_ENTRY = {("ckpt_mlp", "ckpt_mlp"): "match_steps", ("ckpt_lstm", "ckpt_lstm"): "match_steps_lstm",
          ("ckpt_mlp", "zoo_mlp"): "match_steps_zoo", ("ckpt_mlp", "zoo_lstm"): "match_steps_zoo_lstm",
          ("ckpt_lstm", "zoo_lstm"): "match_steps_lstm_zoo_lstm", ("ckpt_mlp", "ckpt_lstm"): "match_steps_cross",
          ("ckpt_lstm", "ckpt_mlp"): "match_steps_cross", ("ckpt_lstm", "zoo_mlp"): "match_steps_lstm_zoo"}


def _seat(table):
    rec = bool(getattr(table, "recurrent", False))
    if hasattr(table, "spec"):
        return Seat("ckpt_lstm" if rec else "ckpt_mlp", table, 2 * table.spec.nlstm if rec else None)
    return Seat("zoo_lstm" if rec else "zoo_mlp", table, 2 * table.hidden if rec else None)


def match_pairing(table0, table1):
    """The :class:`Pairing` of agent 0 playing rows of ``table0`` against agent 1 playing rows of ``table1``; needs no env and no
    GPU.  Checkpoints of one family play from ONE table, zoo nets play agent 1 only; every other pair of tables is refused."""
    s0, s1 = _seat(table0), _seat(table1)
    if s0.family.startswith("zoo"):
        raise ValueError("policy-zoo nets play agent 1 only: agent 0 plays a SnapshotTable or an LstmSnapshotTable")
    if s0.family == s1.family and table0 is not table1:
        if s0.width != s1.width:
            raise ValueError("mixed LSTM widths are not supported (LSTM(%d) against LSTM(%d))" % (s0.width // 2, s1.width // 2))
        raise ValueError("two tables of one family do not play each other: both agents play rows of one table (play_matches)")
    entry = _ENTRY[s0.family, s1.family]
    struct, second = capi.FUSED_ENTRIES["sumo_" + entry]
    recurrent = [side for side, s in enumerate((s0, s1)) if s.family == "ckpt_lstm"]
    return Pairing((s0, s1), entry, struct, second, recurrent[0] if struct is capi.MatchCross else None,
                   (s0, s1)[recurrent[0]].table.spec.nlstm if recurrent else None)


def _check_state(seat, state, N):
    """Shape of ``state``, the recurrent state of the envs' agents that ``seat`` plays (None for an MLP seat)."""
    if seat.width is not None and (tuple(state.shape) != (N, seat.width) or not state.is_contiguous()):
        if seat.family == "zoo_lstm":
            raise ValueError("the zoo nets' recurrent state must be a contiguous float32 [%d][%d] tensor (c | h)" % (N, seat.width))
        raise ValueError("recurrent states must be two contiguous float32 [%d][%d] tensors (c | h)" % (N, seat.width))


def pairing_steps(env, pairing, states, idx0, idx1, score, quota, K, noise=None, fused=True):
    """K match steps of a :func:`match_pairing` on either path: what every step function below and the play drivers end in (the
    drivers look this name up per launch).  ``states``: the pair (agent 0's recurrent state or None, agent 1's or None), float32
    [N][seat width], read and updated in place; idx0 / idx1 are CUDA tensors (fused) or host arrays (step by step); the other
    arguments as :func:`match_steps_fused`.  The env is checked by the callers (:func:`_check_env`)."""
    for seat, state in zip(pairing.seats, states):
        _check_state(seat, state, env.num_envs)
    if fused:
        _refuse_fused_width(pairing.nlstm)
    (_steps_fused if fused else _steps_stepwise)(env, pairing, idx0, idx1, states, score, quota, K, noise)


def _fill_match(mo, pairing, states, sl):
    t = pairing.seats[0].table
    mo.params = t.params.data_ptr()
    mo.nsnap, mo.ob_dim, mo.ac_dim = t.capacity, t.spec.ob_dim, t.spec.ac_dim


def _fill_match_lstm(mo, pairing, states, sl):
    t = pairing.seats[0].table
    mo.proto, mo.nets_dev, mo.nsnap = C.addressof(t.proto), t.nets_dev.data_ptr(), t.capacity
    mo.state0 = states[0][sl].data_ptr()
    if pairing.second is None:                  # agent 1 plays the same table; a zoo net's state travels in the zoo struct
        mo.state1 = states[1][sl].data_ptr()


def _fill_match_cross(mo, pairing, states, sl):
    g = pairing.lstm_side
    lt, mt = pairing.seats[g].table, pairing.seats[1 - g].table
    mo.params = mt.params.data_ptr()
    mo.nsnap_mlp, mo.ob_dim, mo.ac_dim = mt.capacity, mt.spec.ob_dim, mt.spec.ac_dim
    mo.proto, mo.nets_dev, mo.nsnap_lstm = C.addressof(lt.proto), lt.nets_dev.data_ptr(), lt.capacity
    mo.state, mo.lstm_side = states[g][sl].data_ptr(), g


_FILL = {capi.Match: _fill_match, capi.MatchLstm: _fill_match_lstm, capi.MatchCross: _fill_match_cross}


def _steps_fused(env, pairing, idx0, idx1, states, score, quota, K, noise):
    """One fused match launch per env group: the pairing's launch struct, its own fields set by the filler of its class and the
    shared ones (indices, window, quota, noise, score) here, passed to the engine's ``pairing.entry`` (followed by agent 1's zoo
    table struct, with its state rows for zoo LSTM nets) with the group's env-side pointers; raises if the launch was cut short
    (``rollout_status``)."""
    zoo = pairing.seats[1]
    for g in range(env.groups):
        sl = env._gs(g)
        mo = pairing.struct()
        _FILL[pairing.struct](mo, pairing, states, sl)
        mo.idx0, mo.idx1 = idx0[sl].data_ptr(), idx1[sl].data_ptr()
        mo.T, mo.s0, mo.K, mo.quota = int(K), 0, int(K), int(quota)
        keep = None
        if noise is not None:
            keep = [n[:, sl].contiguous() if env.groups > 1 else n for n in noise]
            mo.noise0, mo.noise1 = keep[0].data_ptr(), keep[1].data_ptr()
        mo.score = score[sl].data_ptr()
        second = ()
        if pairing.second is not None:
            second = (zoo.table.struct() if zoo.width is None else zoo.table.struct(states[1][sl]),)
        E = env.engines[g]
        getattr(E, pairing.entry)(mo, *second, *env.env_ptrs(g), stream=env._stream())
        E.rollout_status()
        del keep


def match_steps_fused(env, table, idx0, idx1, score, quota, K, noise=None):
    """K match steps of every env in one ``sumo_match_steps`` launch per env group.  idx0 / idx1 int32 CUDA tensors [N],
    score int32 CUDA [N][3] (updated in place), noise None (deterministic) or a pair of float32 CUDA [K][N][A] tensors.  Raises
    if the launch was cut short (``rollout_status``)."""
    _check_env(env, table)
    pairing_steps(env, match_pairing(table, table), (None, None), idx0, idx1, score, quota, K, noise, True)


def _runs(idx):
    """(start, end, value) of the runs of equal consecutive entries of a host array."""
    cut = np.flatnonzero(np.diff(idx)) + 1
    starts = np.concatenate([[0], cut])
    ends = np.concatenate([cut, [len(idx)]])
    return [(int(s), int(e), int(idx[s])) for s, e in zip(starts, ends)]


def _steps_stepwise(env, pairing, idx0, idx1, states, score, quota, K, noise):
    """The step-by-step loop of every pairing: per step and side, that seat's ``forward(k, side, rows, noise rows or None, action
    rows, mask rows or None)`` for every run ``rows = slice(s, e)`` of envs that share row ``k`` of its table, then ``step_device``
    and the score update.  With a recurrent seat the previous step's done flags become float32 masks: a checkpoint LSTM is
    masked by its own side's, a zoo LSTM net by AGENT 0's (``policy_zoo._evaluate_against`` resets the opponent on them).  idx0 /
    idx1 are host arrays, each checked against its own seat's table."""
    import torch
    s0, s1 = pairing.seats
    idx0, idx1 = np.asarray(idx0, np.int64), np.asarray(idx1, np.int64)
    if min(idx0.min(), idx1.min()) < 0 or idx0.max() >= s0.table.capacity or idx1.max() >= s1.table.capacity:
        raise ValueError("snapshot index outside [0, %d) / [0, %d)" % (s0.table.capacity, s1.table.capacity))
    A, N = s0.table.spec.ac_dim, env.num_envs
    forward = [_FORWARD[s.family](env, s, state, A) for s, state in zip(pairing.seats, states)]
    masked = s0.width is not None or s1.width is not None
    mask_side = [0 if s.family == "zoo_lstm" else side for side, s in enumerate(pairing.seats)]
    acts = env.act_dev                          # the env's action buffer receives both actions, as in the fused launch
    act = [torch.empty((N, A), dtype=torch.float32, device=env.device) for _ in range(2)]
    runs = [_runs(idx0), _runs(idx1)]
    for t in range(int(K)):
        masks = [env.done_dev[:, side].to(torch.float32) if masked else None for side in range(2)]
        for side in range(2):
            for s, e, k in runs[side]:
                rows = slice(s, e)
                forward[side](k, side, rows, None if noise is None else noise[side][t, rows], act[side][rows],
                              masks[mask_side[side]][rows] if masked else None)
            acts[:, side, :A] = act[side]
        _, info, done, _, _, _ = env.step_device(acts)
        _score_step(score, info, done, quota)


def _mlp_side(env, seat, _state, _A):
    """``forward`` of :func:`_steps_stepwise` for a side played by a :class:`SnapshotTable`: one ``ppo_forward`` launch
    (``PPOModel.step``'s kernel) on the rows' observations of that side."""
    import torch
    from . import ppo_capi
    table = seat.table
    D, A = table.spec.ob_dim, table.spec.ac_dim
    L, st, obs = ppo_capi.lib(), env._stream(), env.obs_dev
    nlp = torch.empty(env.num_envs, dtype=torch.float32, device=env.device)

    def forward(k, side, rows, nz, out, _mask):
        ppo_capi.chk(L.ppo_forward(table.params[k].data_ptr(), obs[rows, side].data_ptr(), rows.stop - rows.start, obs.stride(0), D, A,
                                   ppo_capi.FWD_PI, ppo_capi.ptr(nz), None, out.data_ptr(), nlp[rows].data_ptr(), None, None, st))
    return forward


def _lstm_side(env, seat, state, _A):
    """The same for a side played by an :class:`LstmSnapshotTable` or a :class:`policy_zoo.ZooLstmTable` (its nets' policy branch,
    what ``ZooLSTMPolicy.act`` runs): one ``ppo_lstm_step`` launch (the kernel ``LstmPPOModel.step`` runs) on the rows of
    ``state``, masked by the done flags :func:`_steps_stepwise` hands over."""
    from . import ppo_capi
    nets, H = seat.table.nets, seat.width // 2
    L, st, obs = ppo_capi.lib(), env._stream(), env.obs_dev

    def forward(k, side, rows, nz, out, mask):
        S = state[rows]
        ppo_capi.chk(L.ppo_lstm_step(C.byref(nets[k]), obs[rows, side].data_ptr(), rows.stop - rows.start, obs.stride(0),
                                     mask.data_ptr(), S.data_ptr(), S.data_ptr() + 4 * H, 2 * H, ppo_capi.ptr(nz), None,
                                     out.data_ptr(), None, None, None, st))
    return forward


def _zoo_mlp_side(env, seat, _state, A):
    """The same for a side played by a :class:`policy_zoo.ZooTable`: one ``ppo_forward_filtered`` launch (what
    ``ZooMLPPolicy.act`` runs)."""
    import torch
    from . import ppo_capi
    zoo_table = seat.table
    Dz = zoo_table.ob_dim
    L, st, obs = ppo_capi.lib(), env._stream(), env.obs_dev
    nlp = torch.empty(env.num_envs, dtype=torch.float32, device=env.device)

    def forward(k, side, rows, nz, out, _mask):
        f = zoo_table.filt[k]
        ppo_capi.chk(L.ppo_forward_filtered(zoo_table.params[k].data_ptr(), obs[rows, side].data_ptr(), rows.stop - rows.start,
                                            obs.stride(0), Dz, A, ppo_capi.FWD_PI | ppo_capi.FWD_TANH, f[0].data_ptr(), f[1].data_ptr(),
                                            zoo_table.obs_clip, ppo_capi.ptr(nz), None, out.data_ptr(), nlp[rows].data_ptr(), None, None, st))
    return forward


_FORWARD = {"ckpt_mlp": _mlp_side, "ckpt_lstm": _lstm_side, "zoo_mlp": _zoo_mlp_side, "zoo_lstm": _lstm_side}


def match_steps_stepwise(env, table, idx0, idx1, score, quota, K, noise=None):
    """The same K steps on the step-by-step path: per step and side one ``ppo_forward`` launch (``PPOModel.step``'s kernel) for
    every run of envs that share a snapshot, then ``step_device`` and the score update.  idx0 / idx1 are host arrays."""
    _check_env(env, table)
    pairing_steps(env, match_pairing(table, table), (None, None), idx0, idx1, score, quota, K, noise, False)


def match_steps_fused_lstm(env, table, idx0, idx1, states, score, quota, K, noise=None):
    """:func:`match_steps_fused` for an :class:`LstmSnapshotTable`: one ``sumo_match_steps_lstm`` launch per env group.  ``states``
    is a pair of float32 CUDA [N][2 nlstm] tensors (c | h) per agent, read and updated in place.  LSTM(128) only."""
    _check_env(env, table)
    pairing_steps(env, match_pairing(table, table), states, idx0, idx1, score, quota, K, noise, True)


def match_steps_stepwise_lstm(env, table, idx0, idx1, states, score, quota, K, noise=None):
    """The same K steps of an :class:`LstmSnapshotTable` step by step: per step and side one ``ppo_lstm_step`` launch (the kernel
    ``LstmPPOModel.step`` runs) for every run of envs that share a snapshot, masked by that side's done flags of the previous step,
    then ``step_device`` and the score update.  idx0 / idx1 are host arrays; any LSTM width the step kernel is built for."""
    _check_env(env, table)
    pairing_steps(env, match_pairing(table, table), states, idx0, idx1, score, quota, K, noise, False)


def _check_zoo(env, table, zoo_table):
    _check_env(env, table)
    _check_zoo_family(table, zoo_table)
    _check_zoo_dims(table, zoo_table)


def _check_zoo_family(table, zoo_table):
    if getattr(table, "recurrent", False) and not getattr(zoo_table, "recurrent", False):
        raise ValueError("LSTM checkpoints do not play against zoo MLP nets in the fused launch (MLP(64,64) checkpoints only; LSTM "
                         "checkpoints play against zoo LSTM nets, a ZooLstmTable)")


def _check_zoo_dims(table, zoo_table):
    if zoo_table.ac_dim != table.spec.ac_dim or not 1 <= zoo_table.ob_dim <= table.spec.ob_dim:
        raise ValueError("zoo table (ob_dim %d, ac_dim %d) does not fit the env (%d, %d): a zoo MLP net reads the first ob_dim "
                         "observation columns" % (zoo_table.ob_dim, zoo_table.ac_dim, table.spec.ob_dim, table.spec.ac_dim))


def zoo_match_steps_fused(env, table, zoo_table, idx0, idx1, score, quota, K, noise=None):
    """K match steps of MLP checkpoints (agent 0: row idx0[e] of ``table``) against policy-zoo MLP nets (agent 1: row idx1[e] of
    ``zoo_table``, a :class:`policy_zoo.ZooTable`) in one ``sumo_match_steps_zoo`` launch per env group; arguments as
    :func:`match_steps_fused`."""
    _check_zoo(env, table, zoo_table)
    pairing_steps(env, match_pairing(table, zoo_table), (None, None), idx0, idx1, score, quota, K, noise, True)


def zoo_match_steps_stepwise(env, table, zoo_table, idx0, idx1, score, quota, K, noise=None):
    """The same K steps step by step: per step one ``ppo_forward`` launch for every run of envs that share a checkpoint, one
    ``ppo_forward_filtered`` launch (what ``ZooMLPPolicy.act`` runs) for every run that shares a zoo net, then ``step_device`` and
    the score update.  idx0 / idx1 are host arrays."""
    _check_zoo(env, table, zoo_table)
    pairing_steps(env, match_pairing(table, zoo_table), (None, None), idx0, idx1, score, quota, K, noise, False)


def _zoo_lstm_pairing(env, table, zoo_table, states):
    """Checks of the zoo LSTM match steps; returns the pairing and the state pair from ``states``: agent 1's tensor [N][2 * 64]
    for an MLP table, the pair (agent 0 [N][2 nlstm], agent 1 [N][2 * 64]) for an :class:`LstmSnapshotTable`."""
    _check_zoo(env, table, zoo_table)
    if not getattr(zoo_table, "recurrent", False):
        raise ValueError("zoo_lstm_match_steps_* need a policy_zoo.ZooLstmTable (zoo MLP nets play through zoo_match_steps_*)")
    return match_pairing(table, zoo_table), tuple(states) if getattr(table, "recurrent", False) else (None, states)


def zoo_lstm_match_steps_fused(env, table, zoo_table, idx0, idx1, states, score, quota, K, noise=None):
    """K match steps of checkpoints (agent 0: row idx0[e] of ``table``) against policy-zoo LSTM nets (agent 1: row idx1[e] of
    ``zoo_table``, a :class:`policy_zoo.ZooLstmTable`) in one launch per env group: ``sumo_match_steps_zoo_lstm`` for a
    :class:`SnapshotTable` (``states``: agent 1's float32 CUDA [N][128] tensor, c | h), ``sumo_match_steps_lstm_zoo_lstm`` for an
    :class:`LstmSnapshotTable` of LSTM(128) policies (``states``: the pair agent 0 [N][256], agent 1 [N][128]).  The states are
    read and updated in place; the other arguments as :func:`match_steps_fused`."""
    pairing_steps(env, *_zoo_lstm_pairing(env, table, zoo_table, states), idx0, idx1, score, quota, K, noise, True)


def zoo_lstm_match_steps_stepwise(env, table, zoo_table, idx0, idx1, states, score, quota, K, noise=None):
    """The same K steps step by step: per step, for every run of envs that share a checkpoint, one ``ppo_forward`` launch (MLP
    table) or one ``ppo_lstm_step`` launch masked by agent 0's done flags (LSTM table); for every run that shares a zoo net one
    ``ppo_lstm_step`` launch on its policy branch (what ``ZooLSTMPolicy.act`` runs), its state rows masked by AGENT 0's done flags
    of the previous step (``policy_zoo._evaluate_against`` resets the opponent on them); then ``step_device`` and the score
    update.  idx0 / idx1 are host arrays."""
    pairing_steps(env, *_zoo_lstm_pairing(env, table, zoo_table, states), idx0, idx1, score, quota, K, noise, False)


def _cross_pairing(env, mlp_table, lstm_table, lstm_side, state):
    """Checks of the cross-family match steps; returns the pairing of the seating and its state pair."""
    if getattr(mlp_table, "recurrent", False) or not getattr(lstm_table, "recurrent", False):
        raise ValueError("cross-family matches take a SnapshotTable (MLP(64,64)) and an LstmSnapshotTable, in this order")
    if lstm_side not in (0, 1):
        raise ValueError("lstm_side %r: 0 (agent 0 plays the LSTM table) or 1" % (lstm_side,))
    _check_env(env, mlp_table)
    _check_env(env, lstm_table)
    if lstm_side == 0:
        return match_pairing(lstm_table, mlp_table), (state, None)
    return match_pairing(mlp_table, lstm_table), (None, state)


def cross_match_steps_fused(env, mlp_table, lstm_table, lstm_side, idx0, idx1, state, score, quota, K, noise=None):
    """K match steps of MLP(64,64) checkpoints against LSTM(128) checkpoints in one ``sumo_match_steps_cross`` launch per env
    group: agent ``lstm_side`` plays row idx_g[e] of ``lstm_table`` on ``state`` (float32 CUDA [N][256], c | h, read and updated
    in place), the other agent row idx_g[e] of ``mlp_table``.  The other arguments as :func:`match_steps_fused`."""
    pairing_steps(env, *_cross_pairing(env, mlp_table, lstm_table, lstm_side, state), idx0, idx1, score, quota, K, noise, True)


def cross_match_steps_stepwise(env, mlp_table, lstm_table, lstm_side, idx0, idx1, state, score, quota, K, noise=None):
    """The same K steps step by step: the launches of :func:`match_steps_stepwise` for the MLP side and of
    :func:`match_steps_stepwise_lstm` for agent ``lstm_side`` (any LSTM width the step kernel is built for).  idx0 / idx1 are
    host arrays."""
    pairing_steps(env, *_cross_pairing(env, mlp_table, lstm_table, lstm_side, state), idx0, idx1, score, quota, K, noise, False)


def _lstm_zoo_pairing(env, lstm_table, zoo_table, state0):
    if not getattr(lstm_table, "recurrent", False) or getattr(zoo_table, "recurrent", False):
        raise ValueError("lstm_zoo_match_steps_* take an LstmSnapshotTable and a policy_zoo.ZooTable (zoo MLP nets)")
    _check_env(env, lstm_table)
    _check_zoo_dims(lstm_table, zoo_table)
    return match_pairing(lstm_table, zoo_table), (state0, None)


def lstm_zoo_match_steps_fused(env, lstm_table, zoo_table, idx0, idx1, state0, score, quota, K, noise=None):
    """K match steps of LSTM(128) checkpoints (agent 0: row idx0[e] of ``lstm_table`` on ``state0``, float32 CUDA [N][256], read
    and updated in place) against policy-zoo MLP nets (agent 1: row idx1[e] of ``zoo_table``) in one
    ``sumo_match_steps_lstm_zoo`` launch per env group; the other arguments as :func:`match_steps_fused`."""
    pairing_steps(env, *_lstm_zoo_pairing(env, lstm_table, zoo_table, state0), idx0, idx1, score, quota, K, noise, True)


def lstm_zoo_match_steps_stepwise(env, lstm_table, zoo_table, idx0, idx1, state0, score, quota, K, noise=None):
    """The same K steps step by step: per step one ``ppo_lstm_step`` launch masked by agent 0's done flags for every run of envs
    that share a checkpoint, one ``ppo_forward_filtered`` launch for every run that shares a zoo net, then ``step_device`` and the
    score update.  idx0 / idx1 are host arrays."""
    pairing_steps(env, *_lstm_zoo_pairing(env, lstm_table, zoo_table, state0), idx0, idx1, score, quota, K, noise, False)


def match_steps(env, table, idx0, idx1, states, score, quota, K, noise=None, fused=True):
    """K match steps of either table kind on either path: ``states`` is the pair of recurrent state tensors of an
    :class:`LstmSnapshotTable` (ignored for MLP tables); idx0 / idx1 are CUDA tensors (fused) or host arrays (step by step)."""
    _check_env(env, table)
    pairing_steps(env, match_pairing(table, table), states if getattr(table, "recurrent", False) else (None, None), idx0, idx1, score,
                 quota, K, noise, fused)


def _score_step(score, info, done, quota):
    import torch
    fin = done[:, 0] != 0
    f = info[:, :, 7].to(torch.int64)
    w0 = (f[:, 0] & 1) != 0
    w1 = ((f[:, 1] & 1) != 0) & ~w0
    slot = torch.where(w0, 0, torch.where(w1, 1, 2))
    inc = (fin & (score.sum(1) < quota)).to(score.dtype)
    score.scatter_add_(1, slot[:, None], inc[:, None])


# ---- match-ups -------------------------------------------------------------------------------------------------------------
def _play(env, pairing, pairs, rounds_per_env, envs_per_pair, deterministic, seed, adjust_z, chunk, fused):
    """What the play drivers share once their pairing is resolved: the rows of every pair checked against the table of their own
    seat, the quota and the chunk, the fused launch's LSTM width, and :func:`_play_batches` on :func:`pairing_steps` with fresh
    all-zero recurrent states per batch (``LstmPPOModel.initial_state``)."""
    import torch
    s0, s1 = pairing.seats
    row_ok = lambda seat, k: 0 <= k < seat.table.capacity and (seat.family.startswith("zoo") or bool(seat.table.filled[k]))
    pairs = [(int(i), int(j)) for i, j in pairs]
    for i, j in pairs:
        if not (row_ok(s0, i) and row_ok(s1, j)):
            raise ValueError("pair (%d, %d) refers to an empty or non-existent %s" %
                             (i, j, "checkpoint / zoo row" if s1.family.startswith("zoo") else "snapshot row"))
    rounds_per_env, envs_per_pair, chunk = int(rounds_per_env), int(envs_per_pair), int(chunk)
    if rounds_per_env < 1 or chunk < 1:
        raise ValueError("rounds_per_env and chunk must be >= 1")
    if fused:
        _refuse_fused_width(pairing.nlstm)
    new_states = lambda: tuple(None if s.width is None else torch.zeros((env.num_envs, s.width), dtype=torch.float32, device=env.device)
                               for s in pairing.seats)
    steps = lambda idx0, idx1, states, score, noise: pairing_steps(env, pairing, states, idx0, idx1, score, rounds_per_env, chunk, noise,
                                                                  fused)
    return _play_batches(env, s0.table.spec.ac_dim, pairs, rounds_per_env, envs_per_pair, deterministic, seed, adjust_z, chunk, fused,
                         new_states, steps)


def play_matches(env, table, pairs, rounds_per_env, envs_per_pair, deterministic=False, seed=0, adjust_z=EVAL_ADJUST_Z, chunk=64,
                 fused=True):
    """Plays every match-up ``pairs[p] = (i, j)`` (snapshot i as agent 0 against snapshot j as agent 1 of ``table``, a
    :class:`SnapshotTable` or an :class:`LstmSnapshotTable`) on ``envs_per_pair`` envs, ``rounds_per_env`` finished episodes per
    env.  Pairs are played in batches of contiguous env blocks; each batch resets the envs seeded (``seed`` + batch number * N +
    env), zeroes both sides' recurrent states (LSTM tables) and runs ``chunk``-step launches until every env of the batch has its
    quota.  ``adjust_z`` is imposed on every agent for the games and the env's value restored afterwards (None:
    leave it).  Returns one dict per pair: wins, losses, draws, rounds (== envs_per_pair * rounds_per_env), env_steps."""
    _check_env(env, table)
    return _play(env, match_pairing(table, table), pairs, rounds_per_env, envs_per_pair, deterministic, seed, adjust_z, chunk, fused)


def play_cross_matches(env, table0, table1, pairs, rounds_per_env, envs_per_pair, deterministic=False, seed=0, adjust_z=EVAL_ADJUST_Z,
                       chunk=64, fused=True):
    """:func:`play_matches` across the families: ``pairs[p] = (i, j)`` is row i of ``table0`` as agent 0 against row j of
    ``table1`` as agent 1, where exactly one of the two tables is an :class:`LstmSnapshotTable` and the other a
    :class:`SnapshotTable` (either seating).  The recurrent agent's state is zeroed per batch.  Same batching, seeding, quota
    and return value as :func:`play_matches`; ``fused=False`` plays the same games step by step (any LSTM width)."""
    if bool(getattr(table0, "recurrent", False)) == bool(getattr(table1, "recurrent", False)):
        raise ValueError("play_cross_matches takes one SnapshotTable (MLP(64,64)) and one LstmSnapshotTable; two tables of one "
                         "family play through play_matches")
    _check_env(env, table0)
    _check_env(env, table1)
    return _play(env, match_pairing(table0, table1), pairs, rounds_per_env, envs_per_pair, deterministic, seed, adjust_z, chunk, fused)


def _play_batches(env, A, pairs, rounds_per_env, envs_per_pair, deterministic, seed, adjust_z, chunk, fused, new_states, steps):
    """The batching behind :func:`_play`: pairs in batches of contiguous env blocks (:func:`plan_batches`,
    :func:`env_assignment`); per batch a seeded reset, fresh recurrent states (``new_states()``) and
    ``steps(idx0, idx1, states, score, noise)`` launches of ``chunk`` steps -- indices as CUDA tensors when ``fused``, else host
    arrays -- until every env of the batch has its quota."""
    import torch
    N = env.num_envs
    batches = plan_batches(len(pairs), envs_per_pair, N)
    max_launches = -(-rounds_per_env * (env.model.timestep_limit + 1) // chunk) + 1   # every episode ends by the time limit
    gen = torch.Generator(device=env.device)
    gen.manual_seed(int(seed))
    out = [None] * len(pairs)
    prev_adjust, prev_seeds = getattr(env, "adjust_z", 0.0), env.seeds.copy()
    change_z = adjust_z is not None and float(adjust_z) != prev_adjust
    if change_z:
        env.set_adjust_z(adjust_z)
    try:
        for bn, batch in enumerate(batches):
            idx0_h, idx1_h, active = env_assignment(pairs, batch, envs_per_pair, N)
            idx0 = torch.from_numpy(idx0_h).to(env.device)
            idx1 = torch.from_numpy(idx1_h).to(env.device)
            act_t = torch.from_numpy(active).to(env.device)
            score = torch.zeros((N, 3), dtype=torch.int32, device=env.device)
            env.seeds = np.uint64(seed) + np.uint64(bn * N) + np.arange(N, dtype=np.uint64)
            env._needs_seed = True
            env.reset_device()
            states = new_states()
            launches = 0
            while True:
                noise = None if deterministic else tuple(torch.randn((chunk, N, A), generator=gen, device=env.device) for _ in range(2))
                steps(idx0 if fused else idx0_h, idx1 if fused else idx1_h, states, score, noise)
                launches += 1
                if not bool((score.sum(1)[act_t] < rounds_per_env).any()):
                    break
                if launches >= max_launches:
                    raise RuntimeError("matches did not finish within %d launches of %d steps" % (launches, chunk))
            sc = score.cpu().numpy().astype(np.int64)
            for b, p in enumerate(batch):
                s = sc[b * envs_per_pair:(b + 1) * envs_per_pair].sum(0)
                out[p] = dict(wins=int(s[0]), losses=int(s[1]), draws=int(s[2]), rounds=int(s.sum()),
                              env_steps=launches * chunk * envs_per_pair)
    finally:
        env.seeds = prev_seeds
        if change_z:
            torch.cuda.synchronize(env.device)
            env.set_adjust_z(prev_adjust)
    return out


def play_against_zoo(env, table, zoo_table, pairs, rounds_per_env, envs_per_pair, deterministic=True, seed=0, adjust_z=EVAL_ADJUST_Z,
                     chunk=64, fused=True, cross_family=False):
    """:func:`play_matches` with agent 1 played by policy-zoo nets: ``pairs[p] = (i, j)`` is checkpoint row i of ``table`` (a
    :class:`SnapshotTable`, or an :class:`LstmSnapshotTable` against zoo LSTM nets) as agent 0 against net j of ``zoo_table`` (a
    :class:`policy_zoo.ZooTable` or :class:`policy_zoo.ZooLstmTable`) as agent 1 -- the games of the reference's
    eval_robosumo_against_fix.py:196-230 (deterministic by default, as there).  Recurrent states (the zoo LSTM nets', the LSTM
    checkpoints') are allocated and zeroed per batch.  Same batching, seeding, quota and return value as :func:`play_matches`;
    ``fused=False`` plays the same games step by step (bit-identical envs and scores).  ``cross_family=True`` also plays an
    :class:`LstmSnapshotTable` against a :class:`policy_zoo.ZooTable` (``sumo_match_steps_lstm_zoo``); the default refuses it."""
    if cross_family:
        _check_env(env, table)
        _check_zoo_dims(table, zoo_table)
    else:
        _check_zoo(env, table, zoo_table)
    return _play(env, match_pairing(table, zoo_table), pairs, rounds_per_env, envs_per_pair, deterministic, seed, adjust_z, chunk, fused)


def _make_env(env_id, num_env, seed, env):
    if env is not None:
        return env, False
    from .vec_env import make_vec_env
    return make_vec_env(env_id, num_env, seed), True


def _spec_of(env):
    return policies.PolicySpec(env.observation_space[0].shape[0], env.action_space[0].shape[0], value_network="copy", activation="relu")


def _kind_name(kind):
    return "MLP(64,64)" if kind[0] == "mlp" else "LSTM(%d)" % kind[1]


def _table_of(kind, env, paths):
    """The snapshot table of a checkpoint kind (:func:`checkpoint_kind`) filled from ``paths``."""
    if kind[0] == "lstm":
        from .lstm_model import LstmSpec
        spec = LstmSpec(env.observation_space[0].shape[0], env.action_space[0].shape[0], kind[1])
        return LstmSnapshotTable.from_checkpoints(spec, paths, env.device)
    return SnapshotTable.from_checkpoints(_spec_of(env), paths, env.device)


def _network(kind):
    return dict(network=kind[0], nlstm=kind[1])


def compare_history_versions(path1, path2, trials, num_env=256, deterministic=False, seed=0, adjust_z=EVAL_ADJUST_Z,
                             env_id="RoboSumo-Ant-vs-Ant-v0", chunk=64, env=None, fused=True, cross_family=False):
    """compare_history_version.py on the GPU: version i of run ``path1`` (agent 0) against version i of ``path2`` (agent 1),
    ``trials`` games each.  MLP and LSTM runs are told apart by their first checkpoint; both runs must hold the same kind, unless
    ``cross_family`` is set: then an MLP(64,64) run and an LSTM run play each other in the seating given
    (:func:`play_cross_matches`; mixed LSTM widths stay refused).
    Returns dict(versions=[(id1, id2)], win_rate=[P1 wins / trials], results=[play_matches dicts], network='mlp' | 'lstm',
    nlstm=LSTM width or None); a cross-family comparison returns network='cross', nlstm of the recurrent run and
    networks=[dict(network, nlstm) of P1, of P2]."""
    pv = pair_versions(list_checkpoints(path1), list_checkpoints(path2))
    if not pv:
        raise ValueError("no checkpoints to compare")
    paths = [os.path.join(checkpoint_dir(path1), a) for a, _ in pv] + [os.path.join(checkpoint_dir(path2), b) for _, b in pv]
    k1, k2 = checkpoint_kind(paths[0]), checkpoint_kind(paths[len(pv)])
    cross = bool(cross_family) and {k1[0], k2[0]} == {"mlp", "lstm"}
    if k1 != k2 and not cross:
        raise ValueError("P1 holds %s checkpoints and P2 %s checkpoints: both runs must use the same network (MLP-vs-LSTM and "
                         "mixed LSTM widths are not supported)" % (_kind_name(k1), _kind_name(k2)))
    nlstm = k1[1] if k1[0] == "lstm" else k2[1]
    if cross and fused:
        _refuse_fused_width(nlstm)
    env, own = _make_env(env_id, num_env, seed, env)
    try:
        n = len(pv)
        epp, rpe = split_trials(trials, env.num_envs)
        kw = dict(deterministic=deterministic, seed=seed, adjust_z=adjust_z, chunk=chunk, fused=fused)
        if cross:
            res = play_cross_matches(env, _table_of(k1, env, paths[:n]), _table_of(k2, env, paths[n:]), [(k, k) for k in range(n)],
                                     rpe, epp, **kw)
        else:
            res = play_matches(env, _table_of(k1, env, paths), [(k, n + k) for k in range(n)], rpe, epp, **kw)
    finally:
        if own:
            env.close()
    out = dict(versions=pv, win_rate=[r["wins"] / float(trials) for r in res], results=res)
    if cross:
        return dict(out, network="cross", nlstm=nlstm, networks=[_network(k1), _network(k2)])
    return dict(out, **_network(k1))


def round_robin(path, interval, trials, num_env=256, deterministic=False, seed=0, adjust_z=EVAL_ADJUST_Z,
                env_id="RoboSumo-Ant-vs-Ant-v0", chunk=64, env=None, fused=True):
    """Every ``interval``-th version of one run (sorted, ``00000`` excluded) against every other, both seatings, ``trials``
    games per ordered pair.  Returns dict(versions, win, draw, loss): [V][V] rates of version i as agent 0 against version j
    as agent 1 (NaN on the diagonal), results (play_matches dicts by (i, j)) and network / nlstm as
    :func:`compare_history_versions`."""
    interval = int(interval)
    if interval < 1:
        raise ValueError("interval must be >= 1")
    ids = list_checkpoints(path)[::interval]
    if len(ids) < 2:
        raise ValueError("a round robin needs at least two versions (got %d)" % len(ids))
    paths = [os.path.join(checkpoint_dir(path), c) for c in ids]
    kind = checkpoint_kind(paths[0])
    env, own = _make_env(env_id, num_env, seed, env)
    try:
        table = _table_of(kind, env, paths)
        V = len(ids)
        pairs = [(i, j) for i in range(V) for j in range(V) if i != j]
        epp, rpe = split_trials(trials, env.num_envs)
        res = play_matches(env, table, pairs, rpe, epp, deterministic=deterministic, seed=seed, adjust_z=adjust_z, chunk=chunk,
                           fused=fused)
    finally:
        if own:
            env.close()
    M = {k: np.full((V, V), np.nan) for k in ("win", "draw", "loss")}
    for (i, j), r in zip(pairs, res):
        M["win"][i, j], M["draw"][i, j], M["loss"][i, j] = r["wins"] / trials, r["draws"] / trials, r["losses"] / trials
    return dict(versions=ids, results={p: r for p, r in zip(pairs, res)}, **M, **_network(kind))


def select_checkpoints(ids, start=0, interval=1):
    """The checkpoint ids eval_robosumo_against_fix.py evaluates: sorted, from ``start`` on, every ``interval``-th number."""
    start, interval = int(start), int(interval)
    if interval < 1:
        raise ValueError("interval must be >= 1")
    return [c for c in sorted(int(i) for i in ids) if c >= start and (c - start) % interval == 0]


def plan_zoo_evaluation(n_checkpoints, n_opponents, trials, num_env):
    """The pure part of :func:`evaluate_history_against_zoo`: every (checkpoint c, opponent o) pair, checkpoint-major, gets
    ``envs_per_pair`` contiguous envs that play ``rounds_per_env`` games each (:func:`split_trials`: their product is ``trials``);
    pairs fill the envs batch by batch (:func:`plan_batches`).  Returns dict(pairs, envs_per_pair, rounds_per_env, blocks) with
    ``blocks[p] = (batch number, first env, end env)`` of pair p."""
    if n_checkpoints < 1 or n_opponents < 1:
        raise ValueError("need at least one checkpoint and one opponent")
    epp, rpe = split_trials(trials, num_env)
    pairs = [(c, o) for c in range(n_checkpoints) for o in range(n_opponents)]
    blocks = [None] * len(pairs)
    for bn, batch in enumerate(plan_batches(len(pairs), epp, num_env)):
        for b, p in enumerate(batch):
            blocks[p] = (bn, b * epp, (b + 1) * epp)
    return dict(pairs=pairs, envs_per_pair=epp, rounds_per_env=rpe, blocks=blocks)


def group_zoo_opponents(kinds):
    """The pure grouping of :func:`evaluate_history_against_zoo`: ``kinds[k]`` in {'mlp', 'lstm'} is the family of opponent file k.
    Returns the non-empty groups in the order MLP, LSTM as ``[(kind, [positions in the input])]`` -- each group plays in launches
    of its own, its opponents numbered 0 .. in its own zoo table."""
    bad = [k for k in kinds if k not in ("mlp", "lstm")]
    if bad:
        raise ValueError("unknown zoo opponent kind %r" % bad[0])
    return [(kind, pos) for kind, pos in (("mlp", [i for i, k in enumerate(kinds) if k == "mlp"]),
                                          ("lstm", [i for i, k in enumerate(kinds) if k == "lstm"])) if pos]


def plan_mixed_zoo_evaluation(n_checkpoints, kinds, trials, num_env):
    """:func:`plan_zoo_evaluation` per opponent family: ``[dict(kind, opponents=[input positions], plan)]`` for the groups of
    :func:`group_zoo_opponents`."""
    return [dict(kind=kind, opponents=pos, plan=plan_zoo_evaluation(n_checkpoints, len(pos), trials, num_env))
            for kind, pos in group_zoo_opponents(kinds)]


def merge_zoo_results(ids, groups, group_results):
    """One result table ``{(checkpoint id, opponent position in the caller's list): dict}`` from the per-group results
    (``group_results[g][p]`` belongs to pair ``groups[g]['plan']['pairs'][p]`` = (checkpoint c, opponent o of the group))."""
    out = {}
    for grp, res in zip(groups, group_results):
        for (c, o), r in zip(grp["plan"]["pairs"], res):
            n = float(r["rounds"])
            out[(ids[c], grp["opponents"][o])] = dict(win=r["wins"] / n, draw=r["draws"] / n, lose=r["losses"] / n, rounds=r["rounds"],
                                                      env_steps=r["env_steps"])
    return {key: out[key] for key in sorted(out, key=lambda key: (ids.index(key[0]), key[1]))}


def evaluate_history_against_zoo(path, opponent_paths, trials, start=0, interval=1, num_env=256, deterministic=True, fused=True, seed=0,
                                 adjust_z=EVAL_ADJUST_Z, env_id="RoboSumo-Ant-vs-Ant-v0", chunk=64, env=None, cross_family=False):
    """eval_robosumo_against_fix.py on the fused launch: every selected checkpoint of run ``path`` (:func:`select_checkpoints` of
    all of its saved versions) as agent 0 against every policy-zoo file of ``opponent_paths`` as agent 1, exactly ``trials``
    games per (checkpoint, opponent), all match-ups batched over the envs (:func:`plan_zoo_evaluation`) instead of one checkpoint
    after the other.  Each opponent file's family (MLP / LSTM) is read from its length; the MLP files and the LSTM files play in
    launches of their own (:func:`plan_mixed_zoo_evaluation`) and the results come back in the caller's opponent order.  The run's
    checkpoint kind is read with :func:`checkpoint_kind`: MLP(64,64) runs face both families, LSTM runs zoo LSTM files only
    unless ``cross_family`` is set (then their MLP files play too, :func:`play_against_zoo`).
    Returns dict(checkpoints=[ids], opponents=[paths], results={(id, k): dict(win, draw, lose, rounds, env_steps)}) with rates
    over ``rounds == trials`` games against opponent k, plus the families that met: network / nlstm of the run and
    opponent_networks=['mlp' | 'lstm' per opponent]."""
    from .policy_zoo import ZooLstmTable, ZooTable, zoo_file_kind
    if isinstance(opponent_paths, (str, os.PathLike)):
        opponent_paths = [opponent_paths]
    opponent_paths = [str(p) for p in opponent_paths]
    ck = checkpoint_dir(path)
    ids = select_checkpoints([f for f in os.listdir(ck) if f.isdigit() and os.path.isfile(os.path.join(ck, f))], start, interval)
    if not ids:
        raise ValueError("no checkpoints to evaluate in %s" % ck)
    ck_paths = [os.path.join(ck, "%.5i" % c) for c in ids]
    kind = checkpoint_kind(ck_paths[0])
    env, own = _make_env(env_id, num_env, seed, env)
    try:
        table = _table_of(kind, env, ck_paths)
        A = table.spec.ac_dim
        flats = [np.load(os.path.expanduser(p), allow_pickle=False) for p in opponent_paths]
        opp_kinds = [zoo_file_kind(f.size, A) for f in flats]
        groups = plan_mixed_zoo_evaluation(len(ids), opp_kinds, trials, env.num_envs)
        res = []
        for grp in groups:
            zoo_table = (ZooLstmTable if grp["kind"] == "lstm" else ZooTable)([flats[k] for k in grp["opponents"]], A, env.device)
            plan = grp["plan"]
            res.append(play_against_zoo(env, table, zoo_table, plan["pairs"], plan["rounds_per_env"], plan["envs_per_pair"],
                                        deterministic=deterministic, seed=seed, adjust_z=adjust_z, chunk=chunk, fused=fused,
                                        cross_family=cross_family))
    finally:
        if own:
            env.close()
    return dict(checkpoints=ids, opponents=opponent_paths, results=merge_zoo_results(ids, groups, res), opponent_networks=opp_kinds,
                **_network(kind))
