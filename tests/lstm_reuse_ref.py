"""Plain-numpy references for opponent-data reuse by a recurrent learner: the recurrent PPO loss with a ROW MASK (a float64
restatement of oracle/ppo_oracle.py::lstm_ppo_loss_and_grads whose means run over the valid rows) and the batch assembly of
alg_ppo.assemble_recurrent_update_batch.  tests/test_recurrent_reuse_cpu.py checks the first against the oracle function (all rows
valid) and against central finite differences of its own loss."""
import numpy as np

from oracle import ppo_oracle as po


def masked_loss_and_grads(params, obs, masks, actions, advs, returns, oldneglogp, is_weight, valid, S0, cliprange, ent_coef, vf_coef,
                          dtype=np.float64):
    """``po.lstm_ppo_loss_and_grads`` with ``valid`` [T, n] of 0 / 1: an invalid row stays in the recurrence (its observation and mask
    drive the state as before) and leaves the loss -- policy term, value term, approxkl and clipfrac are means over the valid rows
    (count = max(sum valid, 1)); whatever an invalid row holds (NaN included) reaches nothing.  The value term stays unweighted by
    ``is_weight``.  Returns (loss, stats[5], grads list, final state, number of valid rows)."""
    wx, wh, b, pw, pb, logstd, vw, vb = [np.asarray(x, dtype) for x in params]
    obs, masks, A_ = np.asarray(obs, dtype), np.asarray(masks, dtype), np.asarray(actions, dtype)
    adv, R, old, w = (np.asarray(v, dtype) for v in (advs, returns, oldneglogp, is_weight))
    T, n, _ = obs.shape
    H = wh.shape[0]
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    c, h = np.asarray(S0[:, :H], dtype).copy(), np.asarray(S0[:, H:], dtype).copy()
    cache = []
    lat = np.zeros((T, n, H), dtype)
    for t in range(T):
        m = masks[t][:, None]
        cp, hp = c * (1 - m), h * (1 - m)
        z = obs[t] @ wx + hp @ wh + b
        i, f, o, u = sig(z[:, :H]), sig(z[:, H:2 * H]), sig(z[:, 2 * H:3 * H]), np.tanh(z[:, 3 * H:])
        c = f * cp + i * u
        tc = np.tanh(c)
        h = o * tc
        cache.append((cp, hp, i, f, o, u, tc))
        lat[t] = h
    N = T * n
    vmask = np.asarray(valid, dtype).reshape(N) != 0
    cnt = max(int(vmask.sum()), 1)
    L = lat.reshape(N, H)
    mean = L @ pw + pb
    value = (L @ vw + vb)[:, 0]
    Af = A_.reshape(N, -1)
    # the per-row inputs of invalid rows are replaced by harmless numbers before any arithmetic: they leave every sum below
    clean = lambda x, fill: np.where(vmask, x.reshape(N), fill)
    advf, Rf, oldf, wf = clean(adv, 0.0), clean(R, 0.0), clean(old, 0.0), clean(w, 0.0)
    std = np.exp(logstd)
    nlp = po.neglogp(mean, logstd, Af)
    ent = np.sum(logstd + 0.5 * np.log(2.0 * np.pi * np.e))
    vsum = lambda x: np.sum(np.where(vmask, x, 0.0))
    vf_loss = 0.5 * vsum(np.square(value - Rf)) / cnt
    ratio = np.exp(oldf - nlp)
    nanmask = np.isnan(ratio)
    ratio = np.where(nanmask, 2.0, ratio)
    l1 = -advf * ratio
    l2 = -advf * np.clip(ratio, 1.0 - cliprange, 1.0 + cliprange)
    pg_loss = vsum(wf * np.maximum(l1, l2)) / cnt
    approxkl = vsum(nlp - oldf) / cnt
    clipfrac = vsum((np.abs(ratio - 1.0) > cliprange).astype(dtype)) / cnt
    loss = pg_loss - ent * ent_coef + vf_loss * vf_coef
    in_clip = (ratio >= 1.0 - cliprange) & (ratio <= 1.0 + cliprange)
    d_l1 = (l1 >= l2).astype(dtype)
    dratio = np.where(nanmask | ~vmask, 0.0, wf / cnt * (d_l1 * (-advf) + (1.0 - d_l1) * (-advf) * in_clip))
    dnlp = -dratio * ratio
    zz = (Af - mean) / std
    dmean = dnlp[:, None] * (-(zz / std))
    dlogstd = np.sum(dnlp[:, None] * (1.0 - zz * zz), axis=0, keepdims=True) - ent_coef * np.ones_like(logstd)
    dvalue = np.where(vmask, vf_coef * (value - Rf) / cnt, 0.0)
    g_pw, g_pb = L.T @ dmean, dmean.sum(0)
    g_vw, g_vb = L.T @ dvalue[:, None], np.array([dvalue.sum()])
    dlat = (dmean @ pw.T + dvalue[:, None] @ vw.T).reshape(T, n, H)
    g_wx, g_wh, g_b = np.zeros_like(wx), np.zeros_like(wh), np.zeros_like(b)
    dh, dc = np.zeros((n, H), dtype), np.zeros((n, H), dtype)
    for t in range(T - 1, -1, -1):
        cp, hp, i, f, o, u, tc = cache[t]
        dht = dlat[t] + dh
        do = dht * tc
        dct = dc + dht * o * (1.0 - tc * tc)
        dz = np.concatenate([dct * u * i * (1 - i), dct * cp * f * (1 - f), do * o * (1 - o), dct * i * (1 - u * u)], axis=1)
        g_wx += obs[t].T @ dz
        g_wh += hp.T @ dz
        g_b += dz.sum(0)
        m = masks[t][:, None]
        dh = (dz @ wh.T) * (1 - m)
        dc = dct * f * (1 - m)
    stats = np.array([pg_loss, vf_loss, ent, approxkl, clipfrac])
    return loss, stats, [g_wx, g_wh, g_b, g_pw, g_pb, dlogstd, g_vw, g_vb], np.concatenate([c, h], axis=1), int(vmask.sum())


def masked_normalize_advantages(returns, values, valid):
    """model.py:180-185 over the valid rows (float32 subtraction, float64 moments, population std as the kernels take it); 0 on
    invalid rows; all zeros without a valid row."""
    returns, values = np.asarray(returns, np.float32), np.asarray(values, np.float32)
    v = np.asarray(valid) != 0
    out = np.zeros(returns.shape, np.float32)
    if not v.any():
        return out
    adv = (returns - values)[v].astype(np.float64)
    mean = adv.mean()
    var = max((adv * adv).mean() - mean * mean, 0.0)
    out[v] = ((returns - values)[v] - np.float32(mean)) / (np.float32(np.sqrt(var)) + np.float32(1e-8))
    return out


def recurrent_update_batch(obs, returns, masks, actions, values, neglogpacs, rewards, off_policy_ratio, total_ratio, states0, shadow0, *,
                           nenv, neglogp_threshold, use_opponent_data, vgap=None, version_gap=None):
    """alg_ppo.assemble_recurrent_update_batch restated with loops: sequences of agent 0 first, then agent 1's when reuse is on;
    per row ``valid`` and ``weights``.  Arrays are [2, nenv * T, ...] env-major (the ratios [nenv * T])."""
    rows = returns.shape[1]
    usable = [k for k in range(rows) if neglogpacs[1][k] < neglogp_threshold]
    use_opp = not (vgap is not None and version_gap is not None and version_gap > vgap)
    agents = [0, 1] if use_opp else [0]
    arrs = dict(obs=obs, returns=returns, masks=masks, actions=actions, values=values, neglogpacs=neglogpacs, rewards=rewards)
    out = {k: np.concatenate([x[a] for a in agents], axis=0) for k, x in arrs.items()}
    out["states"] = np.concatenate([states0, shadow0], axis=0) if use_opp else states0
    valid, weights = [1.0] * rows, [1.0] * rows
    if use_opp:
        for k in range(rows):
            ok = k in usable
            valid.append(1.0 if ok else 0.0)
            if not ok:
                weights.append(0.0)
            elif use_opponent_data == "direct":
                weights.append(1.0)
            elif use_opponent_data == "off_policy":
                weights.append(float(off_policy_ratio[k]))
            elif use_opponent_data == "both":
                weights.append(float(total_ratio[k]))
            else:
                raise ValueError(use_opponent_data)
    out.update(valid=np.asarray(valid, np.float32), weights=np.asarray(weights, np.float32), nseq=len(agents) * nenv,
               usable_index=np.asarray(usable, np.int64), useful_ratio=len(usable) / float(rows))
    return out
