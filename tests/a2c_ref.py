"""Float64 restatement of the reference's A2C loss (ActorCriticModel, model.py:257-310) and its gradient w.r.t. the 13 parameter
tensors, by hand-written backprop over oracle/ppo_oracle.py's forward pass (checked by finite differences in test_a2c_cpu.py).
    pg = mean(w * adv * neglogp(a)),  vf = 0.5 * mean(w * (v - R)^2),  loss = pg - ent_coef * entropy + vf_coef * vf
``advs`` are the normalised advantages (po.normalize_advantages)."""
import numpy as np

from oracle import ppo_oracle as po


def a2c_loss_and_grads(params, obs, actions, advs, returns, is_weight, ent_coef, vf_coef, dtype=np.float64):
    """Returns (loss, stats [pg_loss, vf_loss, entropy], sums [sum w adv nlp, sum 0.5 w (v-R)^2, sum w], grads list)."""
    p = [np.asarray(x, dtype) for x in params]
    A = np.asarray(actions, dtype)
    adv, R, w = (np.asarray(v, dtype) for v in (advs, returns, is_weight))
    n = A.shape[0]
    mean, value, (x, h1, h2, g1, g2) = po.forward(p, obs, dtype)
    logstd = p[10]
    std = np.exp(logstd)
    nlp = po.neglogp(mean, logstd, A)
    ent = np.sum(logstd + 0.5 * np.log(2.0 * np.pi * np.e))
    pg_sum = np.sum(w * adv * nlp)
    vf_sum = 0.5 * np.sum(w * np.square(value - R))
    pg_loss, vf_loss = pg_sum / n, vf_sum / n
    loss = pg_loss - ent * ent_coef + vf_loss * vf_coef
    # ---- backward
    dnlp = w * adv / n
    z = (A - mean) / std
    dmean = dnlp[:, None] * (-(z / std))                                 # d nlp / d mean = -(a - mean) / std^2
    dlogstd = np.sum(dnlp[:, None] * (1.0 - z * z), axis=0, keepdims=True) - ent_coef * np.ones_like(logstd)
    dvalue = vf_coef * w * (value - R) / n
    grads = [None] * 13
    grads[8] = h2.T @ dmean
    grads[9] = dmean.sum(0)
    grads[10] = dlogstd
    dh2 = (dmean @ p[8].T) * (h2 > 0)
    grads[2] = h1.T @ dh2
    grads[3] = dh2.sum(0)
    dh1 = (dh2 @ p[2].T) * (h1 > 0)
    grads[0] = x.T @ dh1
    grads[1] = dh1.sum(0)
    grads[11] = g2.T @ dvalue[:, None]
    grads[12] = np.array([dvalue.sum()])
    dg2 = (dvalue[:, None] @ p[11].T) * (g2 > 0)
    grads[6] = g1.T @ dg2
    grads[7] = dg2.sum(0)
    dg1 = (dg2 @ p[6].T) * (g1 > 0)
    grads[4] = x.T @ dg1
    grads[5] = dg1.sum(0)
    return loss, np.array([pg_loss, vf_loss, ent]), np.array([pg_sum, vf_sum, np.sum(w)]), grads


def a2c_train_step(params, obs, actions, returns, values, is_weight, lr, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5):
    """ActorCriticModel.train from fresh Adam state: whole-batch advantage normalisation, gradient, clip_by_global_norm,
    TF1 Adam (eps 1e-5).  Returns (new params float64, stats [pg, vf, ent])."""
    advs = po.normalize_advantages(np.asarray(returns, np.float32), np.asarray(values, np.float32))
    _, stats, _, grads = a2c_loss_and_grads(params, obs, actions, advs, returns, is_weight, ent_coef, vf_coef)
    p64 = [np.asarray(p, np.float64) for p in params]
    gc, _ = po.clip_by_global_norm([np.asarray(g, np.float64).reshape(p.shape) for g, p in zip(grads, p64)], max_grad_norm)
    newp, _, _ = po.adam_step(p64, gc, [np.zeros_like(p) for p in p64], [np.zeros_like(p) for p in p64], 1, lr)
    return newp, stats
