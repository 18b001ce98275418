"""float64 reference of the PPO objective for a policy-zoo MLP net (ppo_grad_act with PPO_GRAD_TANH): the frozen observation filter
clip((x - mean) * invstd, +-clip), tanh 64-64 policy and value trunks, the diagonal Gaussian head and the value affine
v = v_scale * head + v_shift.  Loss terms as oracle/ppo_oracle.ppo_loss_and_grads (model.py:65-111), whose ``neglogp`` is imported; the
backprop is written out by hand and checked against central differences of ``loss`` in tests/test_zoo_learner_cpu.py.

``params``: the 13 tensors in the kernel's flat order (policies.PARAM_NAMES; for a zoo file: polfc1 polfc2 vffc1 vffc2 polfinal logstd
vffinal, policy_zoo.zoo_kernel_flat).  ``filt``: None (rows are already filtered) or (mean [D], invstd [D], clip).  Plain numpy."""
import numpy as np

from oracle import ppo_oracle as po


def filter_obs(obs, filt, dtype=np.float64):
    x = np.asarray(obs, dtype)
    if filt is None:
        return x
    mean, invstd, clip = filt
    return np.clip((x - np.asarray(mean, dtype)) * np.asarray(invstd, dtype), -clip, clip)


def forward(params, obs, filt=None, v_scale=1.0, v_shift=0.0, dtype=np.float64):
    """mean [n, A], value [n] (after the affine) and the activations the backward pass needs."""
    p = [np.asarray(t, dtype) for t in params]
    x = filter_obs(obs, filt, dtype)
    h1 = np.tanh(x @ p[0] + p[1])
    h2 = np.tanh(h1 @ p[2] + p[3])
    g1 = np.tanh(x @ p[4] + p[5])
    g2 = np.tanh(g1 @ p[6] + p[7])
    mean = h2 @ p[8] + p[9]
    value = v_scale * (g2 @ p[11] + p[12])[:, 0] + v_shift
    return mean, value, (x, h1, h2, g1, g2)


def _terms(params, obs, actions, advs, returns, oldneglogp, is_weight, cliprange, ent_coef, vf_coef, filt, v_scale, v_shift):
    p = [np.asarray(t, np.float64) for t in params]
    A = np.asarray(actions, np.float64)
    adv, R, old, w = (np.asarray(v, np.float64) for v in (advs, returns, oldneglogp, is_weight))
    mean, value, acts = forward(p, obs, filt, v_scale, v_shift)
    logstd = p[10]
    nlp = po.neglogp(mean, logstd, A)
    ent = np.sum(logstd + 0.5 * np.log(2.0 * np.pi * np.e))
    vf_loss = 0.5 * np.mean(np.square(value - R))
    log_ratio = old - nlp
    ratio = np.exp(log_ratio)
    nanmask = np.isnan(ratio)
    ratio = np.where(nanmask, 2.0, ratio)
    l1 = -adv * ratio
    l2 = -adv * np.clip(ratio, 1.0 - cliprange, 1.0 + cliprange)
    pg_loss = np.mean(w * np.maximum(l1, l2))
    loss = pg_loss - ent * ent_coef + vf_loss * vf_coef
    return dict(p=p, A=A, adv=adv, R=R, old=old, w=w, mean=mean, value=value, acts=acts, nlp=nlp, ent=ent, vf_loss=vf_loss,
                log_ratio=log_ratio, ratio=ratio, nanmask=nanmask, l1=l1, l2=l2, pg_loss=pg_loss, loss=loss)


def loss(params, obs, actions, advs, returns, oldneglogp, is_weight, cliprange, ent_coef, vf_coef, filt=None, v_scale=1.0, v_shift=0.0):
    """The scalar the gradient is taken of (means over the rows)."""
    return float(_terms(params, obs, actions, advs, returns, oldneglogp, is_weight, cliprange, ent_coef, vf_coef, filt, v_scale, v_shift)["loss"])


def loss_and_grads(params, obs, actions, advs, returns, oldneglogp, is_weight, cliprange, ent_coef, vf_coef, filt=None, v_scale=1.0,
                   v_shift=0.0):
    """Returns (loss, stats[5] = pg_loss, vf_loss, entropy, approxkl, clipfrac, log_ratio [n], grads: 13 float64 tensors)."""
    T = _terms(params, obs, actions, advs, returns, oldneglogp, is_weight, cliprange, ent_coef, vf_coef, filt, v_scale, v_shift)
    p, A, adv, R, old, w, mean, value = (T[k] for k in ("p", "A", "adv", "R", "old", "w", "mean", "value"))
    x, h1, h2, g1, g2 = T["acts"]
    ratio, l1, l2 = T["ratio"], T["l1"], T["l2"]
    n = A.shape[0]
    std = np.exp(p[10])
    in_clip = (ratio >= 1.0 - cliprange) & (ratio <= 1.0 + cliprange)
    d_l1 = (l1 >= l2).astype(np.float64)                                # tf.maximum: the first argument on ties
    dratio = w / n * (d_l1 * (-adv) + (1.0 - d_l1) * (-adv) * in_clip)
    dratio = np.where(T["nanmask"], 0.0, dratio)
    dnlp = -dratio * ratio
    z = (A - mean) / std
    dmean = dnlp[:, None] * (-(z / std))
    dhead_v = v_scale * vf_coef * (value - R) / n                        # d / d (raw value head): the affine's scale rides on the delta
    g = [None] * 13
    g[8] = h2.T @ dmean
    g[9] = dmean.sum(0)
    g[10] = np.sum(dnlp[:, None] * (1.0 - z * z), axis=0, keepdims=True) - ent_coef * np.ones_like(p[10])
    dh2 = (dmean @ p[8].T) * (1.0 - h2 * h2)
    g[2] = h1.T @ dh2
    g[3] = dh2.sum(0)
    dh1 = (dh2 @ p[2].T) * (1.0 - h1 * h1)
    g[0] = x.T @ dh1
    g[1] = dh1.sum(0)
    g[11] = g2.T @ dhead_v[:, None]
    g[12] = np.array([dhead_v.sum()])
    dg2 = (dhead_v[:, None] @ p[11].T) * (1.0 - g2 * g2)
    g[6] = g1.T @ dg2
    g[7] = dg2.sum(0)
    dg1 = (dg2 @ p[6].T) * (1.0 - g1 * g1)
    g[4] = x.T @ dg1
    g[5] = dg1.sum(0)
    stats = np.array([T["pg_loss"], T["vf_loss"], T["ent"], np.mean(T["nlp"] - old), np.mean((np.abs(ratio - 1.0) > cliprange).astype(np.float64))])
    return float(T["loss"]), stats, T["log_ratio"], g


def random_net(rng, ob, ac, scale=1.0):
    """13 float32 tensors of a tanh net whose units are neither dead nor saturated on unit-variance rows: first-layer weights
    ~ N(0, 1 / ob), hidden ~ N(0, 1 / 64), heads ~ N(0, 0.1), small biases, logstd ~ N(0, 0.1)."""
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    p = []
    for _ in range(2):
        p += [f(rng.normal(0, scale / np.sqrt(ob), (ob, 64))), f(rng.normal(0, 0.1, 64)), f(rng.normal(0, scale / 8.0, (64, 64))),
              f(rng.normal(0, 0.1, 64))]
    p += [f(rng.normal(0, 0.1, (64, ac))), f(rng.normal(0, 0.1, ac)), f(rng.normal(0, 0.1, (1, ac))), f(rng.normal(0, 0.1, (64, 1))),
          f(rng.normal(0, 0.1, 1))]
    return p
