"""Shared by the zoo LSTM tests (TEST INFRASTRUCTURE): a synthetic policy-zoo LSTM vector and the golden zoo vectors."""
import os

import numpy as np

from robosumo_selfplay_amd import policy_zoo

HERE = os.path.dirname(os.path.abspath(__file__))


def synthetic_lstm_flat(D, A, seed):
    """A zoo-LSTM-shaped vector with a non-trivial observation filter and O(1) weights (built as tests/test_gpu_zoo.py builds its own)."""
    rng = np.random.default_rng(seed)
    sh = policy_zoo.zoo_lstm_shapes(D, A)
    cnt = 500.0
    parts = []
    for k in policy_zoo._ZOO_LSTM_ORDER:
        s = sh[k]
        if k.endswith("/count"):
            v = np.array(cnt)
        elif k.endswith("/sum"):
            v = cnt * rng.normal(0, 0.5, s)
        elif k.endswith("/sumsq"):
            v = cnt * (0.25 + rng.uniform(0.0, 2.0, s))
        elif k == "logstd":
            v = rng.normal(-1.0, 0.3, s)
        elif k.endswith(("/w", "/kernel")):
            v = rng.normal(0, 1.0 / np.sqrt(s[0]), s)
        else:
            v = rng.normal(0, 0.1, s)
        parts.append(np.asarray(v, np.float32).ravel())
    return np.concatenate(parts)


def golden(name):
    """Vector ``name`` (e.g. 'ant-lstm-v3') of tests/golden/zoo_v3_params.npz."""
    with np.load(os.path.join(HERE, "golden", "zoo_v3_params.npz"), allow_pickle=False) as z:
        return z[name].copy()
