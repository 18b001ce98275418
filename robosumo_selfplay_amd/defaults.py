"""Hyper-parameter defaults of the reference (defaults.py:5-84), RoboSumo / ppo and ac branches."""


def robosumo_ppo():
    return dict(nsteps=8192, nminibatches=32, lam=1.0, gamma=0.995, rho_bar=10.0, c_bar=1.0, noptepochs=6, lr=1e-3, cliprange=0.2,
                ent_coef=0.0, value_network="copy", anneal_bound=1000, num_hidden=64, activation="relu")   # defaults.py:8-26


def robosumo_ac():
    return dict(nsteps=5, lam=0.95, gamma=0.995, log_interval=1000, save_interval=3000, ent_coef=0.0, lr=3e-4, value_network="copy",
                anneal_bound=1000, num_hidden=64, activation="relu")                                       # defaults.py:49-62


def get_default_params(env_id, algo="ppo"):
    if algo == "td3":
        raise NotImplementedError("td3 is not ported: the reference's alg_td3.py does not run against its own multi-agent env (it calls "
                                  "env.observation_space.shape[0] on a tuple space and uses a single-env loop), and it needs a replay "
                                  "buffer and a twin-Q critic this project does not have")
    if algo not in ("ppo", "ac"):
        raise NotImplementedError("algo %r: only the ppo and ac branches of defaults.py are ported" % (algo,))
    if not env_id.startswith("RoboSumo"):
        raise NotImplementedError("only RoboSumo envs")
    return robosumo_ppo() if algo == "ppo" else robosumo_ac()
