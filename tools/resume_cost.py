#!/usr/bin/env python3
"""What one resume-state save of ``learn(resume_interval=...)`` costs, next to an update of the same process.

    python tools/resume_cost.py [--out profiles/resume_cost.json] [--updates 5] [--only mlp|lstm]

Two runs of the public ``alg_ppo.learn`` on Ant-vs-Ant with the reference's RoboSumo hyper-parameters (defaults.py) and a state
written after every update: the MLP learner in ``ours`` mode at 4096 envs x nsteps 128 (the flagship shape; ``ours`` is the mode whose
state carries the previous rollout's agent-1 rows) and the LSTM(128) learner at 1024 x 128.  Per run: the wall time of a save -- split
into :func:`resume.capture` (device to host) and :func:`resume.write_state` (serialise, fsync, rename) -- the file size and its split
between the env snapshot, ``opponent_data`` and the rest, and the median update time (rollout + optimiser phase, from ``history``).
The first update (kernel attributes, graph capture) is left out of the medians.  One JSON document; nothing is asserted."""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ANT = "RoboSumo-Ant-vs-Ant-v0"


def serialised_bytes(x):
    import torch
    buf = io.BytesIO()
    torch.save(x, buf)
    return buf.getbuffer().nbytes


def measure(network, num_envs, nsteps, updates):
    import torch
    from robosumo_selfplay_amd import alg_ppo, defaults, resume
    from robosumo_selfplay_amd.vec_env import SumoVecEnv
    kw = defaults.get_default_params(ANT, "ppo")
    kw.update(nsteps=nsteps)
    if network == "lstm":
        for k in ("value_network", "num_hidden", "num_layers", "activation"):
            kw.pop(k, None)
        kw.update(nlstm=128)
    saves = []
    capture0, write0 = resume.capture, resume.write_state

    def capture(**a):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = capture0(**a)
        saves.append(dict(capture_s=time.perf_counter() - t0))
        return st

    def write_state(log_dir, state):
        t0 = time.perf_counter()
        path, size = write0(log_dir, state)
        saves[-1].update(write_s=time.perf_counter() - t0, file_bytes=size)
        return path, size

    env = SumoVecEnv(ANT, num_envs=num_envs, seed=1)
    resume.capture, resume.write_state = capture, write_state
    try:
        with tempfile.TemporaryDirectory(prefix="resume_cost_") as log_dir:
            model = alg_ppo.learn(network=network, env=env, seed=1, nagent=2, total_timesteps=num_envs * nsteps * updates, log_dir=log_dir,
                                  opponent_mode="ours", verbose=False, save_interval=1, resume_interval=1, **kw)
            state = resume.read_state(log_dir)
            t0 = time.perf_counter()
            resume.read_state(log_dir)
            read_s = time.perf_counter() - t0
    finally:
        resume.capture, resume.write_state = capture0, write0
        env.close()
    h = model.history
    update_s = [a + b for a, b in zip(h["rollout_s"], h["update_s"])][1:]
    parts = dict(env=serialised_bytes(state["env"]), opponent_data=serialised_bytes(state["opponent_data"]))
    parts["rest"] = serialised_bytes({k: v for k, v in state.items() if k not in ("env", "opponent_data")})
    med = lambda k: statistics.median(s[k] for s in saves[1:])
    save_s = statistics.median(s["capture_s"] + s["write_s"] for s in saves[1:])
    upd = statistics.median(update_s)
    return dict(network=network, num_envs=num_envs, nsteps=nsteps, updates=updates, nminibatches=kw["nminibatches"], noptepochs=kw["noptepochs"],
                save_s=save_s, capture_s=med("capture_s"), write_s=med("write_s"), read_s=read_s, file_bytes=saves[-1]["file_bytes"],
                part_bytes=parts, update_s=upd, rollout_s=statistics.median(h["rollout_s"][1:]), save_share_of_update=save_s / upd,
                every_save_s=[s["capture_s"] + s["write_s"] for s in saves], every_update_s=[a + b for a, b in zip(h["rollout_s"], h["update_s"])])


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resume_cost.json"))
    ap.add_argument("--updates", type=int, default=5)
    ap.add_argument("--only", choices=["mlp", "lstm"], default=None)
    args = ap.parse_args(argv)
    import torch
    runs = []
    for network, n in (("mlp", 4096), ("lstm", 1024)):
        if args.only in (None, network):
            runs.append(measure(network, n, 128, args.updates))
            r = runs[-1]
            print("%s %d x %d: save %.3f s (capture %.3f, write %.3f), file %.1f MB (env %.1f, opponent_data %.1f, rest %.1f), update %.3f s, "
                  "a save is %.2f updates" % (network, n, 128, r["save_s"], r["capture_s"], r["write_s"], r["file_bytes"] / 1e6,
                                              r["part_bytes"]["env"] / 1e6, r["part_bytes"]["opponent_data"] / 1e6, r["part_bytes"]["rest"] / 1e6,
                                              r["update_s"], r["save_share_of_update"]), flush=True)
    doc = dict(tool="tools/resume_cost.py", device=torch.cuda.get_device_name(0), torch=torch.__version__, runs=runs)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main(sys.argv[1:])
