#!/usr/bin/env python3
"""Watch a match: counterpart of the reference's play_evaluation.py / play_demo.py (and of its video_recorder.py, as files).

    python play.py --p1 results/a/RoboSumo-Ant-vs-Ant-v0-0 --p2 results/b/RoboSumo-Ant-vs-Ant-v0-0 --out demo
    python play.py --p1 results/a/RoboSumo-Ant-vs-Ant-v0-0/checkpoints/00100 --p2 policy_zoo/ant/mlp/agent-params-v1.npy --out demo
    python play.py --replay demo/traj.npz --camera track --out demo_track

A side is a run directory (its latest checkpoint plays), a checkpoint file or -- agent 1 only -- a policy-zoo .npy file; every
pairing the step-by-step match driver plays is playable (MLP, LSTM, across the families, zoo MLP, zoo LSTM).  The match advances
one step at a time on the step-by-step driver with every agent reporting its height under adjust_z = -0.5, as the reference's
play scripts do; after every --every-th step the envs' joint positions are recorded.  Written under --out: traj.npz (qpos, done
flags, score table, env id, the two sides), frames.npy (uint8 [F][n][H][W][3], rendered on the GPU after play) and one animated
GIF per env where PIL is installed.  --replay renders a stored trajectory again without any policy.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def parse_args(argv):
    ap = argparse.ArgumentParser(description="Play two policies against each other and render the match on the GPU.")
    ap.add_argument("--p1", help="agent 0: run directory (latest checkpoint) or checkpoint file")
    ap.add_argument("--p2", help="agent 1: run directory, checkpoint file or policy-zoo .npy file")
    ap.add_argument("--replay", help="a traj.npz written by an earlier call: render it again (no policies)")
    ap.add_argument("--env", default="RoboSumo-Ant-vs-Ant-v0")
    ap.add_argument("--num_env", type=int, default=4)
    ap.add_argument("--episodes", type=int, default=2, help="finished episodes per env")
    ap.add_argument("--max_frames", type=int, default=None, help="stop after this many recorded frames")
    ap.add_argument("--deterministic", action="store_true", help="act with the policy means instead of sampling")
    ap.add_argument("--camera", choices=("arena", "track"), default="arena")
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--every", type=int, default=1, help="record every N-th step")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--fps", type=int, default=20, help="GIF frame rate")
    ap.add_argument("--out", required=True, help="output directory")
    args = ap.parse_args(argv)
    if args.replay:
        if args.p1 or args.p2:
            ap.error("--replay takes no --p1 / --p2")
    elif not (args.p1 and args.p2):
        ap.error("give --p1 and --p2, or --replay")
    if args.num_env < 1 or args.episodes < 1 or args.every < 1 or args.fps < 1 or (args.max_frames is not None and args.max_frames < 1):
        ap.error("--num_env, --episodes, --every, --fps and --max_frames must be >= 1")
    if not (1 <= args.width <= 4096 and 1 <= args.height <= 4096):
        ap.error("--width and --height must lie in [1, 4096]")
    return args


def resolve_side(path):
    """('zoo', file) for a policy-zoo .npy file, else ('ckpt', checkpoint file): the file itself or a run's latest checkpoint."""
    from robosumo_selfplay_amd import matches
    path = os.path.expanduser(str(path))
    if path.endswith(".npy"):
        return "zoo", path
    if os.path.isdir(path):
        ids = matches.list_checkpoints(path)
        ck = matches.checkpoint_dir(path)
        if not ids and not os.path.isfile(os.path.join(ck, "00000")):
            raise ValueError("no checkpoints in %s" % ck)
        return "ckpt", os.path.join(ck, ids[-1] if ids else "00000")
    if not os.path.isfile(path):
        raise ValueError("%s is neither a run directory nor a file" % path)
    return "ckpt", path


def resolve_pairing(env, p1, p2):
    """(pairing, idx0 row, idx1 row) of agent 0 playing ``p1`` against agent 1 playing ``p2`` (``matches.match_pairing``)."""
    from robosumo_selfplay_amd import matches
    (f1, path1), (f2, path2) = resolve_side(p1), resolve_side(p2)
    if f1 == "zoo":
        raise ValueError("policy-zoo nets play agent 1 only: give the checkpoint as --p1 and the .npy file as --p2")
    k1 = matches.checkpoint_kind(path1)
    if f2 == "zoo":
        from robosumo_selfplay_amd.policy_zoo import ZooLstmTable, ZooTable, zoo_file_kind
        table0 = matches._table_of(k1, env, [path1])
        matches._check_env(env, table0)
        flat = np.load(path2, allow_pickle=False)
        zoo = (ZooLstmTable if zoo_file_kind(flat.size, table0.spec.ac_dim) == "lstm" else ZooTable)([flat], table0.spec.ac_dim, env.device)
        matches._check_zoo_dims(table0, zoo)
        return matches.match_pairing(table0, zoo), 0, 0
    k2 = matches.checkpoint_kind(path2)
    if k1 == k2:                                   # one family: both agents play rows of ONE table
        table = matches._table_of(k1, env, [path1, path2])
        matches._check_env(env, table)
        return matches.match_pairing(table, table), 0, 1
    table0, table1 = matches._table_of(k1, env, [path1]), matches._table_of(k2, env, [path2])
    matches._check_env(env, table0)
    matches._check_env(env, table1)
    return matches.match_pairing(table0, table1), 0, 0     # refuses mixed LSTM widths


def play(args):
    """Plays the match step by step; returns (qpos [F][n][nq], done [F][n], score [n][3])."""
    import torch
    from robosumo_selfplay_amd import matches
    from robosumo_selfplay_amd.vec_env import make_vec_env
    env = make_vec_env(args.env, args.num_env, args.seed, adjust_z=matches.EVAL_ADJUST_Z)
    try:
        pairing, r0, r1 = resolve_pairing(env, args.p1, args.p2)
        N, A = env.num_envs, pairing.seats[0].table.spec.ac_dim
        idx0, idx1 = np.full(N, r0, np.int32), np.full(N, r1, np.int32)
        states = tuple(None if s.width is None else torch.zeros((N, s.width), dtype=torch.float32, device=env.device) for s in pairing.seats)
        score = torch.zeros((N, 3), dtype=torch.int32, device=env.device)
        gen = torch.Generator(device=env.device)
        gen.manual_seed(int(args.seed))
        env.reset_device()
        qpos, done = [], []
        limit = args.episodes * (env.model.timestep_limit + 1) + 1          # every episode ends by the time limit
        for step in range(1, limit + 1):
            noise = None if args.deterministic else tuple(torch.randn((1, N, A), generator=gen, device=env.device) for _ in range(2))
            matches.pairing_steps(env, pairing, states, idx0, idx1, score, args.episodes, 1, noise, fused=False)
            if step % args.every == 0:
                torch.cuda.synchronize(env.device)
                qpos.append(np.concatenate([E.get_state()[0] for E in env.engines]))
                done.append(env.done_dev[:, 0].cpu().numpy())
                if args.max_frames is not None and len(qpos) >= args.max_frames:
                    break
            if not bool((score.sum(1) < args.episodes).any()):
                break
        if not qpos:
            raise ValueError("no frame was recorded: --every %d exceeds the %d steps played" % (args.every, step))
        return np.stack(qpos), np.stack(done), score.cpu().numpy()
    finally:
        env.close()


def main(argv):
    args = parse_args(argv)
    from robosumo_selfplay_amd import mjcf, render
    os.makedirs(args.out, exist_ok=True)
    if args.replay:
        traj = render.load_trajectory(args.replay)
        qpos, env_id = traj["qpos"], traj["env_id"]
    else:
        qpos, done, score = play(args)
        env_id = mjcf.canonical_id(args.env)
        path = os.path.join(args.out, "traj.npz")
        render.save_trajectory(path, qpos, done, score, env_id, args.p1, args.p2, args.every)
        print("wrote %s: %d frames of %d envs; score (agent 0 wins, agent 1 wins, draws) %s" % (path, qpos.shape[0], qpos.shape[1],
                                                                                             score.sum(0).tolist()))
    r = render.Renderer(mjcf.load_model(env_id))
    try:
        frames = render.render_trajectory(r, qpos, args.camera, args.width, args.height)
    finally:
        r.close()
    for f in render.write_outputs(args.out, frames, args.fps):
        print("wrote %s" % f)
    return frames


if __name__ == "__main__":
    main(sys.argv[1:])
