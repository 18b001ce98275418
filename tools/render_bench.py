#!/usr/bin/env python3
"""Renderer throughput: the pose launch and the frame launch, timed separately with device events.

Two workloads: a recorded match (64 envs x 200 frames at 320 x 240, rendered in launches of --batch frames, as play.py does) and a
training batch seen once (4096 envs x 1 frame at 64 x 48).  Each launch kind is warmed up, then timed --repeats times between two
events on the stream; the median is reported (and the spread), as frames/s and rays/s (rays = pixels).  The numpy reference's time
for one 64 x 48 frame (tests/render_ref.py, on the host) is written next to them, for scale only.

    python tools/render_bench.py --out profiles/r17_render_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _states(model, n, seed):
    """n plausible states: qpos0 with random joint angles inside their ranges and the torsos moved about the tatami."""
    from robosumo_selfplay_amd import mjcf
    rng = np.random.default_rng(seed)
    q = np.tile(np.asarray(model.qpos0, np.float64), (n, 1))
    for j in range(model.njnt):
        a = int(model.jnt_qposadr[j])
        if int(model.jnt_type[j]) == mjcf.JNT_FREE:
            q[:, a:a + 2] += rng.uniform(-0.5, 0.5, (n, 2))
        else:
            lo, hi = model.jnt_range[j]
            q[:, a] = rng.uniform(lo, hi, n)
    return q


def _timed(torch, fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms = np.array(ms)
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()), repeats=int(repeats))


def workload(torch, r, name, envs, frames, W, H, batch, camera, warmup, repeats, seed):
    from robosumo_selfplay_amd import render
    total = envs * frames
    n = min(batch, total)
    launches = -(-total // n)
    q = torch.from_numpy(_states(r.model, n, seed)).to(r.device)
    cams = render.arena_camera() if camera == "arena" else render.track_camera(r.model, q.cpu().numpy())
    poses = r.poses(q)
    tp = _timed(torch, lambda: r.poses(q), warmup, repeats)
    tf = _timed(torch, lambda: r.frames_from_poses(poses, cams, W, H), warmup, repeats)
    out = dict(name=name, envs=envs, frames=frames, width=W, height=H, camera=camera, frames_per_launch=n, launches=launches,
               ngeom=r.ngeom, pose_launch=tp, frame_launch=tf)
    fsec = tf["median_ms"] * 1e-3
    out["frame_launch"].update(frames_per_s=n / fsec, rays_per_s=n * W * H / fsec)
    out["pose_launch"].update(poses_per_s=n / (tp["median_ms"] * 1e-3))
    out["workload_ms"] = launches * (tp["median_ms"] + tf["median_ms"])
    out["workload_frames_per_s"] = total / (out["workload_ms"] * 1e-3)          # device time of both launch kinds, copies to the host excluded
    return out


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--env", default="RoboSumo-Ant-vs-Ant-v0")
    ap.add_argument("--batch", type=int, default=256, help="frames per launch of the recorded-match workload (play.py's batch)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="JSON output path")
    args = ap.parse_args(argv)
    import torch
    from robosumo_selfplay_amd import mjcf, render
    if not torch.cuda.is_available():
        raise SystemExit("render_bench needs a GPU: nothing is measured without one")
    model = mjcf.load_model(args.env)
    r = render.Renderer(model)
    rec = dict(env=args.env, device=torch.cuda.get_device_name(0), workloads=[])
    for camera in ("arena", "track"):
        rec["workloads"].append(workload(torch, r, "match_64x200_320x240", 64, 200, 320, 240, args.batch, camera, args.warmup, args.repeats,
                                         args.seed))
    rec["workloads"].append(workload(torch, r, "batch_4096x1_64x48", 4096, 1, 64, 48, 4096, "arena", args.warmup, args.repeats, args.seed))
    r.close()
    import render_ref
    q0 = np.asarray(model.qpos0, np.float64)
    ctr, R = render_ref.rounded_frames(model, q0)
    eye, d = render_ref.rays(render.arena_camera().record(), 64, 48)
    t0 = time.perf_counter()
    for _ in range(3):
        render_ref.cast(model, ctr, R, eye, d)
    rec["numpy_reference_64x48_frame_ms"] = (time.perf_counter() - t0) / 3 * 1e3
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    return rec


if __name__ == "__main__":
    main(sys.argv[1:])
