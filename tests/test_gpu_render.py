"""GPU checks of the renderer (csrc/sumo_render.hip) against tests/render_ref.py: geom poses, frames on stable and unstable pixels,
output subsets, image edges, refusals, ``SumoVecEnv.render`` and ``play.py``.

Depth: the largest relative depth error measured over all stable pixels of all views below was 4.371e-7 (MI355X, the close view of
Ant-vs-Ant); the bound DEPTH_REL is 8 times that, 3.5e-6.  At the farthest stable hit of these views (the floor towards the horizon,
64 m) it allows 0.22 mm, and on the tatami (under 12 m) 0.04 mm: far below the 3 mm a misplaced border rod (radius 0.03 m) would
need to pass."""
import os
import subprocess
import sys

import numpy as np
import pytest

import render_ref as rr
from conftest import ROOT

sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

DEPTH_MEASURED = 4.371e-7
DEPTH_REL = 8 * DEPTH_MEASURED
W0, H0 = 64, 48
W1, H1 = 37, 21


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def renderers():
    from robosumo_selfplay_amd import render
    rs = {sc: render.Renderer(rr.model(sc)) for sc in rr.SCENES}
    yield rs
    for r in rs.values():
        r.close()


def _poses32(torch, scene, states):
    """Reference geom poses of the numbered states, rounded to float32: what both sides of the frame tests draw."""
    m = rr.model(scene)
    p = np.stack([rr.poses_array(m, rr.states(scene)[s]) for s in states]).astype(np.float32)
    return torch.from_numpy(p).cuda()


# ---- poses ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", rr.SCENES)
def test_poses_match_the_numpy_kinematics(torch, renderers, scene):
    m, r, q = rr.model(scene), renderers[scene], rr.states(scene)
    assert (r.nq, r.nbody, r.ngeom) == (m.nq, m.nbody, m.ngeom)
    ref = np.stack([rr.poses_array(m, qq) for qq in q])
    tol = 2.0 ** -23 * np.maximum(1.0, np.abs(ref))
    for k in range(len(q)):                                                              # n = 1: every state on its own
        got = r.poses(q[k:k + 1]).cpu().numpy().astype(np.float64)
        assert got.shape == (1, m.ngeom, 12)
        assert (np.abs(got[0] - ref[k]) <= tol[k]).all(), (rr.STATE_NAMES[k], np.abs(got[0] - ref[k]).max())
    for sel in ([0, 1, 4], [2, 3, 1]):                                                   # n = 3: a different state per env
        got = r.poses(torch.from_numpy(q[sel]).cuda()).cpu().numpy().astype(np.float64)
        assert (np.abs(got - ref[sel]) <= tol[sel]).all()
    R = ref[:, :, 3:].reshape(len(q), m.ngeom, 3, 3)                                     # the states differ and the frames are rotations
    assert np.abs(R @ R.transpose(0, 1, 3, 2) - np.eye(3)).max() < 1e-12 and np.abs(ref[1] - ref[0]).max() > 0.1


# ---- frames --------------------------------------------------------------------------------------------------------------------
_worst = {"rel": 0.0, "abs": 0.0}


def _check(out, k, ref):
    """Image ``k`` of a launch's outputs against a reference image."""
    gid, depth, rgb = out["id"][k], out["depth"][k], out["rgb"][k]
    st = ref["stable"]
    assert np.array_equal(gid[st], ref["id"][st])
    assert np.abs(rgb[st].astype(np.int32) - ref["rgb"][st].astype(np.int32)).max() <= 1
    hit = st & (ref["id"] >= 0)
    assert np.isposinf(depth[st & (ref["id"] < 0)]).all() and np.isfinite(depth[hit]).all()
    err = np.abs(depth[hit].astype(np.float64) - ref["depth"][hit])
    rel = (err / ref["depth"][hit]).max()
    _worst["rel"], _worst["abs"] = max(_worst["rel"], rel), max(_worst["abs"], err.max())
    print("largest relative depth error %.3e, absolute %.3e m (farthest hit %.1f m)" % (rel, err.max(), ref["depth"][hit].max()))
    assert DEPTH_REL * ref["depth"][hit].max() < 3e-3                 # the bound itself stays under a tenth of the thinnest radius
    assert rel <= DEPTH_REL
    un = ~st
    assert (gid[un][None] == ref["probe_ids"][:, un]).any(axis=0).all()      # off the mask: still what the centre or a probe point sees
    assert (np.isposinf(depth[un]) == (gid[un] < 0)).all()


def _launch(torch, r, poses, cams, W, H, want=("rgb", "depth", "id")):
    out = r.frames_from_poses(poses, cams, W, H, want)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("scene", rr.SCENES)
@pytest.mark.parametrize("size,view", [(s, v) for s, views in rr.SIZES.items() for v in views], ids=lambda p: str(p).replace(" ", ""))
def test_frames_match_the_reference_with_one_shared_camera(torch, renderers, scene, size, view):
    W, H = size
    out = _launch(torch, renderers[scene], _poses32(torch, scene, rr.FRAME_STATES), rr.view_camera(view), W, H)
    assert out["rgb"].shape == (3, H, W, 3) and out["depth"].shape == (3, H, W) and out["id"].shape == (3, H, W)
    assert out["rgb"].dtype == np.uint8 and out["depth"].dtype == np.float32 and out["id"].dtype == np.int32
    for k, s in enumerate(rr.FRAME_STATES):
        _check(out, k, rr.reference(scene, s, view, W, H))


@pytest.mark.parametrize("scene", rr.SCENES)
def test_frames_match_the_reference_with_one_camera_per_env(torch, renderers, scene):
    views = rr.SIZES[(W0, H0)]
    out = _launch(torch, renderers[scene], _poses32(torch, scene, rr.FRAME_STATES), [rr.view_camera(v) for v in views], W0, H0)
    for k, (s, v) in enumerate(zip(rr.FRAME_STATES, views)):
        _check(out, k, rr.reference(scene, s, v, W0, H0))


def test_alpha_is_opaque_and_every_primitive_is_drawn(torch, renderers):
    scene = rr.SCENES[0]
    m, r = rr.model(scene), renderers[scene]
    out = r.frames_from_poses(_poses32(torch, scene, [0]), rr.view_camera("arena"), W0, H0, ("rgb", "id"))
    rgba = out["rgb"]._base if out["rgb"]._base is not None else out["rgb"]
    assert tuple(rgba.shape) == (1, H0, W0, 4) and bool((rgba[..., 3] == 255).all())
    seen = set(int(m.geom_type[g]) for g in np.unique(out["id"].cpu().numpy()) if g >= 0)
    assert seen == {rr.PLANE, rr.SPHERE, rr.CAPSULE, rr.CYLINDER, rr.BOX}


def test_frames_from_qpos_flatten_leading_axes(torch, renderers):
    scene = rr.SCENES[1]
    r, q = renderers[scene], rr.states(scene)
    a = r.frames(q[[0, 1, 4, 2]].reshape(2, 2, -1), rr.view_camera("close"), W1, H1, ("rgb", "id"))
    assert tuple(a["rgb"].shape) == (2, 2, H1, W1, 3) and tuple(a["id"].shape) == (2, 2, H1, W1)
    b = r.frames(torch.from_numpy(q[[4]]).cuda(), rr.view_camera("close"), W1, H1, ("id",))
    assert torch.equal(a["id"][1, 0], b["id"][0])
    ref = rr.reference(scene, 0, "arena", W1, H1)                                        # the kernel's own poses draw the same picture
    c = r.frames(q[0], rr.view_camera("arena"), W1, H1, ("id",))["id"].cpu().numpy()
    assert c.shape == (H1, W1) and np.array_equal(c[ref["stable"]], ref["id"][ref["stable"]])


# ---- output subsets, repeatability -----------------------------------------------------------------------------------------------
def test_output_subsets_equal_the_full_launch_bitwise(torch, renderers):
    scene = rr.SCENES[1]
    r, poses, cam = renderers[scene], _poses32(torch, scene, rr.FRAME_STATES), rr.view_camera("close")
    full = _launch(torch, r, poses, cam, W1, H1)
    again = _launch(torch, r, poses, cam, W1, H1)
    for k in ("rgb", "depth", "id"):
        assert np.array_equal(full[k].view(np.uint8), again[k].view(np.uint8))            # two identical launches agree bitwise
        one = _launch(torch, r, poses, cam, W1, H1, (k,))
        assert list(one) == [k] and np.array_equal(one[k].view(np.uint8), full[k].view(np.uint8))


# ---- the C ABI directly: edges and refusals --------------------------------------------------------------------------------------
def _raw(torch, r, poses, cams, n, W, H, rgba=None, depth=None, ids=None, ncam=None, light=None, colors="default"):
    from robosumo_selfplay_amd import render, render_capi
    sh = dict(render.SHADING)
    if light is not None:
        sh["light"] = light
    ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    col = r.colors if isinstance(colors, str) else colors
    rc = render_capi.lib().sumo_render_frames(r.h, ptr(poses), n, ptr(cams), cams.shape[0] if ncam is None else ncam, ptr(col),
                                              render_capi.shade(**sh), W, H, ptr(rgba), ptr(depth), ptr(ids), None)
    torch.cuda.synchronize()
    return rc


def test_image_edges_leave_the_neighbouring_rows_alone(torch, renderers):
    """37 x 21 is no multiple of the 16 x 16 tile: each output gets a sentinel row before and after the two images, the second
    image following the first directly."""
    scene = rr.SCENES[0]
    r, poses = renderers[scene], _poses32(torch, scene, [1, 4])
    cams = torch.from_numpy(rr.view_camera("arena").record()[None]).cuda()
    rows = 2 * H1 + 2
    rgba = torch.full((rows, W1, 4), 0x5A, dtype=torch.uint8, device="cuda")
    depth = torch.full((rows, W1), -7.0, dtype=torch.float32, device="cuda")
    ids = torch.full((rows, W1), -99, dtype=torch.int32, device="cuda")
    assert _raw(torch, r, poses, cams, 2, W1, H1, rgba[1:].data_ptr(), depth[1:].data_ptr(), ids[1:].data_ptr()) == 0
    for buf, fill in ((rgba, 0x5A), (depth, -7.0), (ids, -99)):
        assert bool((buf[0] == fill).all()) and bool((buf[-1] == fill).all())
    want = _launch(torch, r, poses, rr.view_camera("arena"), W1, H1)
    body = lambda t: t[1:-1].reshape((2, H1, W1) + tuple(t.shape[2:])).cpu().numpy()
    assert np.array_equal(body(rgba)[..., :3], want["rgb"]) and bool((rgba[1:-1, :, 3] == 255).all())
    assert np.array_equal(body(depth), want["depth"]) and np.array_equal(body(ids), want["id"])
    assert not np.array_equal(want["id"][0], want["id"][1])
    _check(want, 1, rr.reference(scene, 4, "arena", W1, H1))                             # env 1's image is its own


def test_refusals_come_before_any_launch(torch, renderers, ant_model):
    from robosumo_selfplay_amd import capi, render_capi
    scene = rr.SCENES[0]
    r, poses = renderers[scene], _poses32(torch, scene, rr.FRAME_STATES)
    cams = torch.from_numpy(rr.view_camera("arena").record()[None]).cuda()
    out = torch.full((3, H1, W1), -99, dtype=torch.int32, device="cuda")
    host = np.zeros(poses.numel(), np.float32)
    L = render_capi.lib()
    bad = dict(n0=dict(n=0), n_neg=dict(n=-2), w0=dict(W=0), w_big=dict(W=4097), h0=dict(H=0), h_big=dict(H=4097), ncam=dict(ncam=2),
               poses_null=dict(poses=None), cams_null=dict(cams=None, ncam=1), colours_null=dict(colors=None), outputs_null=dict(ids=None),
               light_long=dict(light=(0.0, 0.0, 1.01)), light_zero=dict(light=(0.0, 0.0, 0.0)),
               device_mismatch=dict(poses=host.ctypes.data))
    for name, kw in bad.items():
        args = dict(poses=poses, cams=cams, n=3, W=W1, H=H1, ids=out)
        args.update(kw)
        rc = _raw(torch, r, **args)
        assert rc < 0 and L.sumo_render_last_error(), name
        assert bool((out == -99).all()), name
    assert b"device" in L.sumo_render_last_error()
    assert _raw(torch, r, poses, cams, 3, W1, H1, ids=out) == 0 and bool((out != -99).all())     # the same call, unspoiled, draws
    rc = L.sumo_render_poses(r.h, None, 1, poses.data_ptr(), None)
    assert rc < 0
    assert L.sumo_render_poses(r.h, poses.data_ptr(), 0, poses.data_ptr(), None) < 0
    blob = bytearray(ant_model.to_blob())
    blob[8] ^= 0xFF
    with pytest.raises(capi.SumoHipError, match="malformed"):
        render_capi.create(bytes(blob))
    with pytest.raises(capi.SumoHipError, match="out of range"):
        render_capi.create(ant_model.to_blob(), device=torch.cuda.device_count())


# ---- env -----------------------------------------------------------------------------------------------------------------------
def test_env_render_tiles_the_renderer_frames(torch, renderers):
    from robosumo_selfplay_amd import render
    from robosumo_selfplay_amd.vec_env import SumoVecEnv
    rng = np.random.default_rng(0)
    acts = rng.uniform(-1, 1, (5, 4, 2, 8)).astype(np.float32)
    pics = {}
    for groups in (1, 2):
        env = SumoVecEnv("RoboSumo-Ant-vs-Ant-v0", num_envs=4, seed=3, groups=groups)
        try:
            env.reset()
            a = env.render("rgb_array", width=W0, height=H0)
            for t in range(5):
                env.step(acts[t])
            b = env.render(mode="rgb_array", width=W0, height=H0)
            qpos = np.concatenate([E.get_state()[0] for E in env.engines])
            want = renderers["RoboSumo-Ant-vs-Ant-v0"].frames(qpos, render.arena_camera(), W0, H0)["rgb"].cpu().numpy()
            assert a.shape == (2 * H0, 2 * W0, 3) and a.dtype == np.uint8 and b.shape == a.shape
            assert np.array_equal(b, render.tile_images(want)) and not np.array_equal(a, b)
            assert env.get_images(envs=[2], width=W1, height=H1, camera="track").shape == (1, H1, W1, 3)
            with pytest.raises(NotImplementedError, match="no display path"):
                env.render("human")
            pics[groups] = (a, b)
        finally:
            env.close()
        assert env._renderer is None
    assert np.array_equal(pics[1][0], pics[2][0]) and np.array_equal(pics[1][1], pics[2][1])


# ---- play.py -------------------------------------------------------------------------------------------------------------------
def test_play_records_renders_and_replays(torch, tmp_path):
    from robosumo_selfplay_amd import policies
    from robosumo_selfplay_amd.model import PPOModel
    spec = policies.PolicySpec(121, 8, value_network="copy", activation="relu")
    cks = []
    for name in ("a", "b"):
        p = str(tmp_path / name)
        PPOModel(policy=spec, trainable=False).save(p)
        cks.append(p)
    out, out2 = str(tmp_path / "out"), str(tmp_path / "out2")
    run = lambda argv: subprocess.run([sys.executable, os.path.join(ROOT, "play.py")] + argv, capture_output=True, text=True, timeout=300)
    p = run(["--p1", cks[0], "--p2", cks[1], "--num_env", "2", "--episodes", "1", "--max_frames", "8", "--width", str(W0), "--height", str(H0),
             "--out", out])
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-2000:]
    traj = np.load(os.path.join(out, "traj.npz"))
    frames = np.load(os.path.join(out, "frames.npy"))
    assert traj["qpos"].shape == (8, 2, 30) and traj["done"].shape == (8, 2) and traj["score"].shape == (2, 3)
    assert str(traj["env_id"]) == "RoboSumo-Ant-vs-Ant-v0" and str(traj["p1"]) == cks[0] and str(traj["p2"]) == cks[1]
    assert frames.shape == (8, 2, H0, W0, 3) and frames.dtype == np.uint8
    assert not np.array_equal(frames[0], frames[7]) and len(np.unique(frames[0].reshape(-1, 3), axis=0)) > 8
    p = run(["--replay", os.path.join(out, "traj.npz"), "--width", str(W0), "--height", str(H0), "--out", out2])
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-2000:]
    assert np.array_equal(np.load(os.path.join(out2, "frames.npy")), frames) and not os.path.exists(os.path.join(out2, "traj.npz"))
    try:
        import PIL  # noqa: F401
        assert os.path.exists(os.path.join(out, "env00.gif")) and os.path.exists(os.path.join(out, "env01.gif"))
    except ImportError:
        assert "PIL is not installed" in p.stdout


def test_play_drives_every_pairing_one_step_at_a_time(torch, tmp_path):
    """Every pairing of the step-by-step match driver is playable: checkpoints of both families in both seatings and against zoo
    nets of both families; what ``matches.match_pairing`` refuses, play.py refuses with its message."""
    import joblib
    import play
    from robosumo_selfplay_amd import policies
    from zoo_lstm_helpers import golden, synthetic_lstm_flat
    rng = np.random.RandomState(3)
    files = {"mlp": policies.init_param_list(121, 8), "lstm": policies.init_lstm_param_list(121, 8, 128, rng=rng),
             "lstm64": policies.init_lstm_param_list(121, 8, 64, rng=rng)}
    for name, plist in files.items():
        files[name] = str(tmp_path / name)
        joblib.dump(plist, files[name])
    for name, flat in (("zoo_mlp", golden("ant-mlp-v3")), ("zoo_lstm", synthetic_lstm_flat(120, 8, 8))):
        files[name] = str(tmp_path / (name + ".npy"))
        np.save(files[name], flat)
    args = lambda p1, p2: play.parse_args(["--p1", files[p1], "--p2", files[p2], "--num_env", "2", "--episodes", "1", "--max_frames", "3",
                                           "--deterministic", "--out", str(tmp_path / "o")])
    first = None
    for p1, p2 in (("mlp", "mlp"), ("lstm", "lstm"), ("mlp", "lstm"), ("lstm", "mlp"), ("mlp", "zoo_mlp"), ("mlp", "zoo_lstm"),
                   ("lstm", "zoo_lstm"), ("lstm", "zoo_mlp"), ("lstm64", "mlp")):
        qpos, done, score = play.play(args(p1, p2))
        assert qpos.shape == (3, 2, 30) and done.shape == (3, 2) and score.shape == (2, 3) and np.isfinite(qpos).all(), (p1, p2)
        assert np.abs(qpos[2] - qpos[0]).max() > 1e-4, (p1, p2)
        first = qpos if first is None else first
    assert np.array_equal(play.play(args("mlp", "mlp"))[0], first)                      # deterministic play repeats
    with pytest.raises(ValueError, match="agent 1 only"):
        play.play(args("zoo_mlp", "mlp"))
    with pytest.raises(ValueError, match="mixed LSTM widths"):
        play.play(args("lstm64", "lstm"))
