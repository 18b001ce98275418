"""CPU checks of the rendering layer: libsumo_render.so builds and exports what include/sumo_render.h declares, the product path
refuses to run without a GPU, cameras, colours, tiling, play.py's arguments, the trajectory file and the GIF writer."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest

from conftest import ROOT, has_gpu
from robosumo_selfplay_amd import build, capi, render, render_capi

sys.path.insert(0, ROOT)
import play  # noqa: E402


def _declared():
    txt = open(os.path.join(ROOT, "include", "sumo_render.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(sumo_render_[a-z0-9_]+)\s*\(", txt)))


def test_render_library_is_the_third_job_and_exports_the_header():
    built = build.build_all()
    assert [os.path.basename(p) for p in built] == ["libsumo_hip.so", "libsumo_ppo.so", "libsumo_render.so"]
    L = ctypes.CDLL(build.lib_path("libsumo_render.so"))
    names = _declared()
    assert set(names) == set(render_capi.EXPORTS) and len(names) == 6
    for n in names:
        assert hasattr(L, n), n
    # no other sumo_* / ppo_* entry point: the library is its own translation unit
    import subprocess
    nm = subprocess.run(["nm", "-D", "--defined-only", build.lib_path("libsumo_render.so")], capture_output=True, text=True)
    if nm.returncode == 0:
        ext = set(re.findall(r" T ((?:sumo|ppo)_\w+)", nm.stdout))
        assert ext == set(render_capi.EXPORTS)


def test_header_constants_match_the_binding():
    txt = open(os.path.join(ROOT, "include", "sumo_render.h")).read()
    val = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, txt).group(1))
    assert (val("SUMO_RENDER_MAXGEOM"), val("SUMO_RENDER_MAXBODY"), val("SUMO_RENDER_MAXDIM"), val("SUMO_RENDER_CAM_STRIDE"),
            val("SUMO_RENDER_POSE_STRIDE")) == (render_capi.MAXGEOM, render_capi.MAXBODY, render_capi.MAXDIM, render_capi.CAM_STRIDE,
                                                render_capi.POSE_STRIDE)
    assert ctypes.sizeof(render_capi.Shade) == 32
    assert float(re.search(r"#define\s+SUMO_RENDER_TIE_REL\s+([0-9.e+-]+)f", txt).group(1)) == render_capi.TIE_REL == 2.0 ** -19


def test_bad_blob_is_refused_before_any_device_is_touched(ant_model):
    build.build_all()
    blob = bytearray(ant_model.to_blob())
    blob[8] ^= 0xFF                                     # the magic
    with pytest.raises(capi.SumoHipError, match="malformed model blob"):
        render_capi.create(bytes(blob))
    with pytest.raises(capi.SumoHipError, match="malformed model blob"):
        render_capi.create(bytes(ant_model.to_blob())[:-8])


@pytest.mark.skipif(has_gpu(), reason="only meaningful without a GPU")
def test_no_cpu_fallback(ant_model):
    build.build_all()
    with pytest.raises(capi.SumoHipError):
        render.Renderer(ant_model)
    with pytest.raises(capi.SumoHipError, match="no HIP device"):
        render_capi.create(ant_model.to_blob())
    from robosumo_selfplay_amd.vec_env import SumoVecEnv
    env = object.__new__(SumoVecEnv)                    # the constructor itself refuses to run here; render must as well
    env.closed, env.model, env.num_envs, env.device = True, ant_model, 2, types.SimpleNamespace(index=0)
    with pytest.raises(capi.SumoHipError):
        env.render("rgb_array", width=64, height=48)
    with pytest.raises(NotImplementedError, match="no display path"):
        env.render("human")


def test_camera_record_is_orthonormal():
    rng = np.random.default_rng(0)
    cams = [render.arena_camera(), render.Camera((1.5, -3.0, 1.6), (0, 0, 0.8)), render.Camera((0.01, -0.02, 9.0), (0, 0, 0.5), fovy=30)]
    cams += [render.Camera(rng.uniform(-5, 5, 3), rng.uniform(-1, 1, 3)) for _ in range(5)]
    for c in cams:
        r = c.record()
        assert r.dtype == np.float32 and r.shape == (16,)
        B = r[3:12].reshape(3, 3).astype(np.float64)
        assert np.abs(B @ B.T - np.eye(3)).max() < 1e-6
        assert np.allclose(np.cross(B[0], B[1]), -B[2], atol=1e-6)                      # right x up = -forward
        f = (c.target - c.eye) / np.linalg.norm(c.target - c.eye)
        assert np.abs(B[2] - f).max() < 1e-6 and np.allclose(r[0:3], c.eye.astype(np.float32))
        assert abs(r[12] - np.tan(np.radians(c.fovy) / 2)) < 1e-6 and not r[13:].any()
    with pytest.raises(ValueError):
        render.Camera((0, 0, 1), (0, 0, 0)).record()                                    # looks along its up vector
    with pytest.raises(ValueError):
        render.Camera((0, 0, 1), (0, 0, 1)).record()


def test_track_camera_looks_at_the_torsos_midpoint(ant_model):
    q = np.tile(np.asarray(ant_model.qpos0, np.float64), (3, 1))
    q[1, 0:2] += (0.5, -0.25)
    rec = render.track_camera(ant_model, q)
    assert rec.shape == (3, 16) and rec.dtype == np.float32
    mid = render.torso_positions(ant_model, q).mean(axis=1)
    for k in range(3):
        to_mid = mid[k] - rec[k, 0:3]
        assert np.allclose(to_mid / np.linalg.norm(to_mid), rec[k, 9:12], atol=1e-6)
    assert np.allclose(render.torso_positions(ant_model, q)[0, 0], ant_model.qpos0[0:3])
    assert not np.allclose(rec[0, 0:3], rec[1, 0:3])


@pytest.mark.parametrize("env_id", ["RoboSumo-Ant-vs-Ant-v0", "RoboSumo-Spider-vs-Bug-v0"])
def test_default_colors(env_id):
    from robosumo_selfplay_amd import mjcf
    m = mjcf.load_model(env_id)
    col = render.default_colors(m)
    assert col.shape == (m.ngeom, 3) and col.dtype == np.float32 and col.min() >= 0 and col.max() <= 1
    owner = np.array([int(m.body_rootid[int(m.geom_bodyid[g])]) for g in range(m.ngeom)])
    a0, a1 = (owner == int(m.body_rootid[int(b)]) for b in m.agent_torso)
    assert a0.sum() > 1 and a1.sum() > 1 and not (a0 & a1).any()
    assert len(np.unique(col[a0], axis=0)) == 1 and len(np.unique(col[a1], axis=0)) == 1
    assert not np.allclose(col[a0][0], col[a1][0])
    names = list(m.geom_names)
    assert np.allclose(col[names.index("floor")], (0.2, 0.2, 0.2)) and np.allclose(col[names.index("tatami")], (0.65, 0.57, 0.31))
    for rod in ("topborder", "rightborder", "bottomborder", "leftborder"):
        assert np.allclose(col[names.index(rod)], (0.18, 0.23, 0.38))


@pytest.mark.parametrize("n,grid", [(1, (1, 1)), (2, (2, 1)), (3, (2, 2)), (4, (2, 2)), (5, (3, 2)), (7, (3, 3)), (16, (4, 4))])
def test_tile_images(n, grid):
    imgs = np.arange(n * 3 * 5 * 3, dtype=np.uint8).reshape(n, 3, 5, 3)
    t = render.tile_images(imgs)
    rows, cols = grid
    assert t.shape == (rows * 3, cols * 5, 3) and t.dtype == np.uint8
    for k in range(n):
        r, c = divmod(k, cols)
        assert np.array_equal(t[r * 3:(r + 1) * 3, c * 5:(c + 1) * 5], imgs[k])
    assert not t.reshape(rows, 3, cols, 5, 3).transpose(0, 2, 1, 3, 4).reshape(rows * cols, -1)[n:].any()
    with pytest.raises(ValueError):
        render.tile_images(np.zeros((0, 3, 5, 3), np.uint8))


def test_play_arguments():
    a = play.parse_args(["--p1", "a", "--p2", "b", "--out", "o"])
    assert (a.num_env, a.episodes, a.max_frames, a.camera, a.width, a.height, a.every, a.deterministic) == (4, 2, None, "arena", 320, 240, 1, False)
    a = play.parse_args(["--replay", "t.npz", "--camera", "track", "--out", "o", "--width", "64", "--height", "48"])
    assert a.replay == "t.npz" and a.camera == "track" and (a.width, a.height) == (64, 48)
    for bad in (["--p1", "a", "--out", "o"], ["--replay", "t", "--p1", "a", "--out", "o"], ["--p1", "a", "--p2", "b"],
                ["--p1", "a", "--p2", "b", "--out", "o", "--every", "0"], ["--p1", "a", "--p2", "b", "--out", "o", "--width", "5000"],
                ["--p1", "a", "--p2", "b", "--out", "o", "--camera", "orbit"], ["--p1", "a", "--p2", "b", "--out", "o", "--max_frames", "0"]):
        with pytest.raises(SystemExit):
            play.parse_args(bad)


def test_play_resolves_its_sides(tmp_path):
    ck = tmp_path / "run" / "checkpoints"
    ck.mkdir(parents=True)
    for name in ("00000", "00003", "00010"):
        (ck / name).write_bytes(b"x")
    assert play.resolve_side(str(tmp_path / "run")) == ("ckpt", str(ck / "00010"))
    assert play.resolve_side(str(ck / "00003")) == ("ckpt", str(ck / "00003"))
    assert play.resolve_side("zoo/agent-params-v1.npy") == ("zoo", "zoo/agent-params-v1.npy")
    with pytest.raises(ValueError):
        play.resolve_side(str(tmp_path / "nothing"))


def test_trajectory_round_trip(tmp_path):
    rng = np.random.default_rng(1)
    qpos, done = rng.standard_normal((5, 2, 30)), rng.integers(0, 2, (5, 2)).astype(np.uint8)
    score = np.array([[1, 0, 0], [0, 1, 1]], np.int32)
    p = str(tmp_path / "traj.npz")
    render.save_trajectory(p, qpos, done, score, "RoboSumo-Ant-vs-Ant-v0", "runs/a", "zoo/b.npy", every=3)
    t = render.load_trajectory(p)
    assert np.array_equal(t["qpos"], qpos) and t["qpos"].dtype == np.float64
    assert np.array_equal(t["done"], done) and np.array_equal(t["score"], score)
    assert (t["env_id"], t["p1"], t["p2"], t["every"]) == ("RoboSumo-Ant-vs-Ant-v0", "runs/a", "zoo/b.npy", 3)
    with pytest.raises(ValueError):
        render.save_trajectory(p, qpos, done[:4], score, "e", "a", "b")


def test_gif_writer(tmp_path):
    pytest.importorskip("PIL")
    from PIL import Image
    frames = np.zeros((4, 2, 12, 16, 3), np.uint8)
    for f in range(4):
        frames[f, :, :, 4 * f:4 * f + 4] = (255, 40 * f, 0)
    files = render.write_outputs(str(tmp_path / "out"), frames, fps=10)
    assert [os.path.basename(f) for f in files] == ["frames.npy", "env00.gif", "env01.gif"]
    assert np.array_equal(np.load(files[0]), frames)
    im = Image.open(files[1])
    assert im.n_frames == 4 and im.size == (16, 12)
    im.seek(2)
    assert np.asarray(im.convert("RGB"))[0, 9].tolist()[0] > 200 and np.asarray(im.convert("RGB"))[0, 0].tolist() == [0, 0, 0]


def test_render_library_passes_the_codegen_scan():
    """build.py runs the partial-EXEC save-copy scan on the third library like on the other two; it must come out clean."""
    import shutil
    from robosumo_selfplay_amd import codegen_check
    if not (shutil.which("objcopy") and os.path.exists(os.path.join(codegen_check.LLVM, "llvm-objdump"))):
        pytest.skip("objcopy / llvm-objdump not available")
    build.build_all()
    hits = codegen_check.scan_library(build.lib_path("libsumo_render.so"))
    assert not hits, {k: [t for _, t, _ in v] for k, v in hits.items()}
