"""Pictures of RoboSumo matches: cameras, colours and the two launches of csrc/sumo_render.hip (include/sumo_render.h).

Counterpart of what the reference gets from MuJoCo's offscreen renderer in play_demo.py / play_evaluation.py / video_recorder.py:
``Renderer.frames`` turns joint positions into RGB (and depth / geom id) images on the GPU, ``tile_images`` lays the images of a
vectorised env out in one picture (baselines' ``VecEnv.render``), and the trajectory helpers below are what ``play.py`` records and
replays.  There is no CPU fallback and no window: a frame is an array.

Conventions: pixel (x, y) with row 0 at the top, the ray through the pixel centre; surfaces are seen from
outside only; flat shading ``base * (ambient + diffuse * max(0, n . light))`` with the constants of :data:`SHADING`.
"""
import math
import os

import numpy as np

from . import capi, render_capi

# the one place the shading constants live (the kernel receives them per launch, the tests' reference reads them from here):
# the unit direction TOWARDS the light, the ambient and diffuse weights and the sky colour (tatami.xml's skybox rgb1)
_LIGHT = np.array([0.35, -0.5, 0.8])
SHADING = dict(light=tuple(float(v) for v in _LIGHT / np.linalg.norm(_LIGHT)), ambient=0.35, diffuse=0.65, sky=(0.8, 0.8, 1.0))

# tatami.xml: the floor and tatami materials' rgb1, the border rods' rgba; the two agents' colours are this project's choice
WORLD_COLORS = {"floor": (0.2, 0.2, 0.2), "tatami": (0.65, 0.57, 0.31)}
ROD_COLOR = (0.18, 0.23, 0.38)
AGENT_COLORS = ((0.85, 0.33, 0.25), (0.25, 0.45, 0.85))

ARENA_EYE, ARENA_TARGET = (5.5, -5.5, 4.5), (0.0, 0.0, 0.6)
TRACK_OFFSET = (2.6, -2.6, 2.2)


class Camera(object):
    """A pinhole camera at ``eye`` looking at ``target``; ``fovy`` is the vertical field of view in degrees.  The kernel does no
    look-at arithmetic: :meth:`record` is the float32 [16] record it reads (eye, right, up, forward, tan(fovy / 2), padding), the
    basis computed here in float64 and rounded."""

    def __init__(self, eye, target, fovy=45.0, up=(0.0, 0.0, 1.0)):
        self.eye, self.target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
        self.fovy, self.up = float(fovy), np.asarray(up, np.float64)
        if self.eye.shape != (3,) or self.target.shape != (3,) or self.up.shape != (3,):
            raise ValueError("eye, target and up are 3-vectors")
        if not 0.0 < self.fovy < 180.0:
            raise ValueError("fovy must lie in (0, 180) degrees")

    def record(self):
        return camera_records(self.eye[None], self.target[None], self.fovy, self.up)[0]


def camera_records(eye, target, fovy=45.0, up=(0.0, 0.0, 1.0)):
    """float32 [k][16] camera records of k eye / target pairs (float64 [k][3] each)."""
    eye, target, up = np.asarray(eye, np.float64), np.asarray(target, np.float64), np.asarray(up, np.float64)
    f = target - eye
    nf = np.linalg.norm(f, axis=-1, keepdims=True)
    if not np.all(nf > 0):
        raise ValueError("a camera's eye and target coincide")
    f = f / nf
    r = np.cross(f, up)
    nr = np.linalg.norm(r, axis=-1, keepdims=True)
    if not np.all(nr > 1e-9):
        raise ValueError("a camera looks along its up vector")
    r = r / nr
    u = np.cross(r, f)
    rec = np.zeros((eye.shape[0], render_capi.CAM_STRIDE), np.float64)
    rec[:, 0:3], rec[:, 3:6], rec[:, 6:9], rec[:, 9:12] = eye, r, u, f
    rec[:, 12] = math.tan(math.radians(float(fovy)) / 2.0)
    return rec.astype(np.float32)


def arena_camera():
    """A fixed three-quarter view of the whole tatami."""
    return Camera(ARENA_EYE, ARENA_TARGET)


def torso_positions(model, qpos):
    """World positions [..., 2, 3] of the two agents' torsos (the free joints' positions in ``qpos`` [..., nq])."""
    qpos = np.asarray(qpos, np.float64)
    adr = [int(model.jnt_qposadr[int(model.body_jntadr[int(b)])]) for b in model.agent_torso]
    return np.stack([qpos[..., a:a + 3] for a in adr], axis=-2)


def track_camera(model, qpos):
    """One camera per env: looks at the midpoint of the two torsos from a fixed offset.  ``qpos`` [..., nq] -> float32 records
    [..., 16]."""
    mid = torso_positions(model, qpos).mean(axis=-2)
    lead = mid.shape[:-1]
    mid = mid.reshape(-1, 3)
    return camera_records(mid + np.asarray(TRACK_OFFSET), mid).reshape(lead + (render_capi.CAM_STRIDE,))


def default_colors(model):
    """Base colours float32 [ngeom][3]: the floor, the tatami and the border rods as tatami.xml colours them; every geom of agent 0
    and every geom of agent 1 in that agent's colour (a geom belongs to the agent whose torso is the root of its body)."""
    col = np.zeros((model.ngeom, 3), np.float32)
    roots = [int(model.body_rootid[int(b)]) for b in model.agent_torso]
    for g in range(model.ngeom):
        b = int(model.geom_bodyid[g])
        root = int(model.body_rootid[b])
        if b == 0:
            col[g] = WORLD_COLORS.get(model.geom_names[g], ROD_COLOR)
        else:
            col[g] = AGENT_COLORS[roots.index(root)]
    return col


def tile_images(imgs):
    """n images [n][H][W][C] laid out row by row in one near-square grid [rows * H][cols * W][C] (rows = ceil(sqrt(n)), unused
    cells black): what ``VecEnv.render`` shows of a vectorised env."""
    imgs = np.asarray(imgs)
    if imgs.ndim != 4 or imgs.shape[0] < 1:
        raise ValueError("tile_images takes a non-empty [n][H][W][C] array")
    n, H, W, Cn = imgs.shape
    rows = int(math.ceil(math.sqrt(n)))
    cols = int(math.ceil(n / float(rows)))
    grid = np.zeros((rows * cols, H, W, Cn), imgs.dtype)
    grid[:n] = imgs
    return grid.reshape(rows, cols, H, W, Cn).transpose(0, 2, 1, 3, 4).reshape(rows * H, cols * W, Cn)


WANT = ("rgb", "depth", "id")


class Renderer(object):
    """Owner of one ``sumo_render_t``: geom poses and frames of ``model`` on ``device``."""

    def __init__(self, model, device=0):
        import torch
        if not torch.cuda.is_available():
            raise capi.SumoHipError("Renderer needs a HIP device (there is no CPU fallback in the product path)")
        self._torch = torch
        self.model = model
        self.device = torch.device("cuda", int(device))
        self.h = render_capi.create(model.to_blob(), int(device))
        d = np.zeros(3, np.int32)
        render_capi.chk(render_capi.lib().sumo_render_dims(self.h, d.ctypes.data_as(render_capi.C.c_void_p)))
        self.nq, self.nbody, self.ngeom = (int(x) for x in d)
        self.colors = torch.from_numpy(default_colors(model)).to(self.device)
        self.shade = render_capi.shade(**SHADING)

    def close(self):
        if getattr(self, "h", None):
            render_capi.lib().sumo_render_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return self._torch.cuda.current_stream(self.device).cuda_stream

    def _qpos(self, qpos):
        torch = self._torch
        if not torch.is_tensor(qpos):
            qpos = torch.from_numpy(np.ascontiguousarray(qpos, np.float64))
        if qpos.dtype != torch.float64 or qpos.dim() < 1 or qpos.shape[-1] != self.nq or qpos.numel() == 0:
            raise ValueError("qpos must be a float64 [..., %d] array or CUDA tensor" % self.nq)
        return qpos.to(self.device).contiguous()

    def poses(self, qpos):
        """Geom poses float32 CUDA [..., ngeom][12] (centre, then the rotation row-major) of ``qpos`` float64 [..., nq]."""
        q = self._qpos(qpos)
        n = q.numel() // self.nq
        out = self._torch.empty(tuple(q.shape[:-1]) + (self.ngeom, render_capi.POSE_STRIDE), dtype=self._torch.float32, device=self.device)
        render_capi.chk(render_capi.lib().sumo_render_poses(self.h, q.data_ptr(), n, out.data_ptr(), self._stream()))
        return out

    def _cameras(self, cameras, n):
        torch = self._torch
        if isinstance(cameras, Camera):
            cameras = cameras.record()
        elif not torch.is_tensor(cameras) and len(cameras) and isinstance(cameras[0], Camera):
            cameras = np.stack([c.record() for c in cameras])
        if not torch.is_tensor(cameras):
            cameras = torch.from_numpy(np.ascontiguousarray(cameras, np.float32))
        cams = cameras.to(self.device, torch.float32).reshape(-1, render_capi.CAM_STRIDE).contiguous()
        if cams.shape[0] not in (1, n):
            raise ValueError("%d cameras for %d frames: give one camera or one per frame" % (cams.shape[0], n))
        return cams

    def frames_from_poses(self, poses, cameras, width, height, want=("rgb",), colors=None):
        """:meth:`frames` from geom poses (float32 CUDA [..., ngeom][12]) instead of joint positions."""
        torch = self._torch
        want = (want,) if isinstance(want, str) else tuple(want)
        if not want or any(w not in WANT for w in want):
            raise ValueError("want must name some of %s" % (WANT,))
        if poses.dtype != torch.float32 or not poses.is_cuda or tuple(poses.shape[-2:]) != (self.ngeom, render_capi.POSE_STRIDE):
            raise ValueError("poses must be a float32 CUDA tensor [..., %d][%d]" % (self.ngeom, render_capi.POSE_STRIDE))
        poses = poses.contiguous()
        lead = tuple(poses.shape[:-2])
        n = int(np.prod(lead)) if lead else 1
        cams = self._cameras(cameras, n)
        col = self.colors if colors is None else torch.as_tensor(colors, dtype=torch.float32).to(self.device).contiguous()
        if tuple(col.shape) != (self.ngeom, 3):
            raise ValueError("colors must have shape (%d, 3)" % self.ngeom)
        W, H = int(width), int(height)
        if not (1 <= W <= render_capi.MAXDIM and 1 <= H <= render_capi.MAXDIM):
            raise ValueError("width and height must lie in [1, %d]" % render_capi.MAXDIM)
        shp = lead + (H, W)
        rgba = torch.empty(shp + (4,), dtype=torch.uint8, device=self.device) if "rgb" in want else None
        depth = torch.empty(shp, dtype=torch.float32, device=self.device) if "depth" in want else None
        ids = torch.empty(shp, dtype=torch.int32, device=self.device) if "id" in want else None
        ptr = lambda t: None if t is None else t.data_ptr()
        render_capi.chk(render_capi.lib().sumo_render_frames(self.h, poses.data_ptr(), n, cams.data_ptr(), int(cams.shape[0]), col.data_ptr(),
                                                             self.shade, W, H, ptr(rgba), ptr(depth), ptr(ids), self._stream()))
        out = {}
        if rgba is not None:
            out["rgb"] = rgba[..., :3]
        if depth is not None:
            out["depth"] = depth
        if ids is not None:
            out["id"] = ids
        return out

    def frames(self, qpos, cameras, width, height, want=("rgb",), colors=None):
        """Images of ``qpos`` float64 [..., nq] (host array or CUDA tensor) in one launch pair, all leading axes flattened into the
        launch's n: dict of CUDA tensors ``rgb`` uint8 [..., H][W][3] (a view of the RGBA buffer), ``depth`` float32 [..., H][W]
        (+inf for sky) and ``id`` int32 [..., H][W] (-1 for sky), those named in ``want``.  ``cameras``: a :class:`Camera` or one
        record (shared), or one per frame (a list of cameras or float32 records [..., 16])."""
        return self.frames_from_poses(self.poses(qpos), cameras, width, height, want, colors)


# ---- trajectories (play.py) ----------------------------------------------------------------------------------------------------
def save_trajectory(path, qpos, done, score, env_id, p1, p2, every=1):
    """``traj.npz``: qpos float64 [F][n][nq], done uint8 [F][n], the score table int32 [n][3] (agent 0 wins, agent 1 wins, draws),
    the env id, the two sides' paths and the recording stride."""
    qpos, done, score = np.asarray(qpos, np.float64), np.asarray(done, np.uint8), np.asarray(score, np.int32)
    if qpos.ndim != 3 or done.shape != qpos.shape[:2] or score.shape != (qpos.shape[1], 3):
        raise ValueError("qpos [F][n][nq], done [F][n] and score [n][3] do not fit together")
    np.savez_compressed(path, qpos=qpos, done=done, score=score, env_id=np.str_(env_id), p1=np.str_(p1), p2=np.str_(p2),
                        every=np.int32(every))


def load_trajectory(path):
    with np.load(path, allow_pickle=False) as z:
        return dict(qpos=z["qpos"], done=z["done"], score=z["score"], env_id=str(z["env_id"]), p1=str(z["p1"]), p2=str(z["p2"]),
                    every=int(z["every"]))


def render_trajectory(renderer, qpos, camera="arena", width=320, height=240, batch=256):
    """RGB frames uint8 [F][n][H][W][3] (host) of a recorded trajectory ``qpos`` [F][n][nq]: all F x n frames in launches of up to
    ``batch`` frames.  ``camera``: 'arena', 'track' (one camera per frame, following the torsos) or a :class:`Camera`."""
    qpos = np.asarray(qpos, np.float64)
    F, n, nq = qpos.shape
    flat = qpos.reshape(F * n, nq)
    if camera == "arena":
        cams = arena_camera().record()[None]
    elif camera == "track":
        cams = track_camera(renderer.model, flat)
    elif isinstance(camera, Camera):
        cams = camera.record()[None]
    else:
        raise ValueError("camera must be 'arena', 'track' or a Camera")
    out = np.empty((F * n, int(height), int(width), 3), np.uint8)
    for s in range(0, F * n, int(batch)):
        e = min(s + int(batch), F * n)
        rgb = renderer.frames(flat[s:e], cams if cams.shape[0] == 1 else cams[s:e], width, height)["rgb"]
        out[s:e] = rgb.cpu().numpy()
    return out.reshape(F, n, int(height), int(width), 3)


def write_gif(path, frames, fps=20):
    """An animated GIF of ``frames`` uint8 [F][H][W][3] through PIL.  Returns False (and writes nothing) where PIL is missing."""
    try:
        from PIL import Image
    except ImportError:
        return False
    ims = [Image.fromarray(np.ascontiguousarray(f)) for f in np.asarray(frames, np.uint8)]
    ims[0].save(path, save_all=True, append_images=ims[1:], duration=max(1, int(round(1000.0 / fps))), loop=0)
    return True


def write_outputs(out_dir, frames, fps=20):
    """``frames.npy`` and one GIF per env under ``out_dir`` for ``frames`` [F][n][H][W][3].  Returns the list of files written."""
    os.makedirs(out_dir, exist_ok=True)
    files = [os.path.join(out_dir, "frames.npy")]
    np.save(files[0], frames)
    for e in range(frames.shape[1]):
        p = os.path.join(out_dir, "env%02d.gif" % e)
        if not write_gif(p, frames[:, e], fps):
            print("PIL is not installed: no GIFs written (frames.npy holds the frames)")
            break
        files.append(p)
    return files
