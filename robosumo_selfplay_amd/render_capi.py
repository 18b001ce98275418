"""ctypes binding of include/sumo_render.h (csrc/libsumo_render.so).  No CPU fallback."""
import ctypes as C
import os

from . import build as _build
from .capi import SumoHipError

MAXGEOM, MAXBODY, MAXDIM, CAM_STRIDE, POSE_STRIDE = 128, 96, 4096, 16, 12
TIE_REL = 2.0 ** -19      # SUMO_RENDER_TIE_REL: hits within this of each other, relative, tie and the lower geom id wins
_LIB = None

EXPORTS = ("sumo_render_last_error", "sumo_render_create", "sumo_render_destroy", "sumo_render_dims", "sumo_render_poses",
           "sumo_render_frames")


class Shade(C.Structure):
    """``sumo_render_shade`` of include/sumo_render.h."""
    _fields_ = [("light", C.c_float * 3), ("ambient", C.c_float), ("diffuse", C.c_float), ("sky", C.c_float * 3)]


def lib():
    global _LIB
    if _LIB is None:
        path = os.environ.get("SUMO_RENDER_LIB") or _build.lib_path("libsumo_render.so")
        if not os.path.exists(path):
            raise SumoHipError("%s not found: build it with `python -m robosumo_selfplay_amd.build` "
                               "(the renderer has no CPU fallback)" % path)
        L = C.CDLL(path)
        vp, i32 = C.c_void_p, C.c_int
        L.sumo_render_last_error.restype = C.c_char_p
        L.sumo_render_create.argtypes = [vp, C.c_size_t, i32, C.POINTER(vp)]
        L.sumo_render_destroy.argtypes = [vp]
        L.sumo_render_dims.argtypes = [vp, vp]
        L.sumo_render_poses.argtypes = [vp, vp, i32, vp, vp]
        L.sumo_render_frames.argtypes = [vp, vp, i32, vp, i32, vp, Shade, i32, i32, vp, vp, vp, vp]
        for n in EXPORTS[1:]:
            getattr(L, n).restype = i32
        _LIB = L
    return _LIB


def chk(rc):
    if rc != 0:
        raise SumoHipError("sumo_render error %d: %s" % (rc, lib().sumo_render_last_error().decode()))


def shade(light, ambient, diffuse, sky):
    s = Shade()
    s.light[:] = [float(v) for v in light]
    s.ambient, s.diffuse = float(ambient), float(diffuse)
    s.sky[:] = [float(v) for v in sky]
    return s


def create(blob, device=0):
    """A ``sumo_render_t`` for the model blob (bytes) on ``device``."""
    buf = (C.c_char * len(blob)).from_buffer_copy(blob)
    h = C.c_void_p()
    chk(lib().sumo_render_create(C.cast(buf, C.c_void_p), len(blob), int(device), C.byref(h)))
    return h
