"""Builds and binds tests/host/render_host.cpp: the render kernels' code (steppingstone_amd/csrc/ss_render.hpp) compiled for the CPU
(the recipe of native_build.py).  TEST INFRASTRUCTURE for the GPU-less container; never imported by steppingstone_amd."""
import ctypes as C
import os

import numpy as np

import native_build
from native_build import HOST_DIR, hipcc  # noqa: F401  (hipcc re-exported: the tests ask this module for it)

LIB = os.path.join(HOST_DIR, "librender_host.so")
SRC = os.path.join(HOST_DIR, "render_host.cpp")


class Camera(C.Structure):
    _fields_ = [("mode", C.c_int32), ("eye", C.c_float * 3), ("target", C.c_float * 3), ("fov_y_deg", C.c_float),
                ("far_m", C.c_float), ("flags", C.c_int32)]


def build():
    return native_build.build_host(SRC, LIB)


_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        vp = C.c_void_p
        _lib.rh_body_poses.argtypes = [C.c_int, C.c_int, vp, vp]
        _lib.rh_render.argtypes = [C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def camera(cam):
    """np_render's camera dict -> ss_camera."""
    c = Camera()
    c.mode = int(cam["mode"])
    c.eye[:] = [float(x) for x in cam["eye"]]
    c.target[:] = [float(x) for x in cam["target"]]
    c.fov_y_deg, c.far_m = float(cam["fov_y_deg"]), float(cam["far_m"])
    c.flags = 1 if cam.get("shadows", True) else 0
    return c


def body_poses(kind, packed):
    packed = np.ascontiguousarray(packed, np.float32)
    out = np.zeros((packed.shape[0], 22, 12), np.float32)
    load().rh_body_poses(int(kind), packed.shape[0], _p(packed), _p(out))
    return out


def render(kind, packed, env_ids, W, H, cam):
    """kind 0 / 1; packed [N,186]; cam: np_render camera dict.  -> rgb [M,H,W,3] u8, depth [M,H,W] f32, seg [M,H,W] u8."""
    packed = np.ascontiguousarray(packed, np.float32)
    ids = np.ascontiguousarray(env_ids, np.int32)
    m = ids.size
    rgb = np.zeros((m, H, W, 3), np.uint8)
    depth = np.zeros((m, H, W), np.float32)
    seg = np.zeros((m, H, W), np.uint8)
    c = camera(cam)
    load().rh_render(int(kind), packed.shape[0], _p(packed), _p(ids), m, W, H, C.byref(c), _p(rgb), _p(depth), _p(seg))
    return rgb, depth, seg
