"""Builds and binds tests/host/push_host.cpp: the impulse's code (steppingstone_amd/csrc/ss_push.hpp) compiled for the CPU (the recipe
of native_build.py).  TEST INFRASTRUCTURE for the GPU-less container; never imported by steppingstone_amd."""
import ctypes as C
import os

import numpy as np

import native_build
from native_build import HOST_DIR

LIB = os.path.join(HOST_DIR, "libpush_host.so")
SRC = os.path.join(HOST_DIR, "push_host.cpp")
TRI = 27 * 28 // 2


def build():
    return native_build.build_host(SRC, LIB)


_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        vp = C.c_void_p
        _lib.ph_push.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    return _lib


def push(kind, packed, body, point, impulse, mass=False):
    """kind 0 / 1; row k pushes env k: packed [n,186], body [n] int or None (the torso), point [n,3] or None (the centre of mass),
    impulse [n,6] -> delta_nu [n,27] float32 (NaN rows where the body index is out of range); with mass=True also the lower triangle
    [n,378] of the matrix the solve started from."""
    packed = np.ascontiguousarray(packed, np.float32)
    n = packed.shape[0]
    impulse = np.ascontiguousarray(impulse, np.float32).reshape(n, 6)
    body = None if body is None else np.ascontiguousarray(body, np.int32).reshape(n)
    point = None if point is None else np.ascontiguousarray(point, np.float32).reshape(n, 3)
    out = np.full((n, 27), np.nan, np.float32)
    tri = np.full((n, TRI), np.nan, np.float32) if mass else None
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    load().ph_push(int(kind), n, ptr(packed), ptr(body), ptr(point), ptr(impulse), ptr(out), ptr(tri))
    return (out, tri) if mass else out


def push_modes(kind, packed, body, mode, point, impulse):
    """push() over rows whose point is given per row: mode 0 rows go through the call with point == None, the others with their points"""
    out = np.full((packed.shape[0], 27), np.nan, np.float32)
    null = np.asarray(mode) == 0
    if null.any():
        out[null] = push(kind, packed[null], body[null], None, impulse[null])
    if (~null).any():
        out[~null] = push(kind, packed[~null], body[~null], point[~null], impulse[~null])
    return out
