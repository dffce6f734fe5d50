"""Builds and binds tests/host/kinematics_host.cpp: the kinematic readout's code (steppingstone_amd/csrc/ss_kinematics.hpp) compiled for
the CPU (the recipe of native_build.py).  TEST INFRASTRUCTURE for the GPU-less container; never imported by
steppingstone_amd."""
import ctypes as C
import os

import numpy as np

import native_build
from native_build import HOST_DIR

LIB = os.path.join(HOST_DIR, "libkinematics_host.so")
SRC = os.path.join(HOST_DIR, "kinematics_host.cpp")


def build():
    return native_build.build_host(SRC, LIB)


_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        vp = C.c_void_p
        _lib.kh_kinematics.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp]
    return _lib


def kinematics(kind, packed, twists=True, summary=True, corners=True):
    """kind 0 / 1; packed [N,186] -> dict of the requested outputs of ss_kinematics: body_twist [N,22,6], summary [N,12], corners [N,8,8]."""
    packed = np.ascontiguousarray(packed, np.float32)
    n = packed.shape[0]
    out = {}
    if twists:
        out["body_twist"] = np.zeros((n, 22, 6), np.float32)
    if summary:
        out["summary"] = np.zeros((n, 12), np.float32)
    if corners:
        out["corners"] = np.zeros((n, 8, 8), np.float32)
    ptr = lambda k: out[k].ctypes.data_as(C.c_void_p) if k in out else None
    load().kh_kinematics(int(kind), n, packed.ctypes.data_as(C.c_void_p), ptr("body_twist"), ptr("summary"), ptr("corners"))
    return out
