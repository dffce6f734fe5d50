"""Builds and binds tests/host/eom_host.cpp: the equation-of-motion readout's code (steppingstone_amd/csrc/ss_eom.hpp) compiled for the
CPU (the recipe of native_build.py).  TEST INFRASTRUCTURE for the GPU-less container; never imported by steppingstone_amd."""
import ctypes as C
import os

import numpy as np

import native_build
from native_build import HOST_DIR

LIB = os.path.join(HOST_DIR, "libeom_host.so")
SRC = os.path.join(HOST_DIR, "eom_host.cpp")


def build():
    return native_build.build_host(SRC, LIB)


_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        vp = C.c_void_p
        _lib.eh_eom.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp]
    return _lib


def eom(kind, packed, mass=True, forces=True, jacobians=True):
    """kind 0 / 1; packed [N,186] -> dict of the requested outputs of ss_eom: mass [N,27,27], forces [N,3,27], corner_jac [N,8,3,27]."""
    packed = np.ascontiguousarray(packed, np.float32)
    n = packed.shape[0]
    out = {}
    if mass:
        out["mass"] = np.full((n, 27, 27), np.nan, np.float32)
    if forces:
        out["forces"] = np.full((n, 3, 27), np.nan, np.float32)
    if jacobians:
        out["corner_jac"] = np.full((n, 8, 3, 27), np.nan, np.float32)
    ptr = lambda k: out[k].ctypes.data_as(C.c_void_p) if k in out else None
    load().eh_eom(int(kind), n, packed.ctypes.data_as(C.c_void_p), ptr("mass"), ptr("forces"), ptr("corner_jac"))
    return out
