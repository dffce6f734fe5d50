"""Builds and binds tests/host/forces_host.cpp: the force readout's code (steppingstone_amd/csrc/ss_forces.hpp) compiled for the CPU
with the host harness' own flags (tests/host_lib.py), so that both round alike.  TEST INFRASTRUCTURE for the GPU-less container;
never imported by steppingstone_amd."""
import ctypes as C
import os

import numpy as np

import native_build
from native_build import HOST_DIR

LIB = os.path.join(HOST_DIR, "libforces_host.so")
SRC = os.path.join(HOST_DIR, "forces_host.cpp")


def build():
    return native_build.build_host(SRC, LIB, ["-pthread"])


_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        vp = C.c_void_p
        _lib.fh_step_forces.argtypes = [C.c_int, C.c_int, vp, vp, C.c_int, vp, C.c_float, vp, vp, vp, vp]
    return _lib


def step_forces(kind, packed, act, env_ids=None, power=1.0, contacts=True, joints=True, next_state=True, state_after=False):
    """kind 0 / 1; packed [N,186]; act [m,21] (m == N without env_ids) -> dict of the requested outputs of ss_step_forces: contacts
    [m,4,8,8], joints [m,4,4,21], next_state [m,56]; state_after: also "state" [N,186], the instance's state after the call."""
    packed = np.ascontiguousarray(packed, np.float32)
    n = packed.shape[0]
    ids = None if env_ids is None else np.ascontiguousarray(env_ids, np.int32)
    m = n if ids is None else ids.size
    act = np.ascontiguousarray(act, np.float32).reshape(m, 21)
    out = {}
    if contacts:
        out["contacts"] = np.zeros((m, 4, 8, 8), np.float32)
    if joints:
        out["joints"] = np.zeros((m, 4, 4, 21), np.float32)
    if next_state:
        out["next_state"] = np.zeros((m, 56), np.float32)
    if state_after:
        out["state"] = np.zeros_like(packed)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    load().fh_step_forces(int(kind), n, ptr(packed), ptr(ids), m, ptr(act), float(power), ptr(out.get("contacts")), ptr(out.get("joints")),
                          ptr(out.get("next_state")), ptr(out.get("state")))
    return out
