"""Builds and binds tests/host/lookahead_host.cpp: the look-ahead's code (steppingstone_amd/csrc/ss_lookahead.hpp) and the control step
it restates (step_env, auto-reset as an argument), compiled for the CPU with the host harness' own flags (tests/host_lib.py), so that
both round alike.  TEST INFRASTRUCTURE for the GPU-less container; never imported by steppingstone_amd."""
import ctypes as C
import os

import numpy as np

import native_build
from host_lib import INFO_DTYPE
from native_build import HOST_DIR

LIB = os.path.join(HOST_DIR, "liblookahead_host.so")
SRC = os.path.join(HOST_DIR, "lookahead_host.cpp")
DONE_FILL = 0xA5


def build():
    return native_build.build_host(SRC, LIB, ["-pthread"])


_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        vp = C.c_void_p
        _lib.lh_step.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_int, vp, C.c_float, C.c_int, vp, vp, vp, vp, vp, vp, vp]
        _lib.lh_lookahead.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_int, vp, C.c_float, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp,
                                      vp, vp, vp]
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def work_words():
    return int(load().lh_work_words())


def step(kind, packed, act, seed=0, curriculum=0, power=1.0, auto_reset=False):
    """one control step of ss_step on packed [N,186] under act [N,21] -> (packed_out, obs, rew, done, info)"""
    packed = np.ascontiguousarray(packed, np.float32)
    n = packed.shape[0]
    act = np.ascontiguousarray(act, np.float32).reshape(n, 21)
    out = np.zeros_like(packed)
    obs = np.zeros((n, 60), np.float32)
    rew = np.zeros(n, np.float32)
    done = np.zeros(n, np.uint8)
    info = np.zeros(n, INFO_DTYPE)
    load().lh_step(int(kind), n, int(seed), int(curriculum), None, float(power), int(bool(auto_reset)), _p(packed), _p(act), _p(out),
                   _p(obs), _p(rew), _p(done), _p(info))
    return out, obs, rew, done, info


def lookahead(kind, packed, act, env_ids=None, seed=0, curriculum=0, power=1.0, obs=True, final_state=True, state_after=False,
              fill=None):
    """kind 0 / 1; packed [N,186]; act [m,H,21] (m == N without env_ids) -> dict of ss_lookahead's outputs: rew [m,H], done [m,H]
    uint8, obs [m,H,60], final_state [m,186]; state_after: also "state" [N,186], the instance's state after the call.  fill: the word
    every f32 output holds before the call (default 0; `done` then holds DONE_FILL)."""
    packed = np.ascontiguousarray(packed, np.float32)
    n = packed.shape[0]
    ids = None if env_ids is None else np.ascontiguousarray(env_ids, np.int32)
    m = n if ids is None else ids.size
    act = np.ascontiguousarray(act, np.float32)
    assert act.ndim == 3 and act.shape[0] == m and act.shape[2] == 21
    h = act.shape[1]
    new = lambda shape: np.full(shape, 0 if fill is None else fill, np.float32)
    out = {"rew": new((m, h)), "done": np.full((m, h), 0 if fill is None else DONE_FILL, np.uint8)}
    if obs:
        out["obs"] = new((m, h, 60))
    if final_state:
        out["final_state"] = new((m, 186))
    if state_after:
        out["state"] = np.zeros_like(packed)
    work = np.zeros((max(m, 1), work_words()), np.float32)
    if m:
        load().lh_lookahead(int(kind), n, int(seed), int(curriculum), None, float(power), _p(packed), _p(ids), m, h, _p(act),
                            _p(out.get("obs")), _p(out["rew"]), _p(out["done"]), _p(out.get("final_state")), _p(work), _p(out.get("state")))
    elif state_after:
        out["state"][:] = packed
    return out
