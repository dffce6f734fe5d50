"""Builds and binds tests/host/lookahead_states_host.cpp: the look-ahead from caller-supplied state rows and the observation of a state
row (steppingstone_amd/csrc/ss_lookahead.hpp) compiled for the CPU with the flags of tests/lookahead_host_lib.py, whose lh_step and
lh_lookahead the library holds as well (bound here too, so that both sides of every comparison come from one build).  TEST
INFRASTRUCTURE for the GPU-less container; never imported by steppingstone_amd."""
import ctypes as C
import os
import subprocess

import numpy as np

import native_build
from native_build import HOST_DIR

LIB = os.path.join(HOST_DIR, "liblookahead_states_host.so")
SRC = os.path.join(HOST_DIR, "lookahead_states_host.cpp")
ASAN_SRC = os.path.join(HOST_DIR, "lookahead_states_asan.cpp")
ASAN_BIN = os.path.join(HOST_DIR, "lookahead_states_asan")
DONE_FILL = 0xA5
TAIL = 64                       # canary words behind every buffer


def build():
    return native_build.build_host(SRC, LIB, ["-pthread"])


def build_asan():
    """the stand-alone containment program (its own main), compiled with AddressSanitizer and UBSan; never loaded into Python"""
    if native_build.host_ready(ASAN_SRC, ASAN_BIN) and os.path.getmtime(SRC) <= os.path.getmtime(ASAN_BIN):
        return ASAN_BIN
    flags = [f for f in native_build.HOST_FLAGS if f not in ("-shared", "-fPIC")]
    # Every finding ends the program (-fno-sanitize-recover).  One check of the `undefined` group is off: float-cast-overflow.  The
    # substeps' own trigonometry (ss_sincos, ss_dynamics.hpp) converts the rounded angle to int for its quadrant bits, and a NaN joint
    # angle -- which a NaN action gives ss_step and ss_lookahead just as well -- is outside int: a value, never an index, and the
    # non-finite guard ends that episode.  The conversions of the row's own integer words (row_int, row_u32) are defined for every float.
    # The sanitizers are the HOST's alone: every one of their options goes through -Xarch_host, and the compile is host-only anyway.
    subprocess.check_call([native_build.hipcc()] + flags + ["-g", "-Xarch_host", "-fsanitize=address,undefined",
                                                            "-Xarch_host", "-fno-sanitize=float-cast-overflow",
                                                            "-Xarch_host", "-fno-sanitize-recover=all", "-pthread", ASAN_SRC, "-o", ASAN_BIN])
    return ASAN_BIN


_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        vp = C.c_void_p
        _lib.lh_lookahead.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_int, vp, C.c_float, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp,
                                      vp, vp, vp]
        _lib.lhs_lookahead_states.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_int, vp, C.c_float, vp, vp, C.c_int, vp, C.c_int, vp, vp,
                                              vp, vp, vp, vp, vp]
        _lib.lhs_observe.argtypes = [C.c_int, C.c_int, vp, vp]
        _lib.lhs_get_obs.argtypes = [C.c_int, C.c_int, vp, vp]
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def lookahead(kind, packed, act, env_ids=None, states=None, seed=0, curriculum=0, power=1.0, fill=None):
    """ss_lookahead (states None) or ss_lookahead_states over an instance that holds packed [N,186]: act [m,H,21], env_ids [m] (None:
    0..m-1, m == N), states [m,186] -> dict: obs [m,H,60], rew [m,H], done [m,H] uint8, final_state [m,186], state [N,186] (the
    instance after the call).  Every output is allocated with TAIL canary words behind it, filled with `fill` (default 0; done:
    DONE_FILL); "tails_ok": no canary word was written."""
    packed = np.ascontiguousarray(packed, np.float32)
    n = packed.shape[0]
    ids = None if env_ids is None else np.ascontiguousarray(env_ids, np.int32)
    m = n if ids is None else ids.size
    act = np.ascontiguousarray(act, np.float32)
    assert act.ndim == 3 and act.shape[0] == m and act.shape[2] == 21 and m > 0
    h = act.shape[1]
    f = np.float32(0 if fill is None else fill)
    width = {"obs": h * 60, "rew": h, "final_state": 186, "work": 160}
    raw = {k: np.full(m * w + TAIL, f, np.float32) for k, w in width.items()}
    raw["done"] = np.full(m * h + TAIL, DONE_FILL, np.uint8)
    after = np.zeros_like(packed)
    lib = load()
    if states is None:
        lib.lh_lookahead(int(kind), n, int(seed), int(curriculum), None, float(power), _p(packed), _p(ids), m, h, _p(act), _p(raw["obs"]),
                         _p(raw["rew"]), _p(raw["done"]), _p(raw["final_state"]), _p(raw["work"]), _p(after))
    else:
        states = np.ascontiguousarray(states, np.float32)
        assert states.shape == (m, 186)
        lib.lhs_lookahead_states(int(kind), n, int(seed), int(curriculum), None, float(power), _p(packed), _p(ids), m, _p(states), h,
                                 _p(act), _p(raw["obs"]), _p(raw["rew"]), _p(raw["done"]), _p(raw["final_state"]), _p(raw["work"]),
                                 _p(after))
    ok = all((v[-TAIL:].view(np.int32) == f.view(np.int32)).all() for k, v in raw.items() if k != "done")
    ok = ok and (raw["done"][-TAIL:] == DONE_FILL).all()
    return dict(obs=raw["obs"][:-TAIL].reshape(m, h, 60), rew=raw["rew"][:-TAIL].reshape(m, h), done=raw["done"][:-TAIL].reshape(m, h),
                final_state=raw["final_state"][:-TAIL].reshape(m, 186), state=after, tails_ok=bool(ok))


def observe(kind, states):
    """ss_get_obs_states: states [m,186] -> obs [m,60]"""
    states = np.ascontiguousarray(states, np.float32)
    obs = np.zeros((states.shape[0], 60), np.float32)
    load().lhs_observe(int(kind), states.shape[0], _p(states), _p(obs))
    return obs


def get_obs(kind, packed):
    """ss_set_state(packed) + ss_get_obs on an instance of packed.shape[0] envs -> obs [N,60]"""
    packed = np.ascontiguousarray(packed, np.float32)
    obs = np.zeros((packed.shape[0], 60), np.float32)
    load().lhs_get_obs(int(kind), packed.shape[0], _p(packed), _p(obs))
    return obs
