"""Builds and binds tests/host/lookahead_policy_host.cpp: the closed-loop look-ahead (look_row with the action source of
steppingstone_amd/csrc/ss_policy.hpp) compiled for the CPU with the flags of tests/lookahead_host_lib.py, and the host forms of
ss_policy_words / ss_policy_pack and of the MLP.
TEST INFRASTRUCTURE for the GPU-less container; never imported by steppingstone_amd."""
import ctypes as C
import os
import subprocess

import numpy as np

import native_build
import policy_nets
from native_build import HOST_DIR

LIB = os.path.join(HOST_DIR, "liblookahead_policy_host.so")
SRC = os.path.join(HOST_DIR, "lookahead_policy_host.cpp")
DEPS = [os.path.join(HOST_DIR, f) for f in ("lookahead_states_host.cpp", "lookahead_host.cpp")]
ASAN_SRC = os.path.join(HOST_DIR, "lookahead_policy_asan.cpp")
ASAN_BIN = os.path.join(HOST_DIR, "lookahead_policy_asan")
DONE_FILL = 0xA5
TAIL = 64                       # canary words behind every buffer
MAX_LAYERS = 8


class Desc(C.Structure):
    _fields_ = [("layers", C.c_int32), ("width", C.c_int32 * (MAX_LAYERS + 1)), ("activation", C.c_int32 * MAX_LAYERS)]


def desc_of(layers):
    d = Desc()
    d.layers = len(layers)
    d.width[0] = layers[0][0].shape[1]
    for i, (w, b, a) in enumerate(layers):
        d.width[i + 1] = w.shape[0]
        d.activation[i] = policy_nets.CODE[a]
    return d


def _newer(src, out):
    return os.path.exists(out) and all(os.path.getmtime(s) <= os.path.getmtime(out) for s in [src] + DEPS)


def build():
    if not _newer(SRC, LIB) and os.path.exists(LIB):
        os.remove(LIB)
    return native_build.build_host(SRC, LIB, ["-pthread"])


def build_asan():
    """the stand-alone program (its own main), compiled with AddressSanitizer and UBSan; never loaded into Python.  Flags as
    lookahead_states_host_lib.build_asan: the sanitizers are the host's alone, float-cast-overflow is off for ss_sincos' quadrant bits."""
    if native_build.host_ready(ASAN_SRC, ASAN_BIN) and _newer(SRC, ASAN_BIN):
        return ASAN_BIN
    flags = [f for f in native_build.HOST_FLAGS if f not in ("-shared", "-fPIC")]
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
        _lib.lhp_policy_words.restype = C.c_longlong
        _lib.lhp_policy_words.argtypes = [vp]
        _lib.lhp_policy_pack.argtypes = [vp, vp, vp, vp]
        _lib.lhp_policy_eval.argtypes = [vp, vp, C.c_int, vp, vp]
        _lib.lhp_lookahead_policy.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_int, vp, C.c_float, vp, vp, C.c_int, vp, C.c_int, vp, vp,
                                              vp, vp, vp, vp, vp, vp, vp, vp]
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def words(desc):
    return int(load().lhp_policy_words(C.byref(desc) if desc is not None else None))


def pack(layers):
    """-> (Desc, packed blob float32)"""
    d = desc_of(layers)
    n = words(d)
    assert n > 0
    ws = [np.ascontiguousarray(w, np.float32) for w, _, _ in layers]
    bs = [np.ascontiguousarray(b, np.float32) for _, b, _ in layers]
    wp = (C.c_void_p * len(layers))(*[w.ctypes.data for w in ws])
    bp = (C.c_void_p * len(layers))(*[b.ctypes.data for b in bs])
    blob = np.full(n, np.nan, np.float32)
    assert load().lhp_policy_pack(C.byref(d), wp, bp, _p(blob)) == 0
    return d, blob


def policy_eval(layers, x):
    d, blob = pack(layers)
    x = np.ascontiguousarray(x, np.float32)
    y = np.zeros((x.shape[0], 21), np.float32)
    assert load().lhp_policy_eval(C.byref(d), _p(blob), x.shape[0], _p(x), _p(y)) == 0
    return y


def lookahead_policy(kind, packed, layers, horizon, env_ids=None, states=None, offsets=None, seed=0, curriculum=0, power=1.0, fill=None,
                     want=("act", "obs", "final_state")):
    """ss_lookahead_policy over an instance that holds packed [N,186] -> dict: act [m,H,21], obs [m,H,60], rew, done, final_state
    [m,186] (those of `want`; the others are passed as NULL), state [N,186] (the instance after the call), tails_ok"""
    packed = np.ascontiguousarray(packed, np.float32)
    n = packed.shape[0]
    ids = None if env_ids is None else np.ascontiguousarray(env_ids, np.int32)
    m = n if ids is None else ids.size
    h = int(horizon)
    d, blob = pack(layers)
    f = np.float32(0 if fill is None else fill)
    width = {"act": h * 21, "obs": h * 60, "rew": h, "final_state": 186, "work": 160}
    raw = {k: np.full(m * w + TAIL, f, np.float32) for k, w in width.items() if k in want or k in ("rew", "work")}
    raw["done"] = np.full(m * h + TAIL, DONE_FILL, np.uint8)
    after = np.zeros_like(packed)
    if states is not None:
        states = np.ascontiguousarray(states, np.float32)
        assert states.shape == (m, 186)
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets, np.float32)
        assert offsets.shape == (m, h, 21)
    rc = load().lhp_lookahead_policy(int(kind), n, int(seed), int(curriculum), None, float(power), _p(packed), _p(ids), m, _p(states), h,
                                     C.byref(d), _p(blob), _p(offsets), _p(raw.get("act")), _p(raw.get("obs")), _p(raw["rew"]),
                                     _p(raw["done"]), _p(raw.get("final_state")), _p(raw["work"]), _p(after))
    assert rc == 0
    ok = all((v[-TAIL:].view(np.int32) == f.view(np.int32)).all() for k, v in raw.items() if k != "done")
    ok = ok and (raw["done"][-TAIL:] == DONE_FILL).all()
    shape = {"act": (m, h, 21), "obs": (m, h, 60), "rew": (m, h), "final_state": (m, 186)}
    out = {k: raw[k][:-TAIL].reshape(shape[k]) for k in shape if k in raw}
    out.update(done=raw["done"][:-TAIL].reshape(m, h), state=after, tails_ok=bool(ok))
    return out
