"""Builds and binds tests/device/ss_probe.hip: the step kernels' spatial algebra, contact stage, env formulas, one whole substep, the env
logic of a control step and the forms that must agree bitwise with the ones they replaced, behind one C entry, one operator per call;
and ssp_mlp, one MLP phase of the closed-loop look-ahead's policy (mlp()).
    host flavour:   compiled here for the CPU (the recipe of native_build.py) into tests/host/libss_probe_host.so, numpy pointers;
    device flavour: steppingstone_amd/lib/libss_probe.so, built for gfx950 by steppingstone_amd.build.build_probe(), torch tensors.
TEST INFRASTRUCTURE; never imported by steppingstone_amd."""
import ctypes as C
import os

import numpy as np

import native_build
from native_build import HOST_DIR, ROOT, hipcc  # noqa: F401  (re-exported: the tests ask this module for ROOT and hipcc())

HOST_LIB = os.path.join(HOST_DIR, "libss_probe_host.so")
SRC = os.path.join(ROOT, "tests", "device", "ss_probe.hip")

# the op numbers of ss_probe.hip's enum, in its order
OPS = ["rot", "rot2", "cross_r", "cross_rP", "xmotion", "xforce", "xmotionP", "xforceP", "xinertia", "xinertiaP", "abi_body",
       "abi_add_bodyP", "body_bias", "body_biasP", "imp_up", "imp_down", "imp_down_pair", "imp_up_pair", "imp_down_pair_loaded",
       "aba_acc", "aba_accP", "quat_rot", "mirror_sv", "abi_dense", "pack", "sincos", "chol", "xchg", "philox",
       "fk_detect", "jacobian_rows", "contact_ops", "sampler", "window_prob", "obs_terms", "substep",
       "pk_half", "limit_forms", "tau_pair", "step_score", "ep_return", "step_logic"]
OP = {name: i for i, name in enumerate(OPS)}
UNSUPPORTED = -2


def host_ready():
    """the host build exists and is newer than its sources"""
    return native_build.host_ready(SRC, HOST_LIB)


def build_host():
    # -ffp-contract=on as in the product's FLAGS: the probe's operators fuse on the CPU where they fuse on the GPU
    return native_build.build_host(SRC, HOST_LIB, ["-ffp-contract=on", "-pthread", "-DSS_PROBE_HOST"])


def _bind(path):
    lib = C.CDLL(path)
    lib.ssp_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ssp_run.restype = C.c_int
    lib.ssp_mlp.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.ssp_mlp.restype = C.c_int
    return lib


MAX_LAYERS, MAX_WIDTH, ROWS = 8, 256, 32
PREFILL = 0x7FC5A5A5          # a quiet NaN with a payload of its own: a stale word that is read turns up as a NaN, one left alone as these bits


class PolicyDesc(C.Structure):          # ss_policy_desc (include/steppingstone.h)
    _fields_ = [("layers", C.c_int32), ("width", C.c_int32 * (MAX_LAYERS + 1)), ("activation", C.c_int32 * MAX_LAYERS)]


def mlp(flavour, widths, codes, packed, x, prefill=PREFILL):
    """ssp_mlp: one MLP phase of the net (widths [layers + 1], activation codes [layers]) over the packed words `packed` on the rows
    x [n,60] -> the two activation blocks by row, uint32 bit patterns [32 * groups, 2, 256] (rows past n included: on the device they
    were staged as the prefill)."""
    lib = load(flavour)
    d = PolicyDesc()
    d.layers = len(codes)
    for i, w in enumerate(widths):
        d.width[i] = int(w)
    for i, a in enumerate(codes):
        d.activation[i] = int(a)
    x = np.ascontiguousarray(x, np.float32)
    packed = np.ascontiguousarray(packed, np.float32)
    n = x.shape[0]
    assert x.shape == (n, 60) and n > 0
    groups = (n + ROWS - 1) // ROWS
    words = groups * 2 * MAX_WIDTH * ROWS
    if flavour == "host":
        out = np.zeros(words, np.float32)
        rc = lib.ssp_mlp(C.byref(d), packed.ctypes.data_as(C.c_void_p), n, x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                         prefill, None)
    else:
        import torch
        up = lambda a: torch.from_numpy(a.view(np.int32).copy()).to("cuda:0").contiguous()
        d_p, d_x = up(packed), up(x)
        d_out = torch.zeros(words, dtype=torch.int32, device="cuda:0")
        stream = torch.cuda.current_stream(d_x.device)
        rc = lib.ssp_mlp(C.byref(d), C.c_void_p(d_p.data_ptr()), n, C.c_void_p(d_x.data_ptr()), C.c_void_p(d_out.data_ptr()), prefill,
                         C.c_void_p(stream.cuda_stream))
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
    assert rc == 0, "ssp_mlp returned %d" % rc
    return np.ascontiguousarray(out.view(np.uint32).reshape(groups, 2, MAX_WIDTH, ROWS).transpose(0, 3, 1, 2)).reshape(groups * ROWS, 2, MAX_WIDTH)


def c_fmaf(a, b, c):
    """the C library's fmaf, elementwise (host build)"""
    lib = load("host")
    a, b, c = (np.ascontiguousarray(v, np.float32) for v in (a, b, c))
    out = np.empty_like(a)
    lib.ssp_fmaf.argtypes = [C.c_int] + [C.c_void_p] * 4
    lib.ssp_fmaf.restype = None
    lib.ssp_fmaf(a.size, *[v.ctypes.data_as(C.c_void_p) for v in (a, b, c, out)])
    return out


_libs = {}


def load(flavour):
    if flavour not in _libs:
        if flavour == "host":
            _libs[flavour] = _bind(build_host())
        else:
            # torch first, as everywhere in the package: the probe library then binds to the HIP runtime torch has loaded and
            # initialised.  Loaded the other way round, the process ends up with two HIP runtimes and the second finds no device.
            import torch
            torch.cuda.init()
            from steppingstone_amd import build
            _libs[flavour] = _bind(build.build_probe())
    return _libs[flavour]


def widths(flavour, op):
    """(IN_W, OUT_W) of an op, as the library itself states them."""
    w = load(flavour).ssp_run(OP[op], 0, 0, None, None, None)
    assert w > 0, "ssp_run(%s): %d" % (op, w)
    return w // 1000, w % 1000


def run(flavour, op, kind, inp):
    """inp [n, IN_W] float32 (raw bits where the op wants integers) -> out [n, OUT_W] float32, or None where the flavour does not
    support the op.  kind: 0 walker3d, 1 mike."""
    lib = load(flavour)
    iw, ow = widths(flavour, op)
    inp = np.ascontiguousarray(inp, np.float32)
    n = inp.shape[0]
    assert inp.shape == (n, iw), (op, inp.shape, iw)
    if flavour == "host":
        out = np.full((n, ow), np.nan, np.float32)
        rc = lib.ssp_run(OP[op], int(kind), n, inp.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), None)
    else:
        import torch
        # bit-preserving upload: some columns hold integer words that are NaN patterns as floats
        d_in = torch.from_numpy(inp.view(np.int32).copy()).to("cuda:0").contiguous()
        d_out = torch.full((n, ow), -1, dtype=torch.int32, device="cuda:0")
        stream = torch.cuda.current_stream(d_in.device)
        rc = lib.ssp_run(OP[op], int(kind), n, C.c_void_p(d_in.data_ptr()), C.c_void_p(d_out.data_ptr()), C.c_void_p(stream.cuda_stream))
        torch.cuda.synchronize()
        out = d_out.cpu().numpy().view(np.float32)
    if rc == UNSUPPORTED:
        return None
    assert rc == 0, "ssp_run(%s) returned %d" % (op, rc)
    return out
