"""Builds and binds tests/device/ss_probe.hip: the step kernels' spatial algebra, contact stage, env formulas, one whole substep, the env
logic of a control step and the forms that must agree bitwise with the ones they replaced, behind one C entry, one operator per call.
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
    return lib


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
