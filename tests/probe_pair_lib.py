"""Builds and binds tests/device/ss_probe_pair.hip: the joint torques of a {leg, arm} pair of joints (ss_dynamics.hpp) beside the
scalar code they replace, one case per lane.
    host flavour:   compiled here for the CPU (hipcc --cuda-host-only) into tests/host/libss_probe_pair_host.so, numpy pointers;
    device flavour: steppingstone_amd/lib/libss_probe_pair.so, built for gfx950 by steppingstone_amd.build.build_probe_pair(), torch tensors.
TEST INFRASTRUCTURE; never imported by steppingstone_amd."""
import ctypes as C
import os
import subprocess

import numpy as np

import probe_lib

ROOT = probe_lib.ROOT
HOST_LIB = os.path.join(probe_lib.HOST_DIR, "libss_probe_pair_host.so")
SRC = os.path.join(ROOT, "tests", "device", "ss_probe_pair.hip")
OP = {"tau": 0}
hipcc = probe_lib.hipcc


def build_host():
    if probe_lib.host_ready(SRC, HOST_LIB):
        return HOST_LIB
    subprocess.check_call([hipcc(), "--cuda-host-only", "-x", "hip", "-O1", "-std=c++17", "-fno-signed-zeros", "-ffp-contract=on",
                           "-fPIC", "-shared", "-fno-math-errno", "-DSS_HOST_HARNESS", "-DSS_PROBE_HOST", SRC, "-o", HOST_LIB])
    return HOST_LIB


_libs = {}


def load(flavour):
    if flavour not in _libs:
        if flavour == "host":
            path = build_host()
        else:
            import torch                  # first, as in probe_lib.load: one HIP runtime per process
            torch.cuda.init()
            from steppingstone_amd import build
            path = build.build_probe_pair()
        lib = C.CDLL(path)
        lib.sspr_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.sspr_run.restype = C.c_int
        _libs[flavour] = lib
    return _libs[flavour]


def widths(flavour, op):
    w = load(flavour).sspr_run(OP[op], 0, 0, None, None, None)
    assert w > 0, w
    return w // 1000, w % 1000


def run(flavour, op, kind, inp):
    """inp [n, IN_W] float32 -> out [n, OUT_W] float32, every word moved as raw bits (NaN payloads survive)"""
    lib = load(flavour)
    iw, ow = widths(flavour, op)
    inp = np.ascontiguousarray(inp, np.float32)
    n = inp.shape[0]
    assert inp.shape == (n, iw), (op, inp.shape, iw)
    if flavour == "host":
        out = np.zeros((n, ow), np.float32)
        rc = lib.sspr_run(OP[op], int(kind), n, inp.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), None)
    else:
        import torch
        d_in = torch.from_numpy(inp.view(np.int32).copy()).to("cuda:0").contiguous()
        d_out = torch.full((n, ow), -1, dtype=torch.int32, device="cuda:0")
        stream = torch.cuda.current_stream(d_in.device)
        rc = lib.sspr_run(OP[op], int(kind), n, C.c_void_p(d_in.data_ptr()), C.c_void_p(d_out.data_ptr()), C.c_void_p(stream.cuda_stream))
        torch.cuda.synchronize()
        out = d_out.cpu().numpy().view(np.float32)
    assert rc == 0, "sspr_run(%s) returned %d" % (op, rc)
    return out
