"""The one recipe for the CPU builds of kernel code the tests load (hipcc --cuda-host-only): the host harness, the render and
kinematics hosts, the operator probe.  TEST INFRASTRUCTURE; never imported by steppingstone_amd."""
import glob
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_DIR = os.path.join(ROOT, "tests", "host")
CSRC = os.path.join(ROOT, "steppingstone_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include", "steppingstone.h")
# what every host library is compiled with; a library's own flags (build_host's extra_flags) come on top and differ on purpose
HOST_FLAGS = ["--cuda-host-only", "-x", "hip", "-O1", "-std=c++17", "-fPIC", "-shared", "-fno-signed-zeros", "-fno-math-errno",
              "-DSS_HOST_HARNESS"]


def hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def host_ready(src, lib):
    """lib exists and is newer than src, every header of the kernels and the C header"""
    deps = [src, INCLUDE] + glob.glob(os.path.join(CSRC, "*.hpp"))
    return os.path.exists(lib) and all(os.path.getmtime(d) <= os.path.getmtime(lib) for d in deps)


def build_host(src, lib, extra_flags=()):
    """lib from src unless host_ready.  The compiler's diagnostics stay on stderr: a compile error in a host build must be readable."""
    if host_ready(src, lib):
        return lib
    cc = hipcc()
    if not cc:
        raise FileNotFoundError("hipcc")
    subprocess.check_call([cc] + HOST_FLAGS + list(extra_flags) + [src, "-o", lib])
    return lib
