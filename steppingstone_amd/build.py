"""Build libsteppingstone.so (hand-written HIP for gfx950) in-tree with hipcc.

hipcc cross-compiles without a GPU, so this runs in the GPU-less build container; the resulting .so travels to the
GPU box with the repository snapshot.

    python -m steppingstone_amd.build [--force] [--fuzz]      the product library (and the schedule-fuzzed test build)
    python -m steppingstone_amd.build --variant NAME [hipcc flags ...]
                                                              var/libss_NAME.so: the same recipe plus the given flags (-DSS_PGS_ITERS=...,
                                                              -DSS_PROFILE_PHASES, ...), for A/B runs through STEPPINGSTONE_LIB
"""
import os
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
LIBDIR = os.path.join(PKG, "lib")
LIB = os.path.join(LIBDIR, "libsteppingstone.so")
SOURCES = ["ss_api.hip", "ss_rollout3.hip", "ss_render.hip", "ss_kinematics.hip", "ss_forces.hip", "ss_eom.hip", "ss_push.hip", "ss_lookahead.hip", "ss_policy.hip"]
# ss_rollout3.hip (the three-helper rollout kernel) is compiled without the max-ILP scheduling strategy: see its header.  So is
# ss_render.hip: the render kernel is 9 % faster without it (4096 envs at 64 x 64, RGB + depth + seg, shadows: 0.889 against 0.977 ms
# per call; DESIGN.md "Rendering").  So is ss_kinematics.hip: the strategy buys the readout no time and costs it registers -- 64 VGPRs
# without it, 87 with it, at the same time per call within the spread between processes (DESIGN.md 5.3 has both builds' figures).
# ss_forces.hip (the force readout: the plain step kernel's substeps) keeps the strategy: 256 VGPRs + 256 AGPRs either way, but no scratch
# with it against 236 B per lane without, and 90 against 112 us per call at 4096 envs, 119 against 148 at 32768.
# ss_eom.hip (the equation-of-motion readout) keeps it as well: with and without it the kernel takes the same 216 VGPRs, 148 B of scratch
# per lane and 41 536 B of LDS (occupancy 2 waves per SIMD either way), so the resources give no reason to leave the default
# ss_push.hip (the impulse) keeps it too: 243 against 242 VGPRs, 148 B of scratch, 54 688 B of LDS and occupancy 2 either way, and 63.5
# against 63.2 us per call at 4096 envs, 432.7 against 434.9 at 32768
# ss_lookahead.hip (the look-ahead: the plain step kernel's substeps, H control steps per launch) keeps it: 256 VGPRs + 254 AGPRs and no
# scratch with it, 256 + 256 and 180 B per lane without, and 1074 against 1112 us per call of 16 steps at 4096 rows, 1138 against 1188
# at 32768.  Its second instantiation, the look-ahead from caller-supplied state rows, has the same figures, and the
# observation of state rows (one lane per row) takes 156 VGPRs and no scratch.
# ss_policy.hip (the closed-loop look-ahead: look_row with an MLP between the control steps, four wavefronts per workgroup) keeps it, as
# the look-ahead whose per-lane code it instantiates (DESIGN.md 5.3 has its figures).
NO_MAX_ILP = {"ss_rollout3.hip", "ss_render.hip", "ss_kinematics.hip"}
HEADERS = ["ss_math.hpp", "ss_pair.hpp", "ss_dynamics.hpp", "ss_kernels.hpp", "ss_model_tables.hpp", "ss_render.hpp", "ss_visual_tables.hpp", "ss_kinematics.hpp", "ss_forces.hpp", "ss_eom.hpp", "ss_push.hpp", "ss_lookahead.hpp", "ss_policy.hpp",
           os.path.join("..", "..", "include", "steppingstone.h")]
# -O3 without the SLP vectorizer, signed zeros not honoured.  Measured on gfx950 / ROCm 7.2:
#   * SLP vectorisation (packed v_pk_fma_f32 / v_pk_mul_f32) miscompiled the 1-env-per-lane kernel of v1-v3 (wrong,
#     run-to-run varying results next to KBs of scratch); the current kernel passes parity with it but is 30 %
#     slower (aligned register pairs -> 536 B/lane of scratch): -fno-slp-vectorize stays;
#   * -fno-signed-zeros lets the compiler drop the "+ 0" of zero-initialised accumulators and fold x*y+0 into a
#     multiply: 0.1068 -> 0.1026 ms/step, all GPU parity tests green (it had triggered the v1-v3 miscompile too, so
#     it is re-validated by the full GPU suite on every build change);
#   * -fassociative-math would give another 1.5 % but re-orders the sums of the spec: not used.
# No other fast-math flags: -ffinite-math-only would delete the non-finite guard of PHYSICS.md 4.8.
#   * -ffp-contract=on (fuse a*b+c only inside one source expression) instead of HIP's default "fast": the kernel
#     variants (with / without helper wavefronts) then round identically, so results do not depend on batch size or on
#     the number of GPUs a batch is sharded over (bitwise; tested).  Costs 3 % on the plain variant, nothing on the
#     helper variant.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-slp-vectorize", "-fno-signed-zeros",
         "-ffp-contract=on"]
# scheduling only (no effect on values): the max-ILP machine scheduler is worth 1.4 % on the step kernel.  It is an
# -mllvm option, so build() falls back to the plain flags if a compiler does not know it.
OPTIONAL_FLAGS = ["-mllvm", "-amdgpu-sched-strategy=max-ilp"]

def hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    return "hipcc"


def _up_to_date(lib, deps):
    """lib exists and no dependency that exists is newer"""
    return os.path.exists(lib) and all(os.path.getmtime(d) <= os.path.getmtime(lib) for d in deps if os.path.exists(d))


def stale(lib=LIB):
    return not _up_to_date(lib, [os.path.join(CSRC, s) for s in SOURCES + HEADERS])


FUZZ_LIB = os.path.join(LIBDIR, "libsteppingstone_fuzz.so")
VARDIR = os.path.join(os.path.dirname(PKG), "var")      # git-ignored: tuning variants


def _compile_lib(out, extra_flags, tag, verbose):
    """Every translation unit in parallel, then the link.  A compiler that does not know the optional -mllvm flag gets the plain
    flags on a second pass; that pass keeps its diagnostics (a genuine compile error must be readable)."""
    objdir = os.path.join(LIBDIR, "obj")
    os.makedirs(objdir, exist_ok=True)

    def compile_one(src, with_optional, quiet):
        obj = os.path.join(objdir, src.replace(".hip", tag + ".o"))
        cmd = [hipcc()] + FLAGS + extra_flags + (OPTIONAL_FLAGS if with_optional else []) + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        return obj, subprocess.Popen(cmd, stderr=subprocess.DEVNULL if quiet else None)

    for with_optional in (True, False):
        jobs = [compile_one(src, with_optional and src not in NO_MAX_ILP, quiet=with_optional and not verbose) for src in SOURCES]
        rcs = [p.wait() for _, p in jobs]
        if all(rc == 0 for rc in rcs):
            break
        if not with_optional:
            raise subprocess.CalledProcessError(max(rcs), "hipcc -c (diagnostics above)")
    cmd = [hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC"] + [o for o, _ in jobs] + ["-o", out]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return out


def build_fuzz(force=False, verbose=False):
    """The -DSS_FUZZ_SCHED build of the same sources (lib/libsteppingstone_fuzz.so): every wavefront sleeps a pseudo-random time at the
    start of each barrier window.  TEST BUILD -- tests/test_gpu_sched_fuzz.py requires its results to be bit-identical to the
    product library's; nothing in the package loads it."""
    if not force and not stale(FUZZ_LIB):
        return FUZZ_LIB
    os.makedirs(LIBDIR, exist_ok=True)
    return _compile_lib(FUZZ_LIB, ["-DSS_FUZZ_SCHED"], "_fuzz", verbose)


PROBE_LIB = os.path.join(LIBDIR, "libss_probe.so")
PROBE_SRC = os.path.join(os.path.dirname(PKG), "tests", "device", "ss_probe.hip")


def build_probe(force=False, verbose=False):
    """lib/libss_probe.so from tests/device/ss_probe.hip: the step kernels' spatial algebra, contact stage, env formulas, one substep
    and the forms that replaced older ones, behind one C entry, one operator per launch, compiled with the product's FLAGS (so the
    operators round as they do inside the step kernels).  TEST BUILD -- tests/test_spatial_ops.py, test_contact_ops.py and
    test_substep.py hold the operators against fp64 references, test_pair_broadcast.py, test_limit_forms.py and test_pair_response.py
    hold the new forms to the old ones bitwise; nothing in the package loads it."""
    if not force and _up_to_date(PROBE_LIB, [PROBE_SRC] + [os.path.join(CSRC, h) for h in HEADERS]):
        return PROBE_LIB
    os.makedirs(LIBDIR, exist_ok=True)
    cmd = [hipcc()] + FLAGS + ["-shared", PROBE_SRC, "-o", PROBE_LIB]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return PROBE_LIB


def build_variant(name, extra_flags, verbose=False):
    """var/libss_<name>.so: the product recipe plus extra_flags.  A tuning build: nothing in the package loads it (point
    STEPPINGSTONE_LIB at it: tools/ab_libs.sh, tools/state_hash.py, tools/sched_fuzz.py)."""
    os.makedirs(VARDIR, exist_ok=True)
    return _compile_lib(os.path.join(VARDIR, "libss_%s.so" % name), list(extra_flags), "_var_" + name, verbose)


def build(force=False, verbose=False):
    if not force and not stale():
        return LIB
    os.makedirs(LIBDIR, exist_ok=True)
    return _compile_lib(LIB, [], "", verbose)


if __name__ == "__main__":
    if "--variant" in sys.argv:
        i = sys.argv.index("--variant")
        print(build_variant(sys.argv[i + 1], sys.argv[i + 2:], verbose=True))
        sys.exit(0)
    build(force="--force" in sys.argv, verbose=True)
    if "--fuzz" in sys.argv:
        build_fuzz(force="--force" in sys.argv, verbose=True)
    print(LIB)
