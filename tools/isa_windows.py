"""Static instruction counts of the three-helper rollout kernel between its barriers (hipcc -S of that one instantiation; no
GPU needed): which wavefront issues how many VALU instructions in which window of a substep -- the numbers behind DESIGN.md
section 5.1's window table and section 9's "what is left".  The compiler lays the code out as: prologue | helper wavefronts
(#0->#0b cos/sin, #0b->#1 kinematics / detection / rows / bias / extra, #1->#2 operators part A, #2->#3 part B) | main wavefront
(#0->#0b joint torques, #0b->#1 pass 1 + leg/arm half of pass 2, #1->#2 spine + base factorisation, #2->#3 pass 3 + foot twist,
#3->end: rows y = Lambda w, the PGS (its sweep loop appears ONCE here and runs kPgsIters - 1 times, the last sweep is straight-line
code behind it), response of the tree, integration and the control step's epilogue) | tail.  With limb_tail_offload() (ss_dynamics.hpp) the
table has two windows more per side, split at every s_barrier like the rest: helpers #3->#3r (the reset pose), #3r->the barrier in front of
the epilogue (helper 1: arm down-sweep and arm joints, helper 2: the base's integration, both in the one window of the layout); main
wavefront #3->#3r (rows y = Lambda w, PGS, response up to dv0), #3r->epilogue barrier (spine + leg down-sweep, eight joints' integration).

Below the window table: the instructions the main wavefront EXECUTES per substep, by class -- every line of its substep loop once
(every branch inside it taken as falling through: the contact branch is always taken at the benchmark's workload) and the lines of
the sweep loop kPgsIters - 1 times.  The classes that produce no value are listed apart: register copies (v_mov_b32 from a register;
DPP moves are lane exchanges and not among them), literal materialisation (v_mov_b32 / s_mov_b32 of a 32-bit literal), AGPR <-> VGPR
moves and s_nop.

usage: python tools/isa_windows.py [extra hipcc flags]                 the sources of this tree
       python tools/isa_windows.py --csrc DIR [extra hipcc flags]      the headers in DIR (a copy of steppingstone_amd/csrc of another
                                                                       commit, its include/ two levels up as in the tree): A/B tables"""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from steppingstone_amd.build import FLAGS, NO_MAX_ILP, OPTIONAL_FLAGS, hipcc  # noqa: E402

# the kernel lives in ss_rollout3.hip: compiled as build.py compiles that unit
FLAGS = FLAGS + ([] if "ss_rollout3.hip" in NO_MAX_ILP else OPTIONAL_FLAGS)
KERNEL = "_ZN2ss21rollout_kernel_helpedINS_13ModelWalker3DELi3EEEvNS_6ParamsENS_6StepIOE"


def cls(op, args=""):
    if op.startswith("v_pk_"):
        return "packed f32"
    if re.match(r"v_(fma|fmac|mul|add|sub|subrev|fmamk|fmaak|mac)_f32", op):
        return "scalar f32"
    if op.startswith("v_accvgpr"):
        return "agpr moves"
    if op.startswith("v_mov_b32"):
        if "quad_perm" in args or "row_" in args:
            return "other VALU"          # a DPP move is a lane exchange
        src = args.split(",")[1].strip().split()[0] if "," in args else ""
        return "v_mov reg" if re.match(r"(v\d|s\d|v\[|s\[|vcc|exec|m0)", src) else "v_mov lit"
    if op.startswith("v_"):
        return "other VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith("s_waitcnt"):
        return "s_waitcnt"
    if op == "s_nop":
        return "s_nop"
    if op.startswith("s_"):
        return "scalar ALU"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "scratch" if op.startswith("scratch_") else "global memory"
    return "other"


COLS = ["packed f32", "scalar f32", "agpr moves", "v_mov reg", "v_mov lit", "s_nop", "other VALU", "LDS", "scalar ALU", "global memory", "scratch",
        "s_waitcnt"]
VALU = COLS[:5] + ["other VALU"]
INSTR = re.compile(r"\s+([a-z_0-9]+)\s*(.*)")


def count(lines):
    c = collections.Counter()
    for l in lines:
        m = INSTR.match(l)
        if m and not l.strip().startswith((".", ";")):
            c[cls(m.group(1), m.group(2))] += 1
            if m.group(1) == "s_mov_b32" and re.search(r",\s*0x[0-9a-f]+$", l.rstrip()):
                c["s_mov lit"] += 1
    return c


def blocks(body):
    """[(label, the compiler's loop comment, lines)] of the basic blocks: a block starts at a label or at a '; %bb.N:' comment"""
    out, cur = [], None
    for l in body:
        m = re.match(r"(?:\.L(BB\d+_\d+):|; %bb\.(\d+):)(.*)", l)
        if m:
            cur = [m.group(1) or "bb." + m.group(2), m.group(3), []]
            out.append(cur)
        elif cur is not None:
            if not cur[2] and re.match(r"\s+;", l):
                cur[1] += " " + l.strip()        # the comment goes on over the next lines
            else:
                cur[2].append(l)
    return out


def main():
    argv = sys.argv[1:]
    csrc = os.path.join(ROOT, "steppingstone_amd", "csrc")
    given = "--csrc" in argv
    if given:
        i = argv.index("--csrc")
        csrc = os.path.abspath(argv[i + 1])
        argv = argv[:i] + argv[i + 2:]
    with tempfile.TemporaryDirectory() as d:
        src, out = os.path.join(d, "one.hip"), os.path.join(d, "one.s")
        open(src, "w").write('#include <hip/hip_runtime.h>\n#include "%s"\ntemplate __global__ void ss::rollout_kernel_helped<ss::ModelWalker3D, 3>'
                             '(ss::Params, ss::StepIO);\n' % os.path.join(csrc, "ss_kernels.hpp"))
        subprocess.check_call([hipcc()] + FLAGS + argv + ["-S", "--cuda-device-only", src, "-o", out],
                              stderr=subprocess.DEVNULL)
        text = open(out).read().split("\n")
    m = re.search(r"constexpr int kPgsIters = (\d+);", open(os.path.join(csrc, "ss_dynamics.hpp")).read())
    sweeps = int(m.group(1)) - 1           # the sweep loop's trip count
    a = next(i for i, l in enumerate(text) if l.startswith(KERNEL + ":"))
    b = next(i for i in range(a, len(text)) if "s_endpgm" in text[i])
    body = text[a:b + 1]
    res = {}
    for l in text[b:]:
        m = re.match(r"^; (NumVgprs|NumAgprs|ScratchSize|LDSByteSize): (\d+)", l)
        if m and m.group(1) not in res:
            res[m.group(1)] = int(m.group(2))
        if len(res) == 4:
            break
    print("sources: %s" % ("the directory given with --csrc" if given else "this tree"))
    print("kernel rollout_kernel_helped<Walker3D,3>: %s" % res)
    bars = [i for i, l in enumerate(body) if re.match(r"\s+s_barrier", l)]
    marks = [0] + bars + [len(body)]
    print("%-14s %6s | %s" % ("ISA lines", "VALU", " ".join("%13s" % c for c in COLS)))
    for lo, hi in zip(marks[:-1], marks[1:]):
        c = count(body[lo:hi])
        valu = sum(c[k] for k in VALU)
        if valu or c["LDS"]:
            print("%6d-%-7d %6d | %s" % (lo, hi, valu, " ".join("%13d" % c[k] for k in COLS)))
    # the main wavefront's substep loop: the last depth-2 loop that has a depth-3 loop inside (the helpers' loops come first in the layout)
    bl = blocks(body)
    heads = [lab for lab, com, _ in bl if re.search(r"This Loop Header: Depth=2", com)
             and any("Depth=3" in c2 and re.search(r"Parent Loop %s Depth=2" % lab, c2) for _, c2, _ in bl)]
    if not heads:
        print("no substep loop with a sweep loop inside found: no executed-per-substep count")
        return
    head = heads[-1]
    mine = [(lab, com, ls) for lab, com, ls in bl if lab == head or re.search(r"(Header=|Parent Loop )%s Depth=2" % head, com)]
    once = count([l for _, _, ls in mine for l in ls])
    sweep = count([l for _, com, ls in mine if "Depth=3" in com for l in ls])
    # `once` holds the sweep loop's lines once already: the other sweeps - 1 passes are added
    ex = collections.Counter({k: once[k] + (sweeps - 1) * sweep[k] for k in set(once) | set(sweep)})
    print("main wavefront, substep loop %s: %d basic blocks, sweep loop x %d" % (head, len(mine), sweeps))
    skip = ("other", "s_mov lit")
    print("  %-22s %9s %9s %9s" % ("class", "loop once", "sweep", "executed"))
    for k in COLS + ["s_mov lit"]:
        print("  %-22s %9d %9d %9d%s" % (k, once[k], sweep[k], ex[k], "   (among scalar ALU)" if k == "s_mov lit" else ""))
    tot = lambda c: sum(v for k, v in c.items() if k not in skip)
    print("  %-22s %9d %9d %9d" % ("all", tot(once), tot(sweep), tot(ex)))
    print("  executed per substep: %d; of them without a value (v_mov reg + v_mov lit + s_mov lit + agpr moves + s_nop): %d"
          % (tot(ex), ex["v_mov reg"] + ex["v_mov lit"] + ex["s_mov lit"] + ex["agpr moves"] + ex["s_nop"]))
    # the control step's epilogue: the basic blocks of the main wavefront's control-step loop (the substep loop's parent) that the layout
    # has behind the substep loop's last one.  A STATIC count (its branches -- reset, target advance -- are not all taken in a step): for
    # A/B tables of the same code, not for clocks
    last = max(i for i, (lab, com, _) in enumerate(bl) if lab == head or re.search(r"(Header=|Parent Loop )%s Depth=2" % head, com))
    outer = re.search(r"Parent Loop (BB\d+_\d+) Depth=1", next(com for lab, com, _ in bl if lab == head)).group(1)
    behind = count([l for _, com, ls in bl[last + 1:] if re.search(r"Header=%s Depth=1" % outer, com) for l in ls])
    print("main wavefront, behind the substep loop (the control step's epilogue, static): %d VALU, %d LDS, %d global memory, %d in all"
          % (sum(behind[k] for k in VALU), behind["LDS"], behind["global memory"], tot(behind)))


if __name__ == "__main__":
    main()
