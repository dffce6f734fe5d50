"""The three-helper K-step kernel's main wavefront hands the arm down-sweep, the arm joints' integration and the base's integration of
every substep to helper wavefronts (ss_dynamics.hpp, limb_tail_offload()), and with them the arm records, the base's rotation, the
quaternion and the free base twist, which it used to park in AGPRs across the rows and the PGS.  Counted on this tree's sources by
tools/isa_windows.py (hipcc -S of that one instantiation for gfx950; no GPU), against the parent's table in
profiles/limb_tail_isa_windows_parent.txt (the same tool on the parent's sources; the same figures as
profiles/reset_pose_isa_windows_new.txt) and the figures recorded in profiles/limb_tail_isa_windows_new.txt:

  * the main wavefront executes fewer instructions per substep than the parent's 4945: no more than the recorded 4788;
  * the sweep loop is still 214 instructions per pass;
  * no scratch, NumVgprs <= 256, LDSByteSize == 92160 (the hand-over uses words that are dead at that moment);
  * the control step's epilogue (static) has no more VALU instructions than the parent's 2044."""
import os
import re
import subprocess
import sys

import pytest

import probe_lib
from test_reset_pose_count import parse

ROOT = probe_lib.ROOT
BEFORE = os.path.join(ROOT, "profiles", "reset_pose_isa_windows_new.txt")
PARENT = os.path.join(ROOT, "profiles", "limb_tail_isa_windows_parent.txt")
NEW = os.path.join(ROOT, "profiles", "limb_tail_isa_windows_new.txt")
SUBSTEP, SWEEP, EPILOGUE_VALU = 4945, 214, 2044


def sweep_of(text):
    m = re.search(r"^\s+all\s+(\d+)\s+(\d+)\s+(\d+)\s*$", text, re.M)
    assert m, text[-2000:]
    return int(m.group(2))


def test_limb_tail_leaves_the_main_wavefronts_substep():
    if not probe_lib.hipcc():
        pytest.skip("no hipcc: the kernel cannot be compiled to assembly")
    before, parent, recorded = (open(p).read() for p in (BEFORE, PARENT, NEW))
    for text in (before, parent):
        p = parse(text)
        assert p["substep"] == SUBSTEP and p["epilogue_valu"] == EPILOGUE_VALU and sweep_of(text) == SWEEP, p
    recorded = dict(parse(recorded), sweep=sweep_of(recorded))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_windows.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         universal_newlines=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    new = dict(parse(out.stdout), sweep=sweep_of(out.stdout))
    print("executed per substep: %d (parent %d, recorded %d); sweep loop %d per pass; epilogue, static: %d VALU (parent %d, recorded %d); "
          "VGPRs %d, AGPRs %d, scratch %d, LDS %d" % (new["substep"], SUBSTEP, recorded["substep"], new["sweep"], new["epilogue_valu"],
                                                       EPILOGUE_VALU, recorded["epilogue_valu"], new["vgprs"], new["agprs"], new["scratch"],
                                                       new["lds"]))
    assert new["substep"] < SUBSTEP
    assert new["substep"] <= recorded["substep"] < SUBSTEP
    assert new["sweep"] == recorded["sweep"] == SWEEP
    assert new["scratch"] == 0 and new["vgprs"] <= 256
    assert new["lds"] == 92160
    assert new["epilogue_valu"] <= EPILOGUE_VALU
    assert new["epilogue_valu"] <= recorded["epilogue_valu"] <= EPILOGUE_VALU
