"""The three-helper K-step kernel's main wavefront no longer evaluates joint_tau for the spine joints 0..2 in front of barrier #0b
(ss_dynamics.hpp, spine_tau_offload(): helper 1 evaluates them in front of #1 and hands tau / Dadd over in six words of Lambda_own's
place).  Counted on this tree's sources by tools/isa_windows.py (hipcc -S of that one instantiation for gfx950; no GPU), against
the parent's table in profiles/spine_tau_isa_windows_parent.txt (the same tool on the parent's sources; the same figures as
profiles/limb_tail_isa_windows_new.txt):

  * the main wavefront executes at most the parent's 4788 - 40 instructions per substep;
  * the control step's epilogue (static) has no more VALU instructions than the parent's 2040.  (The compare form of "at its limit",
    which took 146 of them, passed its bitwise checks and was measured slower together with the spine torques: it is not in,
    docs/HISTORY.md "Spine torques on helper 1", and its bound of 2040 - 120 is not asserted);
  * the sweep loop is still 214 instructions per pass;
  * no scratch, NumVgprs <= 256, LDSByteSize == 92160 (the hand-over uses words that are dead at that moment)."""
import os
import subprocess
import sys

import pytest

import probe_lib
from test_limb_tail_count import sweep_of
from test_reset_pose_count import parse

ROOT = probe_lib.ROOT
BEFORE = os.path.join(ROOT, "profiles", "limb_tail_isa_windows_new.txt")
PARENT = os.path.join(ROOT, "profiles", "spine_tau_isa_windows_parent.txt")
SUBSTEP, SWEEP, EPILOGUE_VALU = 4788, 214, 2040


def test_spine_torques_leave_the_main_wavefront():
    if not probe_lib.hipcc():
        pytest.skip("no hipcc: the kernel cannot be compiled to assembly")
    for path in (BEFORE, PARENT):
        text = open(path).read()
        p = parse(text)
        assert p["substep"] == SUBSTEP and p["epilogue_valu"] == EPILOGUE_VALU and sweep_of(text) == SWEEP, (path, p)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_windows.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         universal_newlines=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    new = dict(parse(out.stdout), sweep=sweep_of(out.stdout))
    print("executed per substep: %d (parent %d); sweep loop %d per pass; epilogue, static: %d VALU (parent %d); VGPRs %d, AGPRs %d, "
          "scratch %d, LDS %d" % (new["substep"], SUBSTEP, new["sweep"], new["epilogue_valu"], EPILOGUE_VALU, new["vgprs"], new["agprs"],
                                  new["scratch"], new["lds"]))
    assert new["substep"] <= SUBSTEP - 40
    assert new["epilogue_valu"] <= EPILOGUE_VALU
    assert new["sweep"] == SWEEP
    assert new["scratch"] == 0 and new["vgprs"] <= 256
    assert new["lds"] == 92160
