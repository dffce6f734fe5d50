"""What the main wavefront of the three-helper K-step kernel executes per substep, counted on this tree's sources by
tools/isa_windows.py (hipcc -S of that one instantiation for gfx950; no GPU): no scratch, and fewer instructions than before the
joint torques of the {leg, arm} pairs went onto packed instructions -- the figure of profiles/stream_cut_isa_windows_new.txt, which
is read from that file.  The count is the compiler's: the test holds the direction of the cut, not its size."""
import os
import re
import subprocess
import sys

import pytest

import probe_lib

ROOT = probe_lib.ROOT
BEFORE = os.path.join(ROOT, "profiles", "stream_cut_isa_windows_new.txt")


def parse(text):
    res = re.search(r"'ScratchSize': (\d+)", text)
    ex = re.search(r"executed per substep: (\d+);", text)
    scratch_class = re.search(r"^\s+scratch\s+(\d+)\s+(\d+)\s+(\d+)\s*$", text, re.M)
    assert res and ex and scratch_class, text[-2000:]
    return int(res.group(1)), int(ex.group(1)), int(scratch_class.group(3))


def test_main_wavefront_executes_fewer_instructions_and_has_no_scratch():
    if not probe_lib.hipcc():
        pytest.skip("no hipcc: the kernel cannot be compiled to assembly")
    _, before, _ = parse(open(BEFORE).read())
    assert 5000 < before < 5500, before
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_windows.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         universal_newlines=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    scratch, executed, scratch_instr = parse(out.stdout)
    print("executed per substep: %d (before: %d), ScratchSize %d, scratch instructions executed %d" % (executed, before, scratch, scratch_instr))
    assert scratch == 0 and scratch_instr == 0
    assert executed < before
