"""The contact response of the three-helper K-step kernel reads the spine + leg joint records and the base factor back from the hand-off
region (ss_dynamics.hpp, response_from_lds()) instead of carrying them through the rows and the PGS in AGPR copies.  Counted on this
tree's sources by tools/isa_windows.py (hipcc -S of that one instantiation for gfx950; no GPU): the main wavefront executes fewer
instructions per substep than the parent did (profiles/resp_lds_isa_windows_parent.txt, read from that file: 5053) and no more than
the 4951 of the crude first form (all the loads directly in front of the response; docs/HISTORY.md has every form that was counted),
and without scratch.  The AGPR moves, the LDS instructions, the sweep loop's count per pass and the packed / scalar f32 counts are
printed beside the parent's; they are not asserted, later changes are free to move them."""
import os
import re
import subprocess
import sys

import pytest

import probe_lib

ROOT = probe_lib.ROOT
PARENT = os.path.join(ROOT, "profiles", "resp_lds_isa_windows_parent.txt")
FIRST_FORM = 4951


def parse(text):
    scratch = re.search(r"'ScratchSize': (\d+)", text)
    ex = re.search(r"executed per substep: (\d+);", text)
    rows = {}
    for k in ("packed f32", "scalar f32", "agpr moves", "LDS", "all"):
        m = re.search(r"^\s+%s\s+(\d+)\s+(\d+)\s+(\d+)\s*$" % k, text, re.M)
        assert m, (k, text[-2000:])
        rows[k] = tuple(int(g) for g in m.groups())       # loop once, one pass of the sweep loop, executed
    assert scratch and ex, text[-2000:]
    return int(scratch.group(1)), int(ex.group(1)), rows


def test_response_from_lds_shortens_the_main_wavefronts_stream():
    if not probe_lib.hipcc():
        pytest.skip("no hipcc: the kernel cannot be compiled to assembly")
    _, parent, prow = parse(open(PARENT).read())
    assert 5000 < parent < 5100, parent
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_windows.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         universal_newlines=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    scratch, executed, row = parse(out.stdout)
    print("executed per substep: %d (parent %d, first form %d), ScratchSize %d" % (executed, parent, FIRST_FORM, scratch))
    for k, what in (("agpr moves", "AGPR moves"), ("LDS", "LDS instructions"), ("packed f32", "packed f32"), ("scalar f32", "scalar f32")):
        print("  %-18s %5d (parent %d)" % (what, row[k][2], prow[k][2]))
    print("  %-18s %5d (parent %d), AGPR moves in it %d (parent %d)" % ("sweep loop, a pass", row["all"][1], prow["all"][1],
                                                                       row["agpr moves"][1], prow["agpr moves"][1]))
    assert scratch == 0
    assert executed < parent
    assert executed <= FIRST_FORM
