"""The far base of the hand-off region (ss_dynamics.hpp, Lds::hs()) on the main wavefront of the three-helper K-step kernel, counted on
this tree's sources by tools/isa_windows.py (hipcc -S of that one instantiation for gfx950; no GPU): it executes fewer instructions per
substep than the parent did (profiles/far_base_isa_windows_parent.txt, read from that file: 5179) and no more than the 5068 of the
crude first form (the base at byte 65536 itself; docs/HISTORY.md has both forms), and without scratch.  The packed and scalar f32 counts
are printed beside the parent's (address formation only: they were equal when this was written); they are not asserted, later changes
to the arithmetic are free to move them."""
import os
import re
import subprocess
import sys

import pytest

import probe_lib

ROOT = probe_lib.ROOT
PARENT = os.path.join(ROOT, "profiles", "far_base_isa_windows_parent.txt")
FIRST_FORM = 5068


def parse(text):
    scratch = re.search(r"'ScratchSize': (\d+)", text)
    ex = re.search(r"executed per substep: (\d+);", text)
    f32 = [re.search(r"^\s+%s f32\s+\d+\s+\d+\s+(\d+)\s*$" % k, text, re.M) for k in ("packed", "scalar")]
    assert scratch and ex and all(f32), text[-2000:]
    return int(scratch.group(1)), int(ex.group(1)), tuple(int(m.group(1)) for m in f32)


def test_far_base_shortens_the_main_wavefronts_stream():
    if not probe_lib.hipcc():
        pytest.skip("no hipcc: the kernel cannot be compiled to assembly")
    _, parent, parent_f32 = parse(open(PARENT).read())
    assert 5000 < parent < 5500, parent
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_windows.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         universal_newlines=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    scratch, executed, f32 = parse(out.stdout)
    print("executed per substep: %d (parent %d, first form %d), packed / scalar f32 %s (parent %s), ScratchSize %d"
          % (executed, parent, FIRST_FORM, f32, parent_f32, scratch))
    assert scratch == 0
    assert executed < parent and executed <= FIRST_FORM
