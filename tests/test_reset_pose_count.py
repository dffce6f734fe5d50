"""The three-helper K-step kernel's main wavefront no longer draws the reset pose (ss_dynamics.hpp, reset_pose_offload(): a helper
wavefront draws it ahead of time, the main wavefront's reset copies twelve LDS words).  Counted on this tree's sources by
tools/isa_windows.py (hipcc -S of that one instantiation for gfx950; no GPU), against the parent's table in
profiles/reset_pose_isa_windows_parent.txt (the same tool on the parent's sources):

  * the substep loop is untouched: the main wavefront executes no more than the parent's 4945 instructions per substep;
  * no scratch, NumVgprs <= 256, and LDSByteSize is what it was (the pose lives in words the kernel had and did not use);
  * the control step's epilogue -- the blocks of the control-step loop behind the substep loop, a STATIC count that still holds the
    inline draw for the lanes whose counter moved in the step they reset in -- has fewer VALU instructions than the parent's 2127:
    no more than the 2044 recorded in profiles/reset_pose_isa_windows_new.txt."""
import os
import re
import subprocess
import sys

import pytest

import probe_lib

ROOT = probe_lib.ROOT
PARENT = os.path.join(ROOT, "profiles", "reset_pose_isa_windows_parent.txt")
NEW = os.path.join(ROOT, "profiles", "reset_pose_isa_windows_new.txt")
SUBSTEP = 4945


def parse(text):
    res = [re.search(r"'%s': (\d+)" % k, text) for k in ("NumVgprs", "NumAgprs", "ScratchSize", "LDSByteSize")]
    ex = re.search(r"executed per substep: (\d+);", text)
    ep = re.search(r"behind the substep loop \(the control step's epilogue, static\): (\d+) VALU, (\d+) LDS, (\d+) global memory, (\d+) in all", text)
    assert all(res) and ex and ep, text[-2000:]
    return {"vgprs": int(res[0].group(1)), "agprs": int(res[1].group(1)), "scratch": int(res[2].group(1)), "lds": int(res[3].group(1)), "substep": int(ex.group(1)),
            "epilogue_valu": int(ep.group(1)), "epilogue_all": int(ep.group(4))}


def test_reset_pose_leaves_the_main_wavefronts_epilogue():
    if not probe_lib.hipcc():
        pytest.skip("no hipcc: the kernel cannot be compiled to assembly")
    parent, recorded = parse(open(PARENT).read()), parse(open(NEW).read())
    assert parent["substep"] == SUBSTEP and parent["epilogue_valu"] == 2127, parent
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_windows.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         universal_newlines=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    new = parse(out.stdout)
    print("executed per substep: %d (parent %d); epilogue, static: %d VALU, %d in all (parent %d, %d; recorded %d, %d); "
          "VGPRs %d, AGPRs %d (parent %d), scratch %d" % (new["substep"], parent["substep"], new["epilogue_valu"], new["epilogue_all"],
                                                         parent["epilogue_valu"], parent["epilogue_all"], recorded["epilogue_valu"],
                                                         recorded["epilogue_all"], new["vgprs"], new["agprs"], parent["agprs"], new["scratch"]))
    assert new["substep"] <= SUBSTEP
    assert new["scratch"] == 0 and new["vgprs"] <= 256
    assert new["lds"] == parent["lds"] == 92160          # (40 + 50) float4 slots x 64 lanes x 16 B
    assert new["epilogue_valu"] < parent["epilogue_valu"]
    assert new["epilogue_valu"] <= recorded["epilogue_valu"] == parent["epilogue_valu"] - 83
