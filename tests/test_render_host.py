"""The render kernels' own code (steppingstone_amd/csrc/ss_render.hpp, compiled for the CPU through tests/host/render_host.cpp) against
the numpy restatement of docs/RENDER.md (tests/np_render.py) on oracle states of both robots, curricula 0 and 5, shadows on and off.
Skipped without hipcc."""
import shutil

import numpy as np
import pytest

import np_render as nr
import oracle_lib as ol

pytestmark = pytest.mark.skipif(not (shutil.which("hipcc") or shutil.which("/opt/rocm/bin/hipcc")), reason="needs hipcc")


def _states(kind, cur, n=6, steps=45, seed=21):
    o = ol.OracleEnv(kind, n, seed=seed)
    o.set_curriculum(cur)
    o.reset()
    for t in range(steps):
        o.step(o.random_actions(t))
    return o.get_state()


@pytest.mark.parametrize("kind,k", [("walker3d", 0), ("mike", 1)])
@pytest.mark.parametrize("cur", [0, 5])
def test_host_frames_match_numpy(kind, k, cur):
    import render_host_lib as rh
    st = _states(kind, cur)
    ids = [0, 3, 5]
    for shadows in (True, False):
        for cam in (dict(nr.DEFAULT_CAMERA, shadows=shadows), dict(nr.DEFAULT_CAMERA, mode=nr.CHASE, shadows=shadows)):
            rgb, depth, seg = rh.render(k, st, ids, 96, 72, cam)
            for m, e in enumerate(ids):
                ref = nr.render(kind, st[e].astype(np.float64), 96, 72, cam)
                nr.compare((rgb[m], depth[m], seg[m]), ref, "%s c%d env %d shadows %s mode %d" % (kind, cur, e, shadows, cam["mode"]))
                assert (seg[m] > 0).mean() > 0.05


def test_host_body_poses_match_model_fk():
    import render_host_lib as rh
    for kind, k in (("walker3d", 0), ("mike", 1)):
        st = _states(kind, 5, n=4, steps=30)
        got = rh.body_poses(k, st)
        for e in range(st.shape[0]):
            assert np.abs(got[e] - nr.body_poses(kind, st[e])).max() < 2e-5


def test_out_of_range_env_is_background():
    import render_host_lib as rh
    st = _states("walker3d", 0, n=2, steps=0)
    rgb, depth, seg = rh.render(0, st, [-1, 2, 1], 32, 16, nr.DEFAULT_CAMERA)
    ref = nr.render("walker3d", None, 32, 16)
    for m in (0, 1):
        assert (seg[m] == 0).all() and (depth[m] == nr.DEFAULT_CAMERA["far_m"]).all()
        assert np.abs(rgb[m].astype(int) - ref[0]).max() <= 1
    assert (seg[2] > 0).any()


def test_partial_tiles_and_odd_shapes():
    """W, H multiples of 4 but not of 16: the last tiles are partial; the cull mask must not drop what their pixels see."""
    import render_host_lib as rh
    st = _states("mike", 5, n=2)
    cam = dict(nr.DEFAULT_CAMERA, shadows=True)
    rgb, depth, seg = rh.render(1, st, [1], 52, 36, cam)
    nr.compare((rgb[0], depth[0], seg[0]), nr.render("mike", st[1].astype(np.float64), 52, 36, cam), "52x36")


@pytest.mark.parametrize("kind,k", [("walker3d", 0), ("mike", 1)])
def test_other_cameras_on_partial_tiles(kind, k):
    """tests/render_cases.py: FIXED (from the side, straight down and up: the `r` fallback), a close CHASE with a wide field of view, a far
    TRACK with a narrow one, a far plane that cuts the scene -- at sizes whose tiles are partial."""
    import render_cases as rc
    import render_host_lib as rh
    st = _states(kind, 5)
    e = 3
    cams = rc.cameras(st[e, 0:3])
    assert sum(rc.vertical(c) for _, c in cams) == 2 and {c["mode"] for _, c in cams} == {nr.TRACK, nr.CHASE, nr.FIXED}
    seen = 0
    for W, H in rc.HOST_SIZES:
        for name, cam in cams:
            rgb, depth, seg = rh.render(k, st, [e], W, H, cam)
            ref = nr.render(kind, st[e].astype(np.float64), W, H, cam)
            nr.compare((rgb[0], depth[0], seg[0]), ref, "%s %dx%d %s" % (kind, W, H, name))
            if (W, H) == (52, 36):
                assert (ref[2] > 0).mean() > 0.02, "%s: the camera sees nothing" % name
                cut = name == "default, far 2.6 m"
                full = nr.render(kind, st[e].astype(np.float64), W, H, dict(cam, far_m=20.0))[2] if cut else None
                assert not cut or ((full > 0) & (ref[2] == 0)).any(), "the far plane cuts nothing"
                seen += 1
    assert seen == len(cams)
