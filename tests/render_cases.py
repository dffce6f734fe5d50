"""The cameras tests/test_render_host.py and tests/test_gpu_render.py draw besides the default one, as np_render camera dicts, and the frame
sizes whose last tiles are partial.  TEST INFRASTRUCTURE ONLY; no test in it.

cameras(pos): offsets are taken from `pos`, the torso position of the env that is drawn (state words 0:3).  Every number is rounded to
float32 first, so the kernel (an ss_camera of floats) and the numpy restatement see the same camera; the vertical FIXED cameras have the
eye exactly above / below the target and so take the `r` fallback of docs/RENDER.md 1 in both."""
import numpy as np

import np_render as nr

# (W, H): multiples of 4, not of the 16 x 16 tile, in one direction or both; a single partial tile; more than eight tiles across
SIZES = [(52, 36), (36, 52), (20, 4), (4, 20), (4, 4), (132, 68)]
HOST_SIZES = [(52, 36), (20, 4)]


def _f32(v):
    return tuple(float(x) for x in np.asarray(v, np.float32))


def cameras(pos):
    """[(name, np_render camera dict)]"""
    p = np.asarray(pos, np.float32).astype(np.float64)
    at = lambda *o: _f32(p + np.array(o))
    cams = [
        ("fixed, from the side", dict(mode=nr.FIXED, eye=at(0.3, -3.0, 0.2), target=at(0.3, 0.0, -0.3))),
        ("fixed, straight down", dict(mode=nr.FIXED, eye=at(0.0, 0.0, 3.0), target=at(0.0, 0.0, -1.0))),
        ("fixed, straight up", dict(mode=nr.FIXED, eye=at(0.0, 0.0, -2.5), target=at(0.0, 0.0, 0.0))),
        ("chase, close, fov 120", dict(mode=nr.CHASE, eye=_f32((-0.8, -0.35, 0.3)), target=_f32((0.5, 0.0, -0.1)), fov_y_deg=120.0)),
        ("track, 6 m, fov 8", dict(mode=nr.TRACK, eye=_f32((-2.0, -5.5, 1.4)), target=_f32((0.2, 0.0, -0.3)), fov_y_deg=8.0)),
        ("default, far 2.6 m", dict(far_m=float(np.float32(2.6)))),
        ("default", dict()),
        ("default chase", dict(mode=nr.CHASE)),
    ]
    out = []
    for name, c in cams:
        d = dict(nr.DEFAULT_CAMERA, **c)
        d["eye"], d["target"] = _f32(d["eye"]), _f32(d["target"])
        out.append((name, d))
    return out


def vertical(cam):
    """True for a FIXED camera looking straight up or down"""
    return cam["mode"] == nr.FIXED and cam["eye"][0] == cam["target"][0] and cam["eye"][1] == cam["target"][1]
