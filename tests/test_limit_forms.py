"""The joint-limit forms of ss_dynamics.hpp -- viol = min(q - lo, 0) + max(q - hi, 0) and the limit gains as K's bits under an
all-or-nothing mask (joint_limit) -- and the joint torque / implicit diagonal built on them (joint_tau) must be the forms they
replaced, BITWISE, for every joint of both robots.  The replaced forms are kept verbatim in tests/device/ss_probe.hip, which
evaluates both sides per case, one lane per case.

Grid per joint, q: both bounds, nextafter on either side of each, the bounds +- the smallest and the largest denormal, far outside
(+-1e3, +-3e38, +-inf), +-0, +-denormals, NaN, and 4096 random values across and around the range; qd: 0, +-denormals, +-tiny,
+-huge, +-inf, NaN and random values, paired with the q column in a fixed shuffle.  The zero's sign is not compared where both
sides are zero (the build is -fno-signed-zeros on both sides; every other word is compared as bits, NaN payloads included)."""
import os
import re

import numpy as np
import pytest

import probe_lib

NJ = 21
COLS = ["viol", "kl", "dl", "tau", "Dadd"]
N_RANDOM = 4096


def bounds():
    """(lo, hi)[kind][21] as ss_model_tables.hpp states them"""
    text = open(os.path.join(probe_lib.ROOT, "steppingstone_amd", "csrc", "ss_model_tables.hpp")).read()
    out = []
    for name in ("lo", "hi"):
        rows = re.findall(r"static constexpr float %s\[21\] = \{([^}]*)\}" % name, text)
        assert len(rows) == 2, name
        out.append([np.array([np.float32(v.strip().rstrip("f")) for v in r.split(",")], np.float32) for r in rows])
    return [(out[0][k], out[1][k]) for k in range(2)]


def _f(bits):
    return np.array(bits, np.uint32).view(np.float32)


def grid(kind):
    lo, hi = bounds()[kind]
    rng = np.random.default_rng(77 + kind)
    dmin, dmax = _f([0x00000001])[0], _f([0x007FFFFF])[0]
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    qs, qds = [], []
    for j in range(NJ):
        l, h = lo[j], hi[j]
        assert l < h
        pts = [l, h, np.nextafter(l, -inf), np.nextafter(l, inf), np.nextafter(h, -inf), np.nextafter(h, inf),
               l + dmin, l - dmin, l + dmax, l - dmax, h + dmin, h - dmin, h + dmax, h - dmax,
               np.float32(1e3), np.float32(-1e3), np.float32(3e38), np.float32(-3e38), inf, -inf,
               np.float32(0.0), np.float32(-0.0), dmin, -dmin, dmax, -dmax, nan, _f([0xFFC00123])[0]]
        span = h - l
        r = np.concatenate([rng.uniform(l - span, h + span, N_RANDOM // 2),
                            l + rng.standard_normal(N_RANDOM // 4) * 1e-5, h + rng.standard_normal(N_RANDOM // 4) * 1e-5])
        q = np.concatenate([np.array(pts, np.float32), r.astype(np.float32)])
        sp = np.array([0.0, -0.0, dmin, -dmin, dmax, -dmax, 1e-30, -1e-30, 3e38, -3e38, inf, -inf, nan, 1.0, -1.0, 240.0], np.float32)
        qd = (rng.standard_normal(q.size) * np.exp2(rng.integers(-20, 12, q.size))).astype(np.float32)
        at = rng.permutation(q.size)[:4 * sp.size]
        qd[at] = np.tile(sp, 4)
        qs.append(q)
        qds.append(qd)
    n = qs[0].size
    x = np.zeros((n, 2 + 2 * NJ), np.float32)
    x[:, 0] = rng.uniform(0.2, 1.2, n)                    # power
    x[:, 1] = rng.uniform(-1.0, 1.0, n)                   # action
    for j in range(NJ):
        x[:, 2 + 2 * j], x[:, 3 + 2 * j] = qs[j], qds[j]
    return x


def check(flavour, kind):
    x = grid(kind)
    assert 4000 < x.shape[0] < 5000
    out = probe_lib.run(flavour, "limit_forms", kind, x).reshape(x.shape[0], NJ, 2, 5)
    new, old = out[:, :, 0, :], out[:, :, 1, :]
    same = (new.view(np.uint32) == old.view(np.uint32)) | ((new == 0) & (old == 0))
    if not same.all():
        i, j, c = [int(v[0]) for v in np.nonzero(~same)]
        raise AssertionError("%s kind %d: %d words differ; first: joint %d %s, q %r qd %r: new %r (%#x) old %r (%#x)" % (
            flavour, kind, int((~same).sum()), j, COLS[c], x[i, 2 + 2 * j], x[i, 3 + 2 * j], new[i, j, c],
            new[i, j, c].view(np.uint32), old[i, j, c], old[i, j, c].view(np.uint32)))
    # the grid does reach both sides of the limit on every joint
    assert (old[:, :, 0] > 0).any(axis=0).all() and (old[:, :, 0] < 0).any(axis=0).all() and (old[:, :, 0] == 0).any(axis=0).all()
    return out


@pytest.mark.parametrize("kind", [0, 1], ids=["walker3d", "mike"])
def test_limit_forms_host(kind):
    if not probe_lib.hipcc():
        pytest.skip("no hipcc: the host build of the probe cannot be made")
    check("host", kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1], ids=["walker3d", "mike"])
def test_limit_forms_device(kind):
    check("device", kind)
