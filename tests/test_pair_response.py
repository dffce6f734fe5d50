"""joint_tau's pair overload (ss_dynamics.hpp) -- the explicit joint torque and the implicit diagonal of a {leg, arm} pair of joints on
packed instructions, as the three-helper step kernels compute them for joints (3,13) (4,14) (5,15) (6,16) -- must be joint_tau per
joint, BITWISE, for both robots.  tests/device/ss_probe.hip evaluates both sides per case, one lane per case, one launch per robot.

Inputs: the grid of tests/test_limit_forms.py (both sides of both limits, at the limits, +-0, +-inf, NaN, denormals in q and qd, about 4100
cases per joint) with power 1.0 and 0.6 and actions that take +-0, +-1, +-inf, NaN and denormals as well, drawn apart for the two halves.
Every word is compared as bits, NaN signs and payloads and the sign of a zero included: the two sides are the same expression per half,
and -fno-signed-zeros gives the compiler no occasion to treat them differently.

The contact response's down-sweep on {leg, arm} pairs, which this file was to hold against the scalar imp_down chains as well, is not
in the kernels (docs/HISTORY.md "Joint torques of the {leg, arm} pairs on packed instructions": measured slower, and a NaN left it with
the other sign than imp_down's), so there is nothing of it to test."""

import numpy as np
import pytest

import probe_lib
import test_limit_forms as lf

LEG, ARM = [3, 4, 5, 6], [13, 14, 15, 16]


def _f(bits):
    return np.array(bits, np.uint32).view(np.float32)


def same_bits(new, old):
    return new.view(np.uint32) == old.view(np.uint32)


def tau_rows(kind):
    g = lf.grid(kind)
    n = g.shape[0]
    rng = np.random.default_rng(177 + kind)
    x = np.zeros((n, 3 + 2 * lf.NJ), np.float32)
    x[:, 0] = np.where(np.arange(n) % 2 == 0, np.float32(1.0), np.float32(0.6))
    x[:, 3:] = g[:, 2:]
    sp = np.concatenate([np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, 1e-30, -1e-30], np.float32),
                         _f([0x7FC00000, 0xFFC00123, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF])])
    for col in (1, 2):
        a = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        at = rng.permutation(n)[:8 * sp.size]
        a[at] = np.tile(sp, 8)
        x[:, col] = a
    return x


def check_tau(flavour, kind):
    x = tau_rows(kind)
    assert 4000 < x.shape[0] < 5000
    out = probe_lib.run(flavour, "tau_pair", kind, x).reshape(x.shape[0], 4, 2, 4)
    new, old = out[:, :, 0], out[:, :, 1]
    same = same_bits(new, old)
    zero_sign = ~same & (new == 0) & (old == 0)
    print("%s kind %d tau: %d cases, %d words differ, of them %d in the sign of a zero alone" % (
        flavour, kind, x.shape[0], int((~same).sum()), int(zero_sign.sum())))
    if not same.all():
        i, p, c = [int(v[0]) for v in np.nonzero(~same)]
        j = (LEG, ARM)[c % 2][p]
        raise AssertionError("%s kind %d: %d words differ; first: case %d joint %d %s, q %r qd %r act %r: pair %r (%#x) scalar %r (%#x)" % (
            flavour, kind, int((~same).sum()), i, j, ("tau", "Dadd")[c // 2], x[i, 3 + 2 * j], x[i, 4 + 2 * j], x[i, 1 + c % 2],
            new[i, p, c], new[i, p, c].view(np.uint32), old[i, p, c], old[i, p, c].view(np.uint32)))
    # the limit's gains are on in some cases and off in others, for every joint of the pairs: Dadd takes two values
    assert all(np.unique(old[:, p, c][np.isfinite(old[:, p, c])]).size >= 2 for p in range(4) for c in (2, 3))


@pytest.mark.parametrize("kind", [0, 1], ids=["walker3d", "mike"])
def test_pair_tau_host(kind):
    if not probe_lib.hipcc():
        pytest.skip("no hipcc: the host build of the probe cannot be made")
    check_tau("host", kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1], ids=["walker3d", "mike"])
def test_pair_tau_device(kind):
    check_tau("device", kind)
