"""The half-broadcast packed multiply-add / multiply of ss_pair.hpp (pk_fma_half, pk_mul_half: the factor is the low or the HIGH
half of a pair, picked by the instruction itself) must be two scalar fmaf / two products of the same operands, bitwise, for both
halves -- on the device (inline assembly for the high half) and in the host build of the same header (plain fmaf).

16384 cases = one launch of 256 wavefronts' 64 lanes, through tests/device/ss_probe.hip, which evaluates each form and, beside it,
the scalar reference with every operand made opaque.  The operands are drawn from: +-0, the smallest and the largest denormal of
either sign, +-inf, quiet and signalling NaN payloads, +-1, 1 + 2^-23, the largest and the smallest normal, triples whose product
rounds differently fused and unfused, and random values over 60 binades.  Every case is also evaluated with ONE register as pair and
as factor (the probe's (a, a) columns).  Outputs whose two FACTORS are both NaN are held to "NaN on both sides" (see check); every other output to its bits.  A second, independent reference: exact rational arithmetic rounded once to float32, for
the first 2048 cases with finite operands."""
from fractions import Fraction

import numpy as np
import pytest

import probe_lib

N = 64 * 256
NAMES = ["fma<0>(a,s,c)", "fma<1>(a,s,c)", "fma<0>(a,a,c)", "fma<1>(a,a,c)", "mul<0>(a,s)", "mul<1>(a,s)", "mul<0>(a,a)", "mul<1>(a,a)"]


def _f(bits):
    return np.array(bits, np.uint32).view(np.float32)


def cases():
    rng = np.random.default_rng(20240611)
    special = np.concatenate([
        _f([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x7F800000, 0xFF800000,
            0x7FC00001, 0xFFC12345, 0x7F800001, 0xFFA00000, 0x00800000, 0x80800000, 0x7F7FFFFF, 0xFF7FFFFF]),
        np.array([1.0, -1.0, 1.0 + 2.0 ** -23, 1.0 + 2.0 ** -12, -(1.0 + 2.0 ** -11), 3.0, 1.0 / 3.0, -0.1], np.float32)])
    x = (rng.standard_normal((N, 6)) * np.exp2(rng.integers(-30, 30, (N, 6)))).astype(np.float32)
    pick = rng.random((N, 6)) < 0.35
    x[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    # products that round differently fused and unfused: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24, and the unfused product drops the 2^-24
    e = np.float32(1.0 + 2.0 ** -12)
    m = np.float32(-(1.0 + 2.0 ** -11))
    x[0] = [e, e, e, e, m, m]
    x[1] = [e, 3.0, 7.0, e, m, -3.0]
    x[2] = [np.float32(1.0 / 3.0), np.float32(3.0), np.float32(3.0), np.float32(1.0 / 3.0), -1.0, -1.0]
    x[3:3 + len(special), :] = special[:, None]            # every special in all six places at once
    return x


def round_f32(v):
    """a rational -> the nearest float32, ties to even (one rounding)"""
    if v == 0:
        return np.float32(0.0)
    s, a = (-1.0 if v < 0 else 1.0), abs(v)
    e = a.numerator.bit_length() - a.denominator.bit_length() - 24
    while a >= Fraction(2) ** (e + 24):
        e += 1
    while a < Fraction(2) ** (e + 23):
        e -= 1
    e = max(e, -149)
    q = a / Fraction(2) ** e
    m = q.numerator // q.denominator
    r = q - m
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and (m & 1)):
        m += 1
    with np.errstate(over="ignore"):
        return np.float32(s * np.ldexp(np.float64(m), e))       # m < 2^25: exact in float64; above the range: inf


def exact_reference(x):
    """[n, 16]: the eight outputs by rational arithmetic; rows with a non-finite operand are left out by the caller"""
    out = np.zeros((x.shape[0], 16), np.float32)
    for i, row in enumerate(x):
        a, s, c = [Fraction(float(v)) for v in row[0:2]], [Fraction(float(v)) for v in row[2:4]], [Fraction(float(v)) for v in row[4:6]]
        k = 0
        for fac in (s[0], s[1], a[0], a[1]):
            out[i, k], out[i, k + 1] = round_f32(a[0] * fac + c[0]), round_f32(a[1] * fac + c[1])
            k += 2
        for fac in (s[0], s[1], a[0], a[1]):
            out[i, k], out[i, k + 1] = round_f32(a[0] * fac), round_f32(a[1] * fac)
            k += 2
    return out


def check(flavour):
    x = cases()
    out = probe_lib.run(flavour, "pk_half", 0, x)
    got, ref = out[:, :16].view(np.uint32), out[:, 16:].view(np.uint32)
    # Bits, NaN payloads included -- with ONE exception: where BOTH factors of an output's product are NaN (the half of a and the
    # broadcast factor), which payload comes out depends on which of the two the instruction takes as its first operand, and a
    # product commutes: neither C nor the compiler fixes that order for the scalar reference (a * f may be emitted as f * a).  Only
    # those outputs are held to "NaN on both sides"; a NaN addend, or one NaN factor, leaves nothing to commute.
    nan = np.isnan(x)
    factor = [nan[:, 2], nan[:, 3], nan[:, 0], nan[:, 1]] * 2          # s.x, s.y, a.x, a.y: fma outputs, then mul outputs
    for k, name in enumerate(NAMES):
        g, r = got[:, 2 * k:2 * k + 2], ref[:, 2 * k:2 * k + 2]
        both = nan[:, 0:2] & factor[k][:, None]                        # per half of a: it and the factor are NaN
        ok = (g == r) | (both & np.isnan(g.view(np.float32)) & np.isnan(r.view(np.float32)))
        bad = np.nonzero(~ok.all(axis=1))[0]
        assert bad.size == 0, "%s (%s): %d of %d cases differ from the scalar form, first: in %s got %s want %s" % (
            name, flavour, bad.size, N, x[bad[0]].view(np.uint32), got[bad[0], 2 * k:2 * k + 2], ref[bad[0], 2 * k:2 * k + 2])
    # the fused product keeps the 2^-24 an unfused one would drop
    assert out[0, 0] == np.float32(2.0 ** -24) and out[0, 2] == np.float32(2.0 ** -24), out[0, :4]
    fin = np.nonzero(np.isfinite(x[:2048]).all(axis=1))[0]
    assert fin.size > 100
    want = exact_reference(x[fin])
    g = out[fin, :16]
    same = (g.view(np.uint32) == want.view(np.uint32)) | ((g == 0) & (want == 0))     # the build does not tell +0 from -0
    assert same.all(), "%s: %d outputs differ from the exactly rounded value, first case %s" % (
        flavour, int((~same).sum()), x[fin[np.nonzero(~same.all(axis=1))[0][0]]])
    return out


def test_host_fallback_is_two_fmaf():
    if not probe_lib.hipcc():
        pytest.skip("no hipcc: the host build of the probe cannot be made")
    check("host")


@pytest.mark.gpu
def test_device_broadcast_is_two_fmaf():
    dev = check("device")
    host = check("host")
    num = ~np.isnan(host)
    assert (np.isnan(dev) == np.isnan(host)).all()
    d, h = dev[num], host[num]
    assert ((d.view(np.uint32) == h.view(np.uint32)) | ((d == 0) & (h == 0))).all(), "device and host builds disagree"
