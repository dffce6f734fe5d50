"""The step kernels' spatial algebra, operator by operator, against the fp64 reference of tests/np_spatial.py.

tests/device/ss_probe.hip calls every operator of ss_math.hpp / ss_pair.hpp and the per-joint helpers of ss_dynamics.hpp on one case
per lane.  Two flavours of the same test bodies:
    host    the probe compiled for the CPU at test time (tests/probe_lib.py; skipped without hipcc),
    device  steppingstone_amd/lib/libss_probe.so, built for gfx950 with the product's flags (@pytest.mark.gpu); this flavour adds the
            lane exchange, which has no host form, and prints (information only) how far device and host results differ.
A component passes when |got - ref| <= k * 2^-24 * B, B the reference's running error bound (np_spatial's docstring), and must be
exactly 0 where B is 0.  k per op: np_spatial.OPS; it bounds the fp32 roundings on the longest path of the source, table constants
counting one each.  Every component of every case is judged; the worst err / (2^-24 B) of each op is printed (pytest -s) and kept in
docs/HISTORY.md."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import np_spatial as ns
import probe_lib as pl

HAVE_HIPCC = bool(pl.hipcc())
FLAVOURS = [pytest.param("host", marks=pytest.mark.skipif(not HAVE_HIPCC, reason="needs hipcc")),
            pytest.param("device", marks=pytest.mark.gpu)]


def _ulps_apart(a, b):
    """largest distance between two float32 arrays in units in the last place (ordered-integer distance)"""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.abs(key(a) - key(b)).max())


def _device_vs_host(op, kind, inp, dev, B=None):
    """information only: how far the two builds of the same source are apart.  The distance in ulps is large wherever a component
    cancels towards 0, so it is also given in the unit the bound is stated in."""
    if not pl.host_ready():      # only where the host flavour has been built already: a GPU test compiles nothing
        return
    host = pl.run("host", op, kind, inp)
    if host is None:
        return
    rel = ""
    if B is not None and (B > 0).any():
        d = np.abs(dev.astype(np.float64) - host.astype(np.float64))
        rel = ", %.2f x 2^-24 B" % (d[B > 0] / (ns.U * B[B > 0])).max()
    print("spatial-op device-vs-host %s %s: %d ulp%s" % (op, ns.KINDS[kind], _ulps_apart(dev, host), rel))


@pytest.mark.parametrize("kind", ns.KINDS)
@pytest.mark.parametrize("op", list(ns.OPS))
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_operator_within_its_rounding_bound(flavour, op, kind):
    inp, ref, B, exact = ns.prepared(op, kind)
    got = pl.run(flavour, op, ns.KINDS.index(kind), inp)
    assert got.shape == ref.shape
    worst, fails = ns.judge(got, ref, B, exact, ns.OPS[op].k)
    print("spatial-op %s %s %s: n=%d worst err/(2^-24 B) = %.2f (k = %d)" % (flavour, op, kind, inp.shape[0], worst, ns.OPS[op].k))
    if flavour == "device":
        _device_vs_host(op, ns.KINDS.index(kind), inp, got, B)
    assert not fails, "%s %s: %d components outside k = %d; (case, component, got, ref, ratio): %s; inputs of the first: %s" % (
        op, kind, len(fails), ns.OPS[op].k, fails[:6], inp[fails[0][0]].tolist())


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_sincos_absolute_error(flavour):
    """ss_sincos against fp64 sin / cos to an absolute 4 * 2^-24: every 7th float in |x| <= 3.2, every 97th in |x| <= 1000 and the
    multiples of pi/2 with their fp32 neighbours (host); on the device a 2^20-point, evenly strided subset of that grid plus the same
    multiples."""
    special = ns.sincos_special()
    if flavour == "host":
        step = 1 << 23
        chunks = [special] + [(lo, min(lo + step, ns.SINCOS_GRID)) for lo in range(0, ns.SINCOS_GRID, step)]
        workers = 4            # numpy's sin / cos and the probe call release the interpreter lock
    else:
        sub = ns.sincos_points((np.arange(1 << 20, dtype=np.int64) * ns.SINCOS_GRID) >> 20)
        chunks = [np.concatenate([special, sub])]
        assert chunks[0].size % 64 != 0
        workers = 1

    def one(chunk):
        x = ns.sincos_points(np.arange(chunk[0], chunk[1], dtype=np.int64)) if isinstance(chunk, tuple) else chunk
        return ns.sincos_worst(x, pl.run(flavour, "sincos", 0, x.reshape(-1, 1))) + (x.size,)
    pl.load(flavour)
    with ThreadPoolExecutor(workers) as pool:
        results = list(pool.map(one, chunks))
    worst, at, _ = max(results)
    npts = sum(r[2] for r in results)
    print("spatial-op %s sincos: %d arguments, worst |err| = %.3f x 2^-24 at x = %r" % (flavour, npts, worst, at))
    assert worst <= ns.SINCOS_K, "ss_sincos off by %.3f x 2^-24 at x = %r" % (worst, at)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_chol6_factor_and_solve(flavour):
    """|L L^T - M| <= 14 * 2^-24 |L||L^T| and |b + L L^T x| <= 26 * 2^-24 |L||L^T||x| (twice the textbook gamma_7 and gamma_13: the
    diagonal is a reciprocal square root), float and ssf2 solves, each half of the pair solve against the scalar solve of its
    right-hand side; random SPD matrices and both robots' base inertia at q0."""
    inp = ns.chol_cases()
    out = pl.run(flavour, "chol", 0, inp)
    wf, ws, wp, fails = ns.chol_judge(inp, out)
    print("spatial-op %s chol: n=%d worst factor %.2f (k = %d), solve %.2f (k = %d), pair-vs-scalar %.2f" % (
        flavour, inp.shape[0], wf, ns.CHOL_K_FACTOR, ws, ns.CHOL_K_SOLVE, wp))
    if flavour == "device":
        _device_vs_host("chol", 0, inp, out)
    assert not fails, fails[:8]


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_philox_known_answers_and_u01(flavour):
    inp = ns.philox_cases()
    out = pl.run(flavour, "philox", 0, inp.view(np.float32))
    words = out[:, :4].copy().view(np.uint32)
    for e, (_, _, want) in enumerate(ns.PHILOX_KAT):
        assert tuple(int(w) for w in words[e]) == want, "Random123 known answer %d: got %s" % (e, [hex(int(w)) for w in words[e]])
    assert (words == ns.philox_np(inp[:, :4], inp[:, 4:6])).all()
    u = out[:, 4]
    want = ((inp[:, 6] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    assert (u == want).all() and (u >= 0).all() and (u < 1).all()
    assert u[0] == 0.0 and u[1] == np.float32(1.0 - 2.0 ** -24)          # u01(0), u01(0xFFFFFFFF)


@pytest.mark.skipif(not HAVE_HIPCC, reason="needs hipcc")
def test_lane_exchange_is_refused_on_the_host():
    assert pl.run("host", "xchg", 0, ns.xchg_cases()) is None


@pytest.mark.gpu
def test_lane_exchange():
    """xchg / xchg_u32 / xchg_i hand lane l the bits of lane l ^ 1; xchg_sv and xchg_abi hand it Mir a and Mir I Mir,
    Mir = diag(-1, 1, -1, 1, -1, 1): sign flips only, so equality is exact."""
    inp = ns.xchg_cases()
    out = pl.run("device", "xchg", 0, inp)
    words, sv, abi = ns.xchg_expected(inp)
    got_words = out[:, :3].copy().view(np.uint32)
    for c, name in enumerate(("xchg", "xchg_u32", "xchg_i")):
        bad = np.nonzero(got_words[:, c] != words[:, c])[0]
        assert bad.size == 0, "%s: lane %d holds %#x, its partner sent %#x" % (name, bad[0], got_words[bad[0], c], words[bad[0], c])
    assert (inp.view(np.uint32)[:, 1] == 0xFFFFFFFF).any() and (inp.view(np.int32)[:, 2] < 0).any()
    assert (out[:, 3:9] == sv).all(), "xchg_sv"
    assert (out[:, 9:30] == abi).all(), "xchg_abi"
