"""The policy MLP of the closed-loop look-ahead and its packed weights on their own (steppingstone_amd/csrc/ss_policy.hpp; docs/PHYSICS.md
14), layer by layer, against the numpy reference of tests/np_policy.py.

tests/device/ss_probe.hip's second entry, ssp_mlp, runs ONE MLP phase on rows it is given and dumps both activation blocks whole.  Two
flavours of the same test bodies, as in tests/test_spatial_ops.py:
    host    eval_row (the plain loops the CPU build of the look-ahead runs) on the packed words, compiled here at test time,
    device  mlp_phase, the matrix-instruction kernel, in a workgroup shaped as lookahead_policy_kernel's (@pytest.mark.gpu).
The nets: the three of the look-ahead tests and policy_nets.SHAPES (width 1, the tile edge, 2 / 7 / 8 layers, tile counts 3 / 5 / 7,
an odd number of prefetch groups, a wide layer behind a narrow one).  The rows: np_policy.rows().  The blocks are filled with a NaN
pattern before the phase, so a layer that reads a word its predecessor did not write shows as a NaN.
  1  every word of the dump: a real output within its OWN fp64 bound (np_policy's docstring), a padded column +-0, a word the net never
     writes still the prefill; and the last layer once more from the dumped layer before it, within one layer's bound
  2  the documented sum: for the identity / relu nets the bits are the exact f32 fma chain's (from the bias, k ascending); and a
     zero-bias net on denormal inputs and on products that underflow, where the compared words are themselves denormal, so that a matrix
     instruction that flushed denormal operands or results would differ
  3  a row's bits are its own: not n's, not its position's, not its neighbours' (NaN and huge rows among them)
  4  non-finite values: a NaN weight behind relu reaches every action; an infinite hidden activation, pinned to what the code does
  5  tanhf of the flavour against fp64, in ulps, over a dense sweep: the figure np_policy.TANH_ULPS rests on
  6  the packed form, word by word: ss_policy_pack on the device and the host build's lhp_policy_pack against np_policy.pack
  7  np_policy.fmaf against the C library's fmaf on 1.4 million triples (CPU)
The worst err / bound per net is printed (pytest -s) and kept in docs/HISTORY.md."""
import ctypes as C
import functools

import numpy as np
import pytest

import np_policy as npp
import policy_nets as pn
import probe_lib as pl

HAVE_HIPCC = bool(pl.hipcc())
FLAVOURS = [pytest.param("host", marks=pytest.mark.skipif(not HAVE_HIPCC, reason="needs hipcc")),
            pytest.param("device", marks=pytest.mark.gpu)]
KIND = "walker3d"                        # whose shipped actor; the other nets are the same for both robots
NETS = pn.NAMES + pn.SHAPE_NAMES
CHAIN_NETS = tuple(n for n in NETS if npp.is_chain_net(pn.net(KIND, n)))
ROWSETS = ("n1", "n32", "n33", "n70")
PREFILL = pl.PREFILL


def run(flavour, layers, x):
    return pl.mlp(flavour, npp.widths_of(layers), [pn.CODE[a] for _, _, a in layers], npp.pack(layers)[0], x, PREFILL)


@functools.lru_cache(maxsize=None)
def dump(flavour, name, rows_name):
    d = run(flavour, pn.net(KIND, name), npp.rows()[rows_name])
    d.setflags(write=False)
    return d


def test_the_nets_reach_what_they_are_for():
    assert {"w1", "deep8", "wide8", "t753", "linear"} <= set(CHAIN_NETS)
    hidden, last = set(), set()
    for name in pn.SHAPE_NAMES:
        acts = [a for _, _, a in pn.net(KIND, name)]
        hidden |= set(acts[:-1])
        last.add(acts[-1])
        assert npp.widths_of(pn.net(KIND, name)) == list(pn.SHAPES[name][0])
    assert hidden == last == set(pn.CODE)
    lay = npp.layout(pn.SHAPES["t753"][0])
    assert [n // 32 for n in lay["np"]] == [7, 5, 3, 1] and (lay["kp"][2] // 32) % 2 == 1
    assert npp.layout(pn.SHAPES["w1"][0])["kp"][1] == 32 and npp.layout(pn.SHAPES["t854"][0])["kp"] == [64, 256, 160, 128]


@pytest.mark.parametrize("name", NETS)
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_every_word_within_its_own_bound(flavour, name):
    for rows_name in ROWSETS:
        d = dump(flavour, name, rows_name)
        worst, fails = npp.judge(d, npp.reference(KIND, name, rows_name, flavour), PREFILL)
        local, lfails = npp.judge_last_layer(pn.net(KIND, name), d, npp.rows()[rows_name], npp.TANH_ULPS[flavour])
        print("policy-op %s %s %s: worst err / bound of the last two layers = %.3f, of the last layer from the dumped one before it = %.3f" % (
            flavour, name, rows_name, worst, local))
        assert not fails, "%s %s: %d words; (what, row, block, column, got, want, bound): %s" % (name, rows_name, len(fails), fails[:6])
        assert not lfails, "%s %s: the last layer, %d words; (row, column, got, want, bound): %s" % (name, rows_name, len(lfails), lfails[:6])


def chain_mismatches(flavour, name, rows_name):
    """bool [n]: the row differs from the exact chain in the last layer or in the one before it"""
    layers = pn.net(KIND, name)
    outs = npp.chain_reference(KIND, name, rows_name)
    last, prev = npp.layer_views(layers, dump(flavour, name, rows_name), outs[-1].shape[0])
    bad = ~npp.same_bits(last, outs[-1]).all(1)
    if prev is not None:
        bad |= ~npp.same_bits(prev, outs[-2]).all(1)
    return bad


@pytest.mark.parametrize("name", CHAIN_NETS)
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_bits_are_the_documented_chain(flavour, name):
    for rows_name in ROWSETS:
        bad = chain_mismatches(flavour, name, rows_name)
        print("policy-op %s %s %s: %d of %d rows differ from the exact chain: %s" % (flavour, name, rows_name, bad.sum(), bad.size,
                                                                                  np.nonzero(bad)[0][:12].tolist()))
        assert not bad.any(), "%s %s: rows %s are not the f32 fma chain from the bias in index order" % (name, rows_name,
                                                                                                       np.nonzero(bad)[0][:12].tolist())


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_denormals_survive_the_chain(flavour):
    """The nets above start every chain from a bias near 0.1, which swallows a denormal term whether or not it was flushed.  Here the
    biases are zero: on denormal inputs (times weights of order 0.1 / sqrt(K)) and on normal inputs whose products underflow (weights scaled
    by 2^-100, inputs by 2^-35) the partial sums and the outputs of both layers are denormal or zero, and the bits must still be the
    chain's."""
    g = np.random.default_rng(31)
    mk = lambda n, k, scale: ((g.standard_normal((n, k)) / np.sqrt(k)) * scale).astype(np.float32)
    zero = lambda n: np.zeros(n, np.float32)
    x = npp.rows()["n70"]
    den = x[list(npp.DENORMAL_ROWS)].copy()
    den[1, np.abs(den[1]) >= 2.0 ** -126] = 0                      # row 57 without its normal entries
    cases = [("denormal inputs", [(mk(33, 60, 0.1), zero(33), "identity"), (mk(21, 33, 1), zero(21), "relu")], den),
             ("underflowing products", [(mk(33, 60, 2.0 ** -100), zero(33), "identity"), (mk(21, 33, 1), zero(21), "relu")],
              x[:33] * np.float32(2.0 ** -35))]
    for what, layers, rows in cases:
        outs = npp.chain(layers, rows)
        last, prev = npp.layer_views(layers, run(flavour, layers, rows), rows.shape[0])
        for got, want in ((prev, outs[0]), (last, outs[1])):
            tiny = (want != 0) & (np.abs(want) < 2.0 ** -126)
            assert tiny.mean() > 0.3 and (np.abs(want) < 2.0 ** -120).all(), "%s: the case misses the denormals" % what
            assert npp.same_bits(got, want).all(), "%s: %d of %d words differ from the exact chain (%d of them flushed to zero)" % (
                what, (~npp.same_bits(got, want)).sum(), want.size, ((got == 0) & (want != 0)).sum())


@pytest.mark.parametrize("name", NETS)
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_a_rows_bits_are_its_own(flavour, name):
    layers, x = pn.net(KIND, name), npp.rows()["n70"]
    base = dump(flavour, name, "n70")
    g = np.random.default_rng(17)
    # another order, with rows of NaN, of infinities and of 1e30 between the kept ones
    perm = g.permutation(70)
    y = x[perm].copy()
    junk = np.arange(70) % 5 == 2
    y[junk] = np.array([np.nan, np.inf, 1e30, -np.inf, -1e30], np.float32)[np.arange(junk.sum()) % 5, None]
    got = run(flavour, layers, y)
    keep = np.nonzero(~junk)[0]
    assert (got[keep] == base[perm[keep]]).all(), "%s: a row's bits changed with its position or its neighbours" % name
    # fewer rows: 33 (a second group of one row), 1 (the other 31 rows of the group are the NaN prefill)
    rev = np.arange(69, 36, -1)
    assert (run(flavour, layers, x[rev])[:33] == base[rev]).all(), "%s: n = 33" % name
    for r in (0, 57, 69):
        assert (run(flavour, layers, x[r:r + 1])[0] == base[r]).all(), "%s: row %d alone" % (name, r)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_a_nan_weight_behind_relu_reaches_every_action(flavour):
    layers = [(w.copy(), b, a) for w, b, a in pn.net(KIND, "ragged")]
    assert layers[1][2] == "relu"
    layers[1][0][5, 3] = np.nan
    x = npp.rows()["n33"]
    last, prev = npp.layer_views(layers, run(flavour, layers, x), 33)
    assert np.isnan(prev[:, 5]).all() and np.isfinite(np.delete(prev, 5, 1)).all(), "relu must leave a NaN a NaN"
    assert np.isnan(last).all()


def inf_net(widths, acts, signed_last=False):
    """hidden unit 3 of the first layer is 3e38 x[0]; every later weight is positive (signed_last: but the last layer's), so that an
    infinity meets no infinity of the other sign"""
    g = np.random.default_rng(5)
    out = []
    for i, a in enumerate(acts):
        w = (g.standard_normal((widths[i + 1], widths[i])) / np.sqrt(widths[i])).astype(np.float32)
        if i > 0 and not (signed_last and i == len(acts) - 1):
            w = np.abs(w) + np.float32(0.01)
        out.append((w, (g.standard_normal(widths[i + 1]) * 0.1).astype(np.float32), a))
    out[0][0][3, :] = 0
    out[0][0][3, 0] = 3e38
    return out


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_an_infinite_hidden_activation(flavour):
    """What the code does (docs/PHYSICS.md 14 states it next to f): the infinity of hidden layer l meets the ZERO weights of layer
    l + 1's padded columns, inf * 0 = NaN stands in those columns, and layer l + 2 -- which multiplies them by zero weights again --
    turns every output of the row into NaN.  So: behind a layer l + 1 whose width is a multiple of 32 (no padded column), or with layer
    l + 1 the last one (its padded columns are never read), the actions are those of the unpadded network, tanh(+-inf) = +-1; otherwise
    every action of the row is NaN.  Rows without an infinity are untouched either way."""
    x = npp.rows()["n70"][:8].copy()
    x[:, 0] = np.array([10, 0, -10, 0, 10, 0, -10, 0], np.float32)
    hot, up = x[:, 0] != 0, x[:, 0] > 0
    for mid, nan_actions in ((64, False), (50, True)):
        layers = inf_net((60, 37, mid, 21), ("identity", "identity", "tanh"))
        d = run(flavour, layers, x)
        last, prev = npp.layer_views(layers, d, 8)
        assert np.isinf(prev[hot]).all() and (np.sign(prev[hot]) == np.where(up[hot], 1, -1)[:, None]).all()
        assert np.isfinite(prev[~hot]).all() and np.isfinite(last[~hot]).all()
        pad = d.view(np.float32)[:8, 1, mid:(mid + 31) // 32 * 32]
        if nan_actions:
            assert np.isnan(pad[hot]).all() and (pad[~hot] == 0).all(), "the padded columns of the layer behind the infinity"
            assert np.isnan(last[hot]).all(), "every action of a row with an infinite activation two layers up"
        else:
            assert pad.size == 0 and (last[hot] == np.where(up[hot], 1, -1)[:, None]).all(), "tanh(+-inf) = +-1"
        # the network as PHYSICS 14 defines it (unpadded, float32): +-1 at both widths
        h = x
        for w, b, a in layers:
            with np.errstate(all="ignore"):
                h = (h.astype(np.float32) @ w.T + b).astype(np.float32)
        with np.errstate(all="ignore"):
            assert (np.tanh(h[hot]) == np.where(up[hot], 1, -1)[:, None]).all()
    # the infinity in the LAST hidden layer: the action tile's own padded columns hold the NaN, no action does
    layers = inf_net((60, 37, 21), ("identity", "tanh"), signed_last=True)
    d = run(flavour, layers, x)
    last, _ = npp.layer_views(layers, d, 8)
    want = np.sign(layers[1][0][:, 3])[None, :] * np.where(up[hot], 1, -1)[:, None]
    assert (last[hot] == want).all() and np.isfinite(last[~hot]).all()
    tile_pad = d.view(np.float32)[:8, 1, 21:32]
    assert np.isnan(tile_pad[hot]).all() and (tile_pad[~hot] == 0).all()


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_tanhf_in_ulps(flavour):
    layers, x = npp.tanh_net(), npp.tanh_sweep()
    got = run(flavour, layers, x)[:x.shape[0], 0, :21].view(np.float32)
    arg = x[:, :21]
    off = npp.ulps_off(got, np.tanh(arg.astype(np.float64)))
    at = np.unravel_index(off.argmax(), off.shape)
    print("policy-op %s tanhf: %d arguments, worst %.3f ulp at x = %r" % (flavour, arg.size, off.max(), float(arg[at])))
    assert np.isfinite(got).all() and (np.abs(got) <= 1).all() and (got == arg).mean() < 0.25 and off.max() > 0
    assert np.ceil(off.max()) + 1 <= npp.TANH_ULPS[flavour], "np_policy.TANH_ULPS[%r] is below the measured %.3f ulp, rounded up, plus one" % (
        flavour, off.max())


# ---- the packed form
TAIL, CANARY, NANFILL = 64, 0x5A5A5A5A, 0x7FD12345


def check_blob(name, words):
    """words uint32 [n]: what a pack wrote over a NaN pattern"""
    want, used = npp.pack(pn.net(KIND, name))
    assert words.size == want.size, "%s: %d words, the layout has %d" % (name, words.size, want.size)
    diff = np.nonzero(words != want.view(np.uint32))[0]
    assert diff.size == 0, "%s: %d packed words differ, the first at %d (%s a weight's word): %#x for %#x" % (
        name, diff.size, diff[0], "" if used[diff[0]] else "not", words[diff[0]], want.view(np.uint32)[diff[0]])
    assert (words[~used] == 0).all()


@pytest.mark.skipif(not HAVE_HIPCC, reason="needs hipcc")
@pytest.mark.parametrize("name", NETS)
def test_host_pack_word_by_word(name):
    """lhp_policy_pack over a NaN pattern with a canary tail, as the device test does for ss_policy_pack"""
    import lookahead_policy_host_lib as lhp
    layers = pn.net(KIND, name)
    d = lhp.desc_of(layers)
    n = lhp.words(d)
    assert n == npp.layout(npp.widths_of(layers))["words"]
    ws = [np.ascontiguousarray(w, np.float32) for w, _, _ in layers]
    bs = [np.ascontiguousarray(b, np.float32) for _, b, _ in layers]
    wp, bp = (C.c_void_p * len(layers))(*[w.ctypes.data for w in ws]), (C.c_void_p * len(layers))(*[b.ctypes.data for b in bs])
    target = np.concatenate([np.full(n, NANFILL, np.uint32), np.full(TAIL, CANARY, np.uint32)])
    assert lhp.load().lhp_policy_pack(C.byref(d), wp, bp, target.ctypes.data_as(C.c_void_p)) == 0
    assert (target[n:] == CANARY).all(), "%s: the words behind the blob were written" % name
    check_blob(name, target[:n])
    assert (lhp.pack(layers)[1].view(np.uint32) == target[:n]).all()          # the binding the look-ahead tests pack with


@pytest.mark.gpu
def test_device_pack_word_by_word():
    """The device blob equals the host build's: both are held, bit for bit, to the same np_policy.pack (the host one by
    test_host_pack_word_by_word), so this test compiles no host code on the GPU machine."""
    import torch
    import lookahead_cases as lc
    from steppingstone_amd import _lib
    from steppingstone_amd.envs import SteppingStoneVecEnv, _ptr, _stream
    dev = "cuda:0"
    e = SteppingStoneVecEnv(lc.ENV_IDS[KIND], 1, seed=0, device=dev)
    lib = e.backend.lib
    for name in NETS:
        layers = pn.net(KIND, name)
        d = _lib.PolicyDesc()
        d.layers = len(layers)
        for i, w in enumerate(npp.widths_of(layers)):
            d.width[i] = w
        for i, (_, _, a) in enumerate(layers):
            d.activation[i] = pn.CODE[a]
        n = int(lib.ss_policy_words(C.byref(d)))
        assert n == npp.layout(npp.widths_of(layers))["words"]
        ws = [torch.from_numpy(w.copy()).to(dev) for w, _, _ in layers]
        bs = [torch.from_numpy(b.copy()).to(dev) for _, b, _ in layers]
        wp, bp = (C.c_void_p * len(layers))(*[w.data_ptr() for w in ws]), (C.c_void_p * len(layers))(*[b.data_ptr() for b in bs])
        target = torch.cat([torch.full((n,), NANFILL, dtype=torch.int32), torch.full((TAIL,), CANARY, dtype=torch.int32)]).to(dev)
        assert lib.ss_policy_pack(e.backend.h, C.byref(d), wp, bp, _ptr(target), _stream(e.device)) == 0
        torch.cuda.synchronize()
        got = target.cpu().numpy().view(np.uint32)
        assert (got[n:] == CANARY).all(), "%s: the words behind the blob were written" % name
        check_blob(name, got[:n])
    e.close()


# ---- the emulation of fmaf
@pytest.mark.skipif(not HAVE_HIPCC, reason="needs hipcc")
def test_fmaf_emulation_against_the_c_library():
    """1.4 million triples: random bit patterns (every class of float); normal operands; cancellations a * b ~ -c to the last bits, where
    a double rounding shows; products and sums that land among the denormals; sums at and past the overflow threshold"""
    g = np.random.default_rng(99)
    m = 200_000
    f = lambda bits: bits.astype(np.uint32).view(np.float32)
    rnd = lambda: f(g.integers(0, 1 << 32, m, dtype=np.uint64))
    nrm = lambda lo, hi: (g.standard_normal(m) * np.exp2(g.uniform(lo, hi, m))).astype(np.float32)
    sets = [(rnd(), rnd(), rnd()), (nrm(-20, 20), nrm(-20, 20), nrm(-40, 40))]
    a, b = nrm(-10, 10), nrm(-10, 10)
    p = a.astype(np.float64) * b.astype(np.float64)
    near = (-p).astype(np.float32)
    sets.append((a, b, f(near.view(np.uint32).astype(np.int64) + g.integers(-2, 3, m))))           # cancellation to within 2 ulp
    sets.append((a, b, (-p * (1 + g.integers(-3, 4, m) * 2.0 ** -25)).astype(np.float32)))        # ... around the half-ulp ties
    sets.append((nrm(-70, -55), nrm(-70, -55), nrm(-150, -120)))                                  # denormal results
    with np.errstate(over="ignore"):
        sets.append((nrm(62, 65), nrm(62, 65), nrm(120, 128)))                                    # overflow
    # products that are exact ties of float32 (25 significant bits, the last one set) beside a c far below the last bit of a double:
    # the f64 sum is the tie, whose cast rounds to even, while fmaf goes by the sign of c
    i, j = g.integers(1 << 11, 1 << 12, m) | 1, g.integers(1 << 12, 1 << 13, m) | 1
    scale = np.exp2(g.integers(-30, 30, m))
    sets.append(((i * scale).astype(np.float32), j.astype(np.float32), (g.choice([-1.0, 1.0], m) * scale * np.exp2(-50.0 - g.integers(0, 20, m))).astype(np.float32)))
    worst = 0
    for i, (a, b, c) in enumerate(sets):
        with np.errstate(all="ignore"):
            got, want = npp.fmaf(a, b, c), pl.c_fmaf(a, b, c)
            twice = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
        ok = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
        assert ok.all(), "set %d: fmaf(%r, %r, %r) = %r, the emulation gives %r" % ((i,) + tuple(
            float(v[np.nonzero(~ok)[0][0]]) for v in (a, b, c, want, got)))
        worst += int(((twice.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(twice) & np.isnan(want))).sum())
        if i == 4:
            assert (np.abs(want[want != 0]) < 2.0 ** -126).mean() > 0.2, "the denormal set misses the denormals"
        if i == 5:
            assert np.isinf(want).mean() > 0.1 and np.isfinite(want).mean() > 0.2
    print("fmaf: %d triples; a plain f64 a * b + c differs from fmaf on %d of them" % (len(sets) * m, worst))
    assert worst > 0, "the triples do not tell a double rounding from fmaf"
