"""The policy MLP of the closed-loop look-ahead (docs/PHYSICS.md 14) in numpy, written from that section and from the layout comment at
the head of steppingstone_amd/csrc/ss_policy.hpp; no compiled code.  TEST INFRASTRUCTURE for tests/test_policy_ops.py and the H = 2
look-aheads of tests/test_lookahead_policy.py / tests/test_gpu_lookahead_policy.py.

  layout, w_index, pack     the packed form: per layer the weights as the B operands of the matrix instruction, then the biases
  fmaf, chain               the documented sum, exactly: one f32 fma chain per dot product, from the bias, k ascending, every step a
                            correctly rounded fmaf (exact f64 product, TwoSum, round to odd, one cast; a plain f64 a * b + c rounds
                            twice).  Only for nets whose activations are identity / relu: those have no rounding of their own
  eval64                    every layer in fp64 with a running error bound per element (the style of tests/np_spatial.py)
  blocks, judge             what the probe's dump (tests/probe_lib.py: mlp) must hold word by word, and the verdict
  judge_last_layer          the last layer alone from the dumped layer before it: one layer's bound (the running bound of a deep net
                            grows by a layer's sum |w| ~ sqrt(K) per layer, and a small error in its last layer would hide in it)

The bound.  u = 2^-24.  A sum s = b + sum_k w_k x_k whose inputs carry the errors err(x_k) is held to
    err(s) = (K + 1) u (sum |w_k| |x_k| + |b|) + sum |w_k| err(x_k)
(K the layer's own input width; the padded terms are zeros and round nothing; where the bound is 0 the result must be exact).  Nothing
is added for values below the normal range: the nets' biases are of order 0.1, so no judged sum is denormal, and
test_policy_ops.py holds denormal operands and results to the exact chain, bit for bit, on their own.  An activation has Lipschitz
constant 1, so err(s) passes through, plus its own roundings: none for identity and relu; two for softsign (the sum 1 + |s| and the
correctly rounded division), 2 u / (1 - u) |y|; for tanh T ulp of |y|, T = TANH_ULPS[flavour]: the measured deviation of the flavour's
tanhf from fp64 tanh over a dense sweep (test_policy_ops.py measures it through the probe on every run), rounded up to a whole ulp, plus
one; an ulp of |y| is taken as 2^-23 |y|, its upper end.  Every element is judged against its own bound; no maximum is taken."""
import functools

import numpy as np

import policy_nets as pn

U = 2.0 ** -24
TANH_ULPS = {"host": 4, "device": 3}         # the measured ulps (docs/HISTORY.md) rounded up to a whole one, plus one
TILE, MAX_WIDTH = 32, 256
CHAIN_ACTS = ("identity", "relu")


# ---- the packed form
def layout(widths):
    """widths [layers + 1] -> dict(kp, np, woff, boff: per layer; words)"""
    kp, npad, woff, boff, off = [], [], [], [], 0
    for l in range(len(widths) - 1):
        kp.append(64 if l == 0 else npad[l - 1])
        npad.append((widths[l + 1] + TILE - 1) // TILE * TILE)
        woff.append(off)
        off += npad[l] * kp[l]
        boff.append(off)
        off += npad[l]
    return dict(kp=kp, np=npad, woff=woff, boff=boff, words=off)


def w_index(lay, l, n, k):
    """the word of W[n][k] of layer l (n, k: integer arrays)"""
    kk = k // 2
    return lay["woff"][l] + (((n // 32) * (lay["kp"][l] // 8) + kk // 4) * 64 + (k % 2) * 32 + n % 32) * 4 + kk % 4


def widths_of(layers):
    return [layers[0][0].shape[1]] + [w.shape[0] for w, _, _ in layers]


def pack(layers):
    """-> (blob float32 [words]: every weight and bias at its word, +0 everywhere else; used bool [words]: the words that hold one)"""
    lay = layout(widths_of(layers))
    blob, used = np.zeros(lay["words"], np.float32), np.zeros(lay["words"], bool)
    for l, (w, b, _) in enumerate(layers):
        n, k = np.meshgrid(np.arange(w.shape[0]), np.arange(w.shape[1]), indexing="ij")
        at = w_index(lay, l, n, k)
        assert not used[at].any() and np.unique(at).size == at.size and at.max() < lay["boff"][l] and at.min() >= lay["woff"][l]
        blob[at], used[at] = w, True
        at = lay["boff"][l] + np.arange(b.size)
        assert not used[at].any()
        blob[at], used[at] = b, True
    return blob, used


# ---- the exact chain
def fmaf(a, b, c):
    """the correctly rounded float32 a * b + c, elementwise.  The f64 product of two floats is exact; TwoSum gives the f64 sum s and its
    exact error e; s is moved to the neighbour with an odd last bit where e != 0 and its own is even (round to odd), after which the cast
    to float32 rounds once: 53 bits are more than 24 + 2.  Infinities and NaNs take the plain f64 path."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = np.ascontiguousarray(p + c)
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        fin = np.isfinite(s)
        e = np.where(fin, e, 0.0)
        even = (s.view(np.int64) & 1) == 0
        fix = fin & (e != 0) & even
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def act32(a, s):
    if a == "relu":
        return np.where(s < 0, np.float32(0), s)          # a NaN stays a NaN
    assert a == "identity", a
    return s


def is_chain_net(layers):
    return all(a in CHAIN_ACTS for _, _, a in layers)


def chain(layers, x):
    """every layer [n, nout] float32 of an identity / relu net as the documented chain gives it"""
    y, outs = np.asarray(x, np.float32), []
    for w, b, a in layers:
        s = np.broadcast_to(b, (y.shape[0], b.size)).astype(np.float32)
        for k in range(w.shape[1]):
            s = fmaf(y[:, k:k + 1], w[None, :, k], s)
        y = act32(a, s)
        outs.append(y)
    return outs


# ---- fp64 with a running bound
def eval64(layers, x, tanh_ulps):
    """-> [(y, err)] per layer, float64 [n, nout] each"""
    y = np.asarray(x, np.float32).astype(np.float64)
    e, outs = np.zeros_like(y), []
    for w, b, a in layers:
        w64, b64 = w.astype(np.float64), b.astype(np.float64)
        aw, k = np.abs(w64), w.shape[1]
        s = y @ w64.T + b64
        es = (k + 1) * U * (np.abs(y) @ aw.T + np.abs(b64)) + e @ aw.T
        if a == "relu":
            y, e = np.maximum(s, 0), es
        elif a == "softsign":
            y = s / (1 + np.abs(s))
            e = es + 2 * U / (1 - U) * np.abs(y)
        elif a == "tanh":
            y = np.tanh(s)
            e = es + tanh_ulps * 2 * U * np.abs(y)
        else:
            y, e = s, es
        outs.append((y, e))
    return outs


PREFILL, REAL, PAD = 0, 1, 2


def blocks(layers, per_layer):
    """The two activation blocks behind one phase, word by word: layer l writes columns [0, Np_l) of block l & 1 -- its own outputs, then
    zeros -- over what layer l - 2 left there.  per_layer: eval64's list.  -> (val [n,2,256], err [n,2,256], cls [2,256], layer [2,256])"""
    n = per_layer[0][0].shape[0]
    val, err = np.zeros((n, 2, MAX_WIDTH)), np.zeros((n, 2, MAX_WIDTH))
    cls, who = np.zeros((2, MAX_WIDTH), np.int8), np.full((2, MAX_WIDTH), -1)
    npad = layout(widths_of(layers))["np"]
    for l, (y, e) in enumerate(per_layer):
        b, nout = l & 1, y.shape[1]
        val[:, b, :npad[l]], err[:, b, :npad[l]] = 0, 0
        val[:, b, :nout], err[:, b, :nout] = y, e
        cls[b, :nout], cls[b, nout:npad[l]], who[b, :npad[l]] = REAL, PAD, l
    return val, err, cls, who


def judge(dump, ref, prefill):
    """dump: uint32 [>= n, 2, 256] (probe_lib.mlp); ref: blocks(...).  Rows below n: every real word within its own bound (a NaN is
    outside any), every padded word +-0; all rows: every word the net does not write still the prefill.
    -> (worst err / bound over the real words of the last two layers, list of failures (what, row, block, column, got, want, bound))"""
    val, err, cls, who = ref
    n, fails = val.shape[0], []
    got = dump.view(np.float32).astype(np.float64)
    for b, c in zip(*np.nonzero(cls == PREFILL)):
        bad = np.nonzero(dump[:, b, c] != prefill)[0]
        fails += [("prefill", int(r), int(b), int(c), hex(int(dump[r, b, c])), hex(prefill), 0.0) for r in bad[:2]]
    pad = np.broadcast_to(cls == PAD, (n, 2, MAX_WIDTH))
    for r, b, c in zip(*np.nonzero(pad & ((dump[:n] & 0x7FFFFFFF) != 0))):
        fails.append(("pad", int(r), int(b), int(c), float(got[r, b, c]), 0.0, 0.0))
    real = np.broadcast_to(cls == REAL, (n, 2, MAX_WIDTH))
    d = np.abs(got[:n] - val)
    with np.errstate(invalid="ignore"):
        out = real & ~(d <= err)
    for r, b, c in zip(*np.nonzero(out)):
        fails.append(("layer %d" % who[b, c], int(r), int(b), int(c), float(got[r, b, c]), float(val[r, b, c]), float(err[r, b, c])))
    last2 = real & (who >= who.max() - 1)[None] & (err > 0)
    worst = float((d[last2] / err[last2]).max()) if last2.any() and np.isfinite(d[last2]).all() else float("inf") if last2.any() else 0.0
    return worst, fails


def judge_last_layer(layers, dump, x, tanh_ulps):
    """The last layer on its own: from the words it read -- the dumped layer before it (x for a one-layer net), exact inputs -- so its
    bound is one layer's, (K + 1) u (sum |w| |x| + |b|) and the activation's roundings, however deep the net is.
    -> (worst err / bound, list of (row, column, got, want, bound))"""
    n = x.shape[0]
    last, prev = layer_views(layers, dump, n)
    (y, e), = eval64(layers[-1:], x if prev is None else prev, tanh_ulps)
    d = np.abs(last.astype(np.float64) - y)
    with np.errstate(invalid="ignore"):
        out = ~(d <= e)
    fails = [(int(r), int(c), float(last[r, c]), float(y[r, c]), float(e[r, c])) for r, c in zip(*np.nonzero(out))]
    return (float((d / e).max()) if np.isfinite(d).all() else float("inf")), fails


def layer_views(layers, dump, n):
    """the last layer's 21 real columns and the layer before it (its own columns; None for a one-layer net), float32 [n, .]"""
    L = len(layers)
    f = dump.view(np.float32)
    last = f[:n, (L - 1) & 1, :layers[-1][0].shape[0]]
    prev = f[:n, (L - 2) & 1, :layers[-2][0].shape[0]] if L >= 2 else None
    return last, prev


# ---- the rows the tests feed
@functools.lru_cache(maxsize=None)
def rows():
    """{name: x [n,60] float32}, n = 1, 32, 33, 70: standard normal, the same at 1e-3 and at 1e3, and a mixed set whose rows 50..59 are
    +0, -0, one entry at k = 0 (two signs), one at k = 59 (two signs), all denormal, every third entry denormal, one denormal at k = 0,
    one at k = 59.  DENORMAL_ROWS names the rows of "n70" that hold a denormal."""
    g = np.random.default_rng(2024)
    base = g.standard_normal((70, 60)).astype(np.float32)
    mix = base.copy()
    mix[50:60] = 0
    mix[51] = -0.0
    mix[52, 0], mix[53, 0], mix[54, 59], mix[55, 59] = 1.5, -2.25, 0.75, -3.0
    den = (g.integers(1, 1 << 23, (4, 60)).astype(np.uint32) | (g.integers(0, 2, (4, 60)).astype(np.uint32) << np.uint32(31))).view(np.float32)
    mix[56] = den[0]
    mix[57] = base[57]
    mix[57, ::3] = den[1, ::3]
    mix[58, 0], mix[59, 59] = den[2, 0], den[3, 59]
    mix[60:65] *= np.float32(1e-3)
    mix[65:70] *= np.float32(1e3)
    out = {"n1": base[:1].copy(), "n32": base[:32] * np.float32(1e-3), "n33": base[:33] * np.float32(1e3), "n70": mix}
    for v in out.values():
        v.setflags(write=False)
    return out


DENORMAL_ROWS = (56, 57, 58, 59)


@functools.lru_cache(maxsize=None)
def reference(kind, name, rows_name, flavour):
    """blocks() of net `name` on rows()[rows_name] under the flavour's tanh figure: computed once, shared, left unchanged"""
    layers = pn.net(kind, name)
    ref = blocks(layers, eval64(layers, rows()[rows_name], TANH_ULPS[flavour]))
    for a in ref:
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def chain_reference(kind, name, rows_name):
    outs = chain(pn.net(kind, name), rows()[rows_name])
    for a in outs:
        a.setflags(write=False)
    return outs


def same_bits(a, b):
    """float32 arrays equal bit for bit, zeros of either sign equal (the product is built with -fno-signed-zeros), NaN equal to NaN"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0)) | (np.isnan(a) & np.isnan(b))


# ---- tanhf through the probe
def tanh_net():
    """60 -> 21, tanh, W = the first 21 rows of the identity, b = 0: the chain of column n is 0, .., 0 + x_n * 1, .. = x_n exactly, so
    action n is the flavour's tanhf(x_n)"""
    return [(np.eye(21, 60, dtype=np.float32), np.zeros(21, np.float32), "tanh")]


def tanh_sweep():
    """2 x 2^17 arguments: every 1152nd float of [2^-14, 16) and its negative, then a few at the ends, padded to whole rows of 21 (x [n,60])"""
    lo, hi = np.array([2.0 ** -14, 16.0], np.float32).view(np.uint32)
    pos = (int(lo) + (np.arange(1 << 17, dtype=np.int64) * (int(hi) - int(lo)) >> 17)).astype(np.uint32).view(np.float32)
    ends = np.array([0.0, 1e-40, 1e-30, 2.0 ** -24, 16.0, 20.0, 88.0, 89.0, 1e4, 3e38], np.float32)
    arg = np.concatenate([pos, -pos, ends, -ends])
    n = (arg.size + 20) // 21
    x, cols = np.zeros((n, 60), np.float32), np.zeros(n * 21, np.float32)
    cols[:arg.size] = arg
    x[:, :21] = cols.reshape(n, 21)
    return x


def ulps_off(got, want64):
    """|got - want| in units in the last place of float32 at |want| (fp64 want), elementwise"""
    want64 = np.asarray(want64, np.float64)
    with np.errstate(divide="ignore"):
        ex = np.floor(np.log2(np.maximum(np.abs(want64), 2.0 ** -126)))
    return np.abs(np.asarray(got, np.float64) - want64) / 2.0 ** (ex - 23)
