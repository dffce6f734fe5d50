"""The networks of the closed-loop look-ahead tests (tests/test_lookahead_policy.py, tests/test_gpu_lookahead_policy.py) as lists of
(weight [out,in] f32, bias [out] f32, activation) triples, and the references their actions are judged by.  TEST INFRASTRUCTURE.
  shipped   the reference's shipped actor of the robot (tests/golden/shipped_actor_<kind>.npz): 60 -> 256 x5 -> 21
  ragged    60 -> 37 -> 50 -> 21, softsign / relu / tanh, from a seeded numpy generator: widths that are no multiple of the 32-wide tile,
            scaled so that the tanh outputs stay well inside (-1, 1)
  linear    60 -> 21, identity: one layer, no activation
SHAPES / SHAPE_NAMES: eight more, for tests/test_policy_ops.py and the H = 2 look-aheads (NAMES stays the three above)."""
import functools
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("shipped", "ragged", "linear")
CODE = {"identity": 0, "relu": 1, "softsign": 2, "tanh": 3}
# The nets of the operator-level tests (tests/test_policy_ops.py) and of the H = 2 look-aheads: shapes the three above do not reach.
# Weights from a seeded generator with gain 1 / sqrt(K), biases 0.1 sigma: activations stay O(1) at any depth.  Among them every
# activation stands in a hidden and in the last position.  (Np, Kp: a layer's widths rounded up to the 32-column tile; the kernel
# walks Kp in groups of 32 with a prefetch one group ahead, and a layer's Np / 32 tiles go round its four wavefronts.)
_I, _R, _S, _T = "identity", "relu", "softsign", "tanh"
SHAPES = {
    "w1": ((60, 1, 21), (_R, _I)),                                        # width 1; Kp = 32: one group, the prefetch re-reads group 0
    "edge": ((60, 31, 32, 33, 21), (_S, _T, _R, _S)),                     # the tile edge from both sides; groups 1 and 2
    "deep8": ((60,) + (8,) * 7 + (21,), (_I,) * 8),                       # 8 layers, all identity
    "wide8": ((60,) + (256,) * 7 + (21,), (_R, _I, _R, _R, _I, _R, _R, _I)),      # 8 layers at full width
    "t854": ((60, 255, 129, 97, 21), (_T, _S, _R, _T)),                   # tiles 8 / 5 / 4, Kp 256 / 160 / 128
    "t753": ((60, 224, 160, 96, 21), (_R, _I, _R, _I)),                   # tiles 7 / 5 / 3, an odd number of groups
    "neck": ((60, 256, 1, 256, 21), (_T, _I, _S, _R)),                    # a wide layer behind a narrow one in the same block
    "p33": ((60, 33, 21), (_T, _S)),                                      # 2 layers: the action tile in the other block
}
SHAPE_NAMES = tuple(SHAPES)


@functools.lru_cache(maxsize=None)
def net(kind, name):
    if name == "shipped":
        w = np.load(os.path.join(GOLD, "shipped_actor_%s.npz" % kind))
        layers = [("fc%d" % i, a) for i, a in ((1, "softsign"), (2, "softsign"), (3, "softsign"), (4, "relu"), (5, "relu"))] + [("out", "tanh")]
        out = [(w[n + ".weight"].astype(np.float32), w[n + ".bias"].astype(np.float32), a) for n, a in layers]
    elif name == "ragged":
        g = np.random.default_rng(7)
        widths, acts = (60, 37, 50, 21), ("softsign", "relu", "tanh")
        out = [((g.standard_normal((widths[i + 1], widths[i])) * (0.8 / np.sqrt(widths[i]))).astype(np.float32),
                (g.standard_normal(widths[i + 1]) * 0.1).astype(np.float32), acts[i]) for i in range(3)]
    elif name == "linear":
        g = np.random.default_rng(11)
        out = [((g.standard_normal((21, 60)) * 0.05).astype(np.float32), (g.standard_normal(21) * 0.1).astype(np.float32), "identity")]
    elif name in SHAPES:
        widths, acts = SHAPES[name]
        g = np.random.default_rng(100 + SHAPE_NAMES.index(name))
        out = [((g.standard_normal((widths[i + 1], widths[i])) / np.sqrt(widths[i])).astype(np.float32),
                (g.standard_normal(widths[i + 1]) * 0.1).astype(np.float32), acts[i]) for i in range(len(acts))]
    else:
        raise KeyError(name)
    for w, b, _ in out:
        w.setflags(write=False)
        b.setflags(write=False)
    return out


def _act(a, x):
    if a == "relu":
        return np.maximum(x, 0)
    if a == "softsign":
        return x / (1 + np.abs(x))
    if a == "tanh":
        return np.tanh(x)
    return x


def eval64(layers, x):
    """the net in fp64 on x [..., 60] (float32 inputs, exactly converted)"""
    y = np.asarray(x, np.float64)
    for w, b, a in layers:
        y = _act(a, y @ w.astype(np.float64).T + b.astype(np.float64))
    return y


def eval32(layers, x):
    """a plain float32 evaluation in index order: every product and every sum rounded to float32, k ascending, the bias added last"""
    y = np.asarray(x, np.float32)
    for w, b, a in layers:
        s = np.zeros(y.shape[:-1] + (w.shape[0],), np.float32)
        for k in range(w.shape[1]):
            s = (s + (y[..., k:k + 1] * w[None, :, k]).astype(np.float32)).astype(np.float32)
        y = _act(a, (s + b).astype(np.float32)).astype(np.float32)
    return y


def judge_actions(layers, act, offset, inputs, live, what=""):
    """Test 2: on the live steps, act - offset against the fp64 evaluation of the net on `inputs` (the observations the actions were
    computed from).  E = the largest deviation of the plain float32 evaluation from fp64 on the same inputs; the code under test must stay
    within 8 E.  The offset is subtracted in fp64 from the float32 sum act = f + offset, whose own rounding (half an ulp of |act|) is
    part of what is measured against E.  -> (E, largest deviation)"""
    x = inputs[live]
    want = eval64(layers, x)
    e = float(np.abs(eval32(layers, x).astype(np.float64) - want).max())
    got = act[live].astype(np.float64) - (0 if offset is None else offset[live].astype(np.float64))
    dev = float(np.abs(got - want).max())
    print("%s: %d live actions rows, E = %.3e, largest deviation %.3e (%.2f E)" % (what, x.shape[0], e, dev, dev / e))
    assert x.shape[0] > 0 and np.isfinite(want).all()
    assert dev <= 8 * e, "%s: actions deviate %.3e from the fp64 net, 8 E = %.3e" % (what, dev, 8 * e)
    return e, dev
