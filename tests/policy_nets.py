"""The networks of the closed-loop look-ahead tests (tests/test_lookahead_policy.py, tests/test_gpu_lookahead_policy.py) as lists of
(weight [out,in] f32, bias [out] f32, activation) triples, and the references their actions are judged by.  TEST INFRASTRUCTURE.
  shipped   the reference's shipped actor of the robot (tests/golden/shipped_actor_<kind>.npz): 60 -> 256 x5 -> 21
  ragged    60 -> 37 -> 50 -> 21, softsign / relu / tanh, from a seeded numpy generator: widths that are no multiple of the 32-wide tile,
            scaled so that the tanh outputs stay well inside (-1, 1)
  linear    60 -> 21, identity: one layer, no activation"""
import functools
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("shipped", "ragged", "linear")
CODE = {"identity": 0, "relu": 1, "softsign": 2, "tanh": 3}


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
