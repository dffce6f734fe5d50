"""The rows tests/test_push.py and tests/test_gpu_push.py judge the impulse on, the asserted error factor, and the judgements both
share.  TEST INFRASTRUCTURE ONLY.

cases(kind): the rows of kinematics_cases.sample(kind) (about 200 per robot) and, per row, a drawn push: body (every one of the 22 at
least 8 times, the massless links included), point mode (0: NULL, the centre of mass; 1: the link origin; 2: 0.3 m off the link origin in
a drawn direction), and a wrench impulse p | L of size log-uniform in 1e-3 .. 1e2 (N s for p, N m s for L), pure p, pure L or mixed; at
least 8 rows are all zeros.  draw(n, seed) is the same drawing for any number of rows (the GPU test's 70).

K: omega <= K is asserted, omega the componentwise backward error of np_push in units of 2^-24.  K is 4 x the worst omega the CPU build
of steppingstone_amd/csrc/ss_push.hpp reached on cases() of both robots (WORST below; docs/HISTORY.md has them per robot), measured
against the fp64 restatement, never against the GPU build: the margin covers the gfx950 build contracting the same source expressions
differently, and the GPU test's states being another draw."""
import functools

import numpy as np

import eom_cases as ec
import kinematics_cases as kc
import np_push as npp

KINDS = kc.KINDS
U = npp.U
NB = 22
OFFSET = 0.3
MODES = ("null", "origin", "offset")
WRENCHES = ("p", "L", "mixed")

# worst omega of the host build over cases() of both robots, rounded up in the third digit, and the asserted factor: 4 x that.
# Measured (walker3d / mike): 31.08 / 37.54.
WORST = 37.6
K = 4.0 * WORST


def model(kind):
    return kc.model(kind)


def draw(n, seed, zeros=10):
    """n pushes: dict(body [n] int32, mode [n] (index into MODES), point [n,3] float32 (zeros for modes 0 and 1), wrench [n] (index into
    WRENCHES), impulse [n,6] float32); `zeros` of the rows have an all-zero impulse"""
    rng = np.random.default_rng([seed, 9127])
    body = rng.permutation(np.arange(n) % NB).astype(np.int32)
    mode = rng.permutation(np.arange(n) % 3)
    wrench = rng.permutation(np.arange(n) % 3)
    d = rng.normal(size=(n, 3))
    point = np.where((mode == 2)[:, None], OFFSET * d / np.linalg.norm(d, axis=1, keepdims=True), 0.0)
    imp = np.zeros((n, 6))
    for h, on in ((0, wrench != 1), (1, wrench != 0)):
        v = rng.normal(size=(n, 3))
        size = 10.0 ** rng.uniform(-3, 2, n)
        imp[:, 3 * h:3 * h + 3] = np.where(on[:, None], size[:, None] * v / np.linalg.norm(v, axis=1, keepdims=True), 0.0)
    imp[rng.choice(n, zeros, replace=False)] = 0.0
    return dict(body=body, mode=mode, point=point.astype(np.float32), wrench=wrench, impulse=imp.astype(np.float32))


@functools.lru_cache(maxsize=None)
def cases(kind):
    st = kc.sample(kind)
    c = draw(st.shape[0], KINDS.index(kind))
    c["st"] = st
    for v in c.values():
        v.setflags(write=False)
    return c


def check_counts(c, per_body=8, zeros=8):
    """the properties of a case set that the tests rely on: a thinned set fails here"""
    nonzero = (c["impulse"] != 0).any(axis=1)
    assert (np.bincount(c["body"], minlength=NB) >= per_body).all() and c["body"].min() >= 0 and c["body"].max() == NB - 1
    assert (~nonzero).sum() >= zeros
    for i, _ in enumerate(MODES):
        assert ((c["mode"] == i) & nonzero).sum() >= per_body, "point mode %s" % MODES[i]
    for i, _ in enumerate(WRENCHES):
        assert ((c["wrench"] == i) & nonzero).sum() >= per_body, "wrench %s" % WRENCHES[i]
    off = np.linalg.norm(c["point"][c["mode"] == 2].astype(np.float64), axis=1)
    assert np.allclose(off, OFFSET, rtol=1e-6) and (c["point"][c["mode"] != 2] == 0).all()
    size = np.concatenate([np.linalg.norm(c["impulse"][:, :3], axis=1), np.linalg.norm(c["impulse"][:, 3:], axis=1)])
    size = size[size > 0]
    assert size.min() < 1e-2 and size.max() > 1e1 and size.min() >= 0.99e-3 and size.max() <= 1.01e2
    p_only = nonzero & (c["wrench"] == 0)
    assert (c["impulse"][p_only, 3:] == 0).all() and (c["impulse"][nonzero & (c["wrench"] == 1), :3] == 0).all()


def point_arg(c, i):
    """row i's point as np_push.reference takes it: None for mode 0"""
    return None if c["mode"][i] == 0 else c["point"][i]


def references(kind, st, c, readouts=None):
    """np_push.reference of every row (readouts: np_eom.readout of the rows, where they exist already)"""
    m = model(kind)
    return [npp.reference(m, st[i], int(c["body"][i]), point_arg(c, i), c["impulse"][i], readouts[i] if readouts else None)
            for i in range(st.shape[0])]


@functools.lru_cache(maxsize=None)
def case_references(kind):
    """references of cases(kind): computed once, shared by the tests, never changed"""
    c = cases(kind)
    return tuple(references(kind, c["st"], c, ec.references(kind)))       # eom_cases' rows are the same sample(kind)


def omegas(refs, dnu):
    return np.array([npp.omega(r, d) for r, d in zip(refs, dnu)])


def shifted(rows):
    return ec.shifted(rows)
