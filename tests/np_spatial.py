"""fp64 references, running error bounds and test cases for the operators that tests/device/ss_probe.hip exposes (the spatial algebra
of ss_math.hpp / ss_pair.hpp and the per-joint helpers of ss_dynamics.hpp).  Built on tests/np_dynamics.py and
steppingstone_amd.model.build(kind): NOT on the generated ss_model_tables.hpp, so a wrong constant in a kernel table or in a literal
pair of ss_pair.hpp shows as an error here.

For every op:  cases(kind) -> inp [n, IN_W] float32 (the probe's input rows; n is never a multiple of 64),
               ref(kind, inp) -> (ref, B, exact), all [n, OUT_W]: the fp64 value, its running error bound (the same formula with every
               factor replaced by its entrywise absolute value) and a mask of the components that must come out bit-exact.
A component passes when |got - ref| <= k * 2^-24 * B; where B == 0 it must be exactly 0 (the kernels drop terms whose constexpr
coefficient is zero, and nothing else).  cos / sin reach the kernels as fp32 inputs and the reference builds its rotation from those
same two numbers, so both sides start from identical data; the model constants are fp64 here and fp32 tables there (one rounding
each, counted in k)."""
import functools

import numpy as np

import np_dynamics as nd
from steppingstone_amd import model as M

U = 2.0 ** -24
KINDS = ["walker3d", "mike"]
N_RANDOM = 64
# the {leg, arm} joint pairs of ss_pair.hpp and their child bodies
PAIR_JOINTS = [(3, 13), (4, 14), (5, 15), (6, 16)]
PAIR_BODIES = [(4, 14), (5, 15), (6, 16), (7, 17)]
ABI_IDX = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]      # Sym3T: xx yy zz xy xz yz


@functools.lru_cache(maxsize=None)
def model(kind):
    return M.build(kind)


# ---------------------------------------------------------------- layouts
def abi_to_dense(a):
    """probe row abi21 (A.m[6], B[3][3] row-major, C.m[6]) -> 6x6 [[A, B], [B^T, C]]."""
    a = np.asarray(a, np.float64)
    I = np.zeros((6, 6))
    for k, (i, j) in enumerate(ABI_IDX):
        I[i, j] = I[j, i] = a[k]
        I[3 + i, 3 + j] = I[3 + j, 3 + i] = a[15 + k]
    I[:3, 3:] = a[6:15].reshape(3, 3)
    I[3:, :3] = I[:3, 3:].T
    return I


def dense_to_abi(I):
    return np.concatenate([[I[i, j] for i, j in ABI_IDX], I[:3, 3:].reshape(9), [I[3 + i, 3 + j] for i, j in ABI_IDX]])


def rot_cs(ax, c, s):
    """Active rotation about coordinate axis ax from a given cosine / sine (not re-normalised: the kernels do not either)."""
    i, j = (ax + 1) % 3, (ax + 2) % 3
    R = np.zeros((3, 3))
    R[ax, ax] = 1.0
    R[i, i] = c
    R[i, j] = -s
    R[j, i] = s
    R[j, j] = c
    return R


def joint_xform(m, j, c, s):
    """(X, |X|) of joint j: X = xform(R^T, r_j); |X| takes every factor's absolute value (|E| |skew r| for the lower-left block)."""
    E = rot_cs(M.AXIS[j], c, s).T
    r = m["r"][j]
    X = nd.xform(E, r)
    aX = np.zeros((6, 6))
    aX[:3, :3] = aX[3:, 3:] = np.abs(E)
    aX[3:, :3] = np.abs(E) @ np.abs(nd.skew(r))
    return X, aX


# ---------------------------------------------------------------- case generation
def _scale(rng):
    return 10.0 ** rng.uniform(-3.0, 3.0)


def _vec(rng, w):
    return rng.uniform(-1.0, 1.0, w) * _scale(rng)


def _abi(rng):
    """random symmetric A and C, general B"""
    return rng.uniform(-1.0, 1.0, 21) * _scale(rng)


def _cs(q):
    return np.float32(np.cos(q)), np.float32(np.sin(q))


def _edge_angles(m, j):
    return [0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi, m["range"][j, 0], m["range"][j, 1]]


def _angle_payload_cases(rng, m, j, payload, axis_payload):
    """[(q, payload)] for joint j: N_RANDOM random draws, the edge angles, a zero payload, a payload along the joint axis only."""
    out = [(rng.uniform(-np.pi, np.pi), payload(rng)) for _ in range(N_RANDOM)]
    out += [(q, payload(rng)) for q in _edge_angles(m, j)]
    out.append((rng.uniform(-np.pi, np.pi), np.zeros_like(payload(rng))))
    out.append((rng.uniform(-np.pi, np.pi), axis_payload(rng, M.AXIS[j])))
    return out


def _sv_axis(rng, ax):
    v = np.zeros(6)
    v[ax], v[3 + ax] = rng.uniform(-1, 1, 2) * _scale(rng)
    return v


def _abi_axis(rng, ax):
    """an inertia that couples the joint axis only: A[ax][ax], B[ax][ax], C[ax][ax]"""
    a = np.zeros(21)
    a[ax], a[6 + 4 * ax], a[15 + ax] = rng.uniform(-1, 1, 3) * _scale(rng)
    return a


def _rec(rng, q):
    """a joint record cs, sn, Uw[3], Uv[3], Dinv, u with independent magnitudes"""
    c, s = _cs(q)
    return np.concatenate([[c, s], _vec(rng, 3), _vec(rng, 3), [_scale(rng)], _vec(rng, 1)])


def _finish(rows, rng, again):
    """float32 rows; one more random case where the count is a multiple of 64 (the device build must meet a partial wavefront)"""
    if len(rows) % 64 == 0:
        rows.append(again(rng))
    return np.asarray(rows, np.float64).astype(np.float32)


def _rng(name, kind):
    return np.random.default_rng([sum(name.encode()), KINDS.index(kind), 20240])


# ---------------------------------------------------------------- ops
class Op:
    k = None            # allowed roundings (the issue's table)
    gpu_only = False

    def __init__(self, name):
        self.name = name

    def cases(self, kind):
        raise NotImplementedError

    def ref(self, kind, inp):
        raise NotImplementedError


def _rows(fn, inp, ow):
    """apply fn(row fp64) -> (ref, B[, exact]) to every row"""
    n = inp.shape[0]
    ref, B, ex = np.zeros((n, ow)), np.zeros((n, ow)), np.zeros((n, ow), bool)
    for e in range(n):
        r = fn(inp[e].astype(np.float64))
        ref[e], B[e] = r[0], r[1]
        if len(r) > 2:
            ex[e] = r[2]
    return ref, B, ex


class Rot(Op):
    """rot<AX> / rotT<AX> at T = float (pair=False) or ssf2 (pair=True): R v, R^T v"""
    k = 8

    def __init__(self, name, pair):
        super().__init__(name)
        self.pair = pair

    def cases(self, kind):
        rng, m = _rng(self.name, kind), model(kind)
        rows = []

        def half(ax, q, v):
            c, s = _cs(q)
            return [c, s] + list(v)

        def one(rng, ax, q=None, v=None):
            hs = []
            for _ in range(2 if self.pair else 1):
                hs += half(ax, rng.uniform(-np.pi, np.pi) if q is None else q, _vec(rng, 3) if v is None else v)
            return [ax] + hs
        for ax in range(3):
            rows += [one(rng, ax) for _ in range(N_RANDOM)]
            j = [2, 1, 0][ax]                    # a joint with this axis (abdomen_x, _y, _z), for lo / hi
            rows += [one(rng, ax, q=q) for q in _edge_angles(m, j)]
            rows.append(one(rng, ax, v=np.zeros(3)))
            rows.append(one(rng, ax, v=np.eye(3)[ax] * _scale(rng)))
        return _finish(rows, rng, lambda r: one(r, 0))

    def ref(self, kind, inp):
        def half(ax, h):
            R = rot_cs(ax, h[0], h[1])
            v = h[2:5]
            return np.concatenate([R @ v, R.T @ v]), np.concatenate([np.abs(R) @ np.abs(v), np.abs(R).T @ np.abs(v)])

        def row(x):
            ax = int(x[0])
            hs = [half(ax, x[1 + 5 * h:6 + 5 * h]) for h in range(2 if self.pair else 1)]
            return np.concatenate([h[0] for h in hs]), np.concatenate([h[1] for h in hs])
        return _rows(row, inp, 12 if self.pair else 6)


class JointOp(Op):
    """An op through joint J (pair=False: [J, half]) or through the {leg, arm} pair i (pair=True: [i, leg half, arm half], each half judged
    against the scalar reference of ITS joint).  A half is [c, s, payload]; subclasses give payload, axis_payload, half_ref."""
    joints = list(range(M.NJ))
    has_angle = True
    hw = ow = None            # half widths in / out (without c, s)

    def __init__(self, name, pair):
        super().__init__(name)
        self.pair = pair

    def payload(self, rng):
        raise NotImplementedError

    def axis_payload(self, rng, ax):
        raise NotImplementedError

    def half_ref(self, m, j, c, s, x):
        raise NotImplementedError

    def _half_rows(self, rng, m, j):
        cs_ = _angle_payload_cases(rng, m, j, self.payload, self.axis_payload)
        if not self.has_angle:
            cs_ = cs_[:N_RANDOM] + cs_[-2:]
            return [list(p) for _, p in cs_]
        return [list(_cs(q)) + list(p) for q, p in cs_]

    def cases(self, kind):
        rng, m = _rng(self.name, kind), model(kind)
        rows = []
        if self.pair:
            for i, (jl, ja) in enumerate(PAIR_JOINTS):
                rows += [[i] + a + b for a, b in zip(self._half_rows(rng, m, jl), self._half_rows(rng, m, ja))]
            again = lambda r: [0] + self._half_rows(r, m, 3)[0] + self._half_rows(r, m, 13)[0]
        else:
            for j in self.joints:
                rows += [[j] + a for a in self._half_rows(rng, m, j)]
            again = lambda r: [self.joints[0]] + self._half_rows(r, m, self.joints[0])[0]
        return _finish(rows, rng, again)

    def _split(self, x):
        return (x[0], x[1], x[2:]) if self.has_angle else (1.0, 0.0, x)

    def ref(self, kind, inp):
        m = model(kind)
        hw = self.hw + (2 if self.has_angle else 0)

        def row(x):
            if self.pair:
                js = PAIR_JOINTS[int(x[0])]
                hs = [self.half_ref(m, js[h], *self._split(x[1 + h * hw:1 + (h + 1) * hw])) for h in range(2)]
            else:
                hs = [self.half_ref(m, int(x[0]), *self._split(x[1:1 + hw]))]
            return tuple(np.concatenate([np.broadcast_to(np.asarray(h[k]), h[0].shape) for h in hs]) for k in range(3))
        return _rows(row, inp, self.ow * (2 if self.pair else 1))


def _no_exact(n):
    return np.zeros(n, bool)


class CrossR(JointOp):
    """cross_r<Model, J> / cross_rP<Model, JL, JA>: r x f"""
    k, hw, ow, has_angle = 8, 3, 3, False

    def payload(self, rng):
        return _vec(rng, 3)

    def axis_payload(self, rng, ax):
        return np.eye(3)[ax] * _scale(rng)

    def half_ref(self, m, j, c, s, f):
        S = nd.skew(m["r"][j])
        return S @ f, np.abs(S) @ np.abs(f), _no_exact(3)


class XMotion(JointOp):
    k, hw, ow = 8, 6, 6

    def payload(self, rng):
        return _vec(rng, 6)

    axis_payload = staticmethod(_sv_axis)

    def half_ref(self, m, j, c, s, p):
        X, aX = joint_xform(m, j, c, s)
        return X @ p, aX @ np.abs(p), _no_exact(6)


class XForce(XMotion):
    def half_ref(self, m, j, c, s, f):
        X, aX = joint_xform(m, j, c, s)
        return X.T @ f, aX.T @ np.abs(f), _no_exact(6)


class XInertia(JointOp):
    k, hw, ow = 16, 21, 21

    def payload(self, rng):
        return _abi(rng)

    axis_payload = staticmethod(_abi_axis)

    def half_ref(self, m, j, c, s, a):
        X, aX = joint_xform(m, j, c, s)
        I = abi_to_dense(a)
        return dense_to_abi(X.T @ I @ X), dense_to_abi(aX.T @ np.abs(I) @ aX), _no_exact(21)


class BodyOp(Op):
    """ops indexed by a body: [b, payload] or, for the pair forms, [i, leg payload, arm payload] for the bodies PAIR_BODIES[i]"""
    hw = ow = None

    def __init__(self, name, pair):
        super().__init__(name)
        self.pair = pair

    def payload(self, rng):
        raise NotImplementedError

    def axis_payload(self, rng, ax):
        raise NotImplementedError

    def half_ref(self, m, b, x):
        raise NotImplementedError

    def _half_rows(self, rng, b):
        ax = M.AXIS[b - 1] if b > 0 else 2
        rows = [self.payload(rng) for _ in range(N_RANDOM)]
        rows.append(np.zeros(self.hw))
        rows.append(self.axis_payload(rng, ax))
        return [list(r) for r in rows]

    def cases(self, kind):
        rng = _rng(self.name, kind)
        rows = []
        if self.pair:
            for i, (bl, ba) in enumerate(PAIR_BODIES):
                rows += [[i] + a + b for a, b in zip(self._half_rows(rng, bl), self._half_rows(rng, ba))]
            again = lambda r: [0] + self._half_rows(r, 4)[0] + self._half_rows(r, 14)[0]
        else:
            for b in range(M.NB):
                rows += [[b] + a for a in self._half_rows(rng, b)]
            again = lambda r: [0] + self._half_rows(r, 0)[0]
        return _finish(rows, rng, again)

    def ref(self, kind, inp):
        m = model(kind)

        def row(x):
            if self.pair:
                bs = PAIR_BODIES[int(x[0])]
                hs = [self.half_ref(m, bs[h], x[1 + h * self.hw:1 + (h + 1) * self.hw]) for h in range(2)]
            else:
                hs = [self.half_ref(m, int(x[0]), x[1:1 + self.hw])]
            return tuple(np.concatenate([h[k] for h in hs]) for k in range(2))
        return _rows(row, inp, self.ow * (2 if self.pair else 1))


class AbiBody(BodyOp):
    """abi_body<b> and abi_add_body<b>(I): spatial_inertia(m, b), and I + spatial_inertia(m, b).  k = 2 is RELATIVE TO THE VALUE:
    |got - ref| <= 2 * 2^-24 * |I_b| for the constant alone.  Adding it to a run-time I rounds once more, relative to the sum:
    the bound of that half is 2 * 2^-24 * |I_b| + 2^-24 * |I + I_b|, written as B = |I_b| + |I + I_b| / 2 under the same k."""
    k, hw = 2, 21

    def __init__(self, name, pair):
        super().__init__(name, pair)
        self.ow = 21 if pair else 42

    def payload(self, rng):
        return _abi(rng)

    axis_payload = staticmethod(_abi_axis)

    def half_ref(self, m, b, a):
        Ib = dense_to_abi(nd.spatial_inertia(m, b))
        tot = a + Ib
        added = (tot, np.abs(Ib) + 0.5 * np.abs(tot))
        if self.pair:
            return added
        return np.concatenate([Ib, added[0]]), np.concatenate([np.abs(Ib), added[1]])


class BodyBias(BodyOp):
    """body_bias<b> / body_biasP: crf(v) I_b v"""
    k, hw, ow = 16, 6, 6

    def payload(self, rng):
        return _vec(rng, 6)

    axis_payload = staticmethod(_sv_axis)

    def half_ref(self, m, b, v):
        Ib = nd.spatial_inertia(m, b)
        return nd.crf(v) @ Ib @ v, np.abs(nd.crf(v)) @ np.abs(Ib) @ np.abs(v)


def _rec_fields(r):
    return r[0], r[1], np.concatenate([r[2:5], r[5:8]]), r[8], r[9]        # cs, sn, U = [Uw, Uv], Dinv, u


class Imp(Op):
    """The impulse recursions and pass 3 of the ABA, with the record's cs, sn, Uw, Uv, Dinv, u as given inputs.
    mode: up | down | down_pair | up_pair | down_pair_loaded | aba | abaP.  The *_pair forms carry two COLUMNS through one joint."""
    k = 16

    def __init__(self, name, mode, joints):
        super().__init__(name)
        self.mode, self.joints = mode, joints

    # -- one column / one chain
    @staticmethod
    def up(m, j, rec, p):
        cs, sn, Uv, Dinv, _ = _rec_fields(rec)
        ax = M.AXIS[j]
        X, aX = joint_xform(m, j, cs, sn)
        u = -p[ax]
        du = Dinv * u
        pa, Bpa = p + Uv * du, np.abs(p) + np.abs(Uv) * abs(du)
        return X.T @ pa, aX.T @ Bpa, u

    @staticmethod
    def down(m, j, rec, ul, d0, loaded):
        cs, sn, Uv, Dinv, _ = _rec_fields(rec)
        ax = M.AXIS[j]
        X, aX = joint_xform(m, j, cs, sn)
        d, Bd = X @ d0, aX @ np.abs(d0)
        dot, Bdot = Uv @ d, np.abs(Uv) @ Bd
        dq = Dinv * ((ul if loaded else 0.0) - dot)
        Bdq = abs(Dinv) * ((abs(ul) if loaded else 0.0) + Bdot)
        d[ax] += dq
        Bd[ax] += Bdq
        return d, Bd, dq, Bdq

    @staticmethod
    def aba(m, j, rec, qd, ap, vb):
        cs, sn, Uv, Dinv, u = _rec_fields(rec)
        ax = M.AXIS[j]
        ai, aj = (ax + 1) % 3, (ax + 2) % 3
        X, aX = joint_xform(m, j, cs, sn)
        a, Ba = X @ ap, aX @ np.abs(ap)
        for o in (0, 3):
            a[o + ai] += qd * vb[o + aj]
            a[o + aj] -= qd * vb[o + ai]
            Ba[o + ai] += abs(qd * vb[o + aj])
            Ba[o + aj] += abs(qd * vb[o + ai])
        dot, Bdot = Uv @ a, np.abs(Uv) @ Ba
        qdd, Bq = Dinv * (u - dot), abs(Dinv) * (abs(u) + Bdot)
        a[ax] += qdd
        Ba[ax] += Bq
        return a, Ba, qdd, Bq

    def _chain_payload(self, rng, m, j, q, sv, zero=False):
        """one chain's / column pair's inputs behind the joint number"""
        z = (lambda w: np.zeros(w)) if zero else None
        vec = lambda w: (z(w) if z else _vec(rng, w))
        first = sv if sv is not None else vec(6)
        rec = _rec(rng, q)
        if self.mode == "up":
            return list(rec) + list(first)
        if self.mode == "down":
            return [1.0 if j <= 7 else 0.0] + list(rec) + list(vec(1)) + list(first)
        if self.mode in ("down_pair", "up_pair"):
            return list(rec) + list(first) + list(vec(6))
        if self.mode == "down_pair_loaded":
            return list(rec) + list(vec(2)) + list(first) + list(vec(6))
        return list(rec) + list(vec(1)) + list(first) + list(vec(6))          # aba: rec, qd, aprev, vb

    def _joint_rows(self, rng, m, j):
        rows = [self._chain_payload(rng, m, j, rng.uniform(-np.pi, np.pi), None) for _ in range(N_RANDOM)]
        rows += [self._chain_payload(rng, m, j, q, None) for q in _edge_angles(m, j)]
        rows.append(self._chain_payload(rng, m, j, rng.uniform(-np.pi, np.pi), None, zero=True))
        rows.append(self._chain_payload(rng, m, j, rng.uniform(-np.pi, np.pi), _sv_axis(rng, M.AXIS[j])))
        return rows

    def cases(self, kind):
        rng, m = _rng(self.name, kind), model(kind)
        rows = []
        if self.mode == "abaP":
            for i, (jl, ja) in enumerate(PAIR_JOINTS):
                rows += [[i] + a + b for a, b in zip(self._joint_rows(rng, m, jl), self._joint_rows(rng, m, ja))]
            again = lambda r: [0] + self._joint_rows(r, m, 3)[0] + self._joint_rows(r, m, 13)[0]
        else:
            for j in self.joints:
                rows += [[j] + a for a in self._joint_rows(rng, m, j)]
            again = lambda r: [self.joints[0]] + self._joint_rows(r, m, self.joints[0])[0]
        return _finish(rows, rng, again)

    def ref(self, kind, inp):
        m = model(kind)
        F, T = False, True

        def row(x):
            j = int(x[0])
            if self.mode == "up":
                o, B, u = self.up(m, j, x[1:11], x[11:17])
                return np.append(o, u), np.append(B, abs(u)), [F] * 6 + [T]
            if self.mode == "down":
                d, Bd, dq, Bdq = self.down(m, j, x[2:12], x[12], x[13:19], x[1] != 0)
                return np.append(d, dq), np.append(Bd, Bdq)
            if self.mode in ("down_pair", "down_pair_loaded"):
                ld = self.mode == "down_pair_loaded"
                ul = x[11:13] if ld else [0.0, 0.0]
                p0 = 13 if ld else 11
                cols = [self.down(m, j, x[1:11], ul[c], x[p0 + 6 * c:p0 + 6 * c + 6], ld) for c in range(2)]
                return np.concatenate([c[0] for c in cols]), np.concatenate([c[1] for c in cols])
            if self.mode == "up_pair":
                cols = [self.up(m, j, x[1:11], x[11 + 6 * c:17 + 6 * c]) for c in range(2)]
                us = [c[2] for c in cols]
                return (np.concatenate([cols[0][0], cols[1][0], us]), np.concatenate([cols[0][1], cols[1][1], np.abs(us)]),
                        [F] * 12 + [T] * 2)
            if self.mode == "aba":
                a, Ba, qdd, Bq = self.aba(m, j, x[1:11], x[11], x[12:18], x[18:24])
                return np.append(a, qdd), np.append(Ba, Bq)
            hs = [self.aba(m, PAIR_JOINTS[j][h], x[1 + 23 * h:11 + 23 * h], x[11 + 23 * h], x[12 + 23 * h:18 + 23 * h],
                           x[18 + 23 * h:24 + 23 * h]) for h in range(2)]
            return (np.concatenate([np.append(h[0], h[2]) for h in hs]), np.concatenate([np.append(h[1], h[3]) for h in hs]))
        ow = {"up": 7, "down": 7, "down_pair": 12, "up_pair": 14, "down_pair_loaded": 12, "aba": 7, "abaP": 14}[self.mode]
        return _rows(row, inp, ow)


class QuatRot(Op):
    k = 4

    def cases(self, kind):
        rng = _rng(self.name, kind)
        rows = []
        for _ in range(3 * N_RANDOM):
            q = rng.normal(size=4)
            rows.append(q / np.linalg.norm(q))
        rows += list(np.eye(4)) + list(-np.eye(4))                        # identity and the three half turns
        h = np.sqrt(0.5)
        rows += [[h, h, 0, 0], [h, 0, h, 0], [h, 0, 0, h], [h, -h, 0, 0], [0.5, 0.5, 0.5, 0.5]]
        return _finish(rows, rng, lambda r: [1, 0, 0, 0.5])

    def ref(self, kind, inp):
        def row(q):
            a = np.abs(q)
            w, x, y, z = a
            B = np.array([[1 + 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z + w * y)],
                          [2 * (x * y + w * z), 1 + 2 * (x * x + z * z), 2 * (y * z + w * x)],
                          [2 * (x * z + w * y), 2 * (y * z + w * x), 1 + 2 * (x * x + y * y)]])
            return nd.quat_rot(q).reshape(9), B.reshape(9)
        return _rows(row, inp, 9)


class Exact(Op):
    """ops that only move or negate values: every component bit-exact"""
    k = 0

    def __init__(self, name, iw, fn):
        super().__init__(name)
        self.iw, self.fn = iw, fn

    def cases(self, kind):
        rng = _rng(self.name, kind)
        rows = [_vec(rng, self.iw) for _ in range(3 * N_RANDOM)] + [np.zeros(self.iw)]
        return _finish(rows, rng, lambda r: _vec(r, self.iw))

    def ref(self, kind, inp):
        ref = np.stack([self.fn(x.astype(np.float64)) for x in inp])
        return ref, np.abs(ref), np.ones(ref.shape, bool)


MIRROR = np.array([-1.0, 1.0, -1.0, 1.0, -1.0, 1.0])      # y-mirror of a spatial vector: axial part (-,+,-), polar part (+,-,+)


def mirror_abi(a):
    return dense_to_abi(np.diag(MIRROR) @ abi_to_dense(a) @ np.diag(MIRROR))


OPS = {}
for _o in [
    Rot("rot", False), Rot("rot2", True),
    CrossR("cross_r", False), CrossR("cross_rP", True),
    XMotion("xmotion", False), XMotion("xmotionP", True), XForce("xforce", False), XForce("xforceP", True),
    XInertia("xinertia", False), XInertia("xinertiaP", True),
    AbiBody("abi_body", False), AbiBody("abi_add_bodyP", True),
    BodyBias("body_bias", False), BodyBias("body_biasP", True),
    # the J each helper is instantiated with, from its call sites in ss_dynamics.hpp:
    Imp("imp_up", "up", list(range(8))),                         # solve(): imp_up<7..3>, then <2..0>
    Imp("imp_down", "down", list(range(8)) + [13, 14, 15, 16]),  # solve(): imp_down<0..7, true>, imp_down<13..16, false>
    Imp("imp_down_pair", "down_pair", list(range(8))),           # operator_T: <3..7>; through imp_down_pair_loaded: <0..7>
    Imp("imp_up_pair", "up_pair", list(range(8))),               # operator_up: <7..3>; operator_pair_b: <2..0>
    Imp("imp_down_pair_loaded", "down_pair_loaded", list(range(8))),   # operator_pair_b: <0..2>, then <3..7>
    Imp("aba_acc", "aba", [0, 1, 2, 7]),                         # substep() pass 3, acc_scalar: spine 0..2 and the ankle 7
    Imp("aba_accP", "abaP", None),                               # substep() pass 3: PairJoint<3+i, 13+i>, i = 0..3
    QuatRot("quat_rot"),
    Exact("mirror_sv", 6, lambda x: MIRROR * x),
    Exact("abi_dense", 21, lambda x: abi_to_dense(x).reshape(36)),
    Exact("pack", 54, lambda x: x),                              # sv_pack / sv_half / abi_half: what goes in comes out, per half
]:
    OPS[_o.name] = _o


@functools.lru_cache(maxsize=None)
def prepared(name, kind):
    """(inp, ref, B, exact) of an op: computed once, shared by the host and the device flavour, never modified"""
    op = OPS[name]
    inp = op.cases(kind)
    ref, B, ex = op.ref(kind, inp)
    for a in (inp, ref, B, ex):
        a.setflags(write=False)
    assert inp.shape[0] % 64 != 0
    return inp, ref, B, ex


def judge(got, ref, B, exact, k):
    """-> (worst err / (2^-24 B) over the bounded components, list of failures (case, component, got, ref, ratio))"""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    fails = []
    zero = (B == 0) & ~exact
    bad = zero & (got != 0)
    ex_bad = exact & (got.astype(np.float32) != ref.astype(np.float32))
    pos = (B > 0) & ~exact
    ratio = np.zeros_like(err)
    ratio[pos] = err[pos] / (U * B[pos])
    over = pos & ~(ratio <= k)                  # catches NaN too
    for e, c in zip(*np.nonzero(bad | ex_bad | over | ~np.isfinite(got))):
        fails.append((int(e), int(c), float(got[e, c]), float(ref[e, c]), float(ratio[e, c])))
    return (float(ratio.max()) if pos.any() else 0.0), fails


# ---------------------------------------------------------------- ss_sincos
SINCOS_K = 4          # absolute: |s - sin x|, |c - cos x| <= 4 * 2^-24


def _bits(x):
    return int(np.float32(x).view(np.uint32))


_NA = _bits(3.2) // 7 + 1          # every 7th float in |x| <= 3.2
_NB = _bits(1000.0) // 97 + 1      # every 97th float in |x| <= 1000
SINCOS_GRID = 2 * (_NA + _NB)      # points of the grid (both signs), indexed by sincos_points()


def sincos_points(idx):
    """grid index (int64 array, 0 <= idx < SINCOS_GRID) -> float32 argument"""
    idx = np.asarray(idx, np.int64)
    b = np.where(idx < 2 * _NA, (idx // 2) * 7, ((idx - 2 * _NA) // 2) * 97).astype(np.uint32)
    b |= ((idx & 1).astype(np.uint32) << np.uint32(31))
    return b.view(np.float32)


def sincos_special():
    """multiples of pi/2 in |x| <= 1000, each with its two fp32 neighbours"""
    kmax = int(1000.0 / (np.pi / 2))
    x = (np.arange(-kmax, kmax + 1) * (np.pi / 2)).astype(np.float32)
    return np.concatenate([x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))])


def sincos_worst(x, got):
    """largest |got - (sin, cos)(x)| / 2^-24 and the argument it is at"""
    x64 = x.astype(np.float64)
    e = np.maximum(np.abs(got[:, 0] - np.sin(x64)), np.abs(got[:, 1] - np.cos(x64)))
    e = np.where(np.isfinite(e), e, np.inf)
    i = int(e.argmax())
    return float(e[i] / U), float(x[i])


# ---------------------------------------------------------------- chol6 / chol6_solve_neg
CHOL_K_FACTOR, CHOL_K_SOLVE = 14, 26


def base_inertia_q0(kind):
    """dense 6x6 of the whole robot's inertia about the base at q0 (composite rigid body)"""
    m = model(kind)
    Ic = [nd.spatial_inertia(m, b) for b in range(M.NB)]
    for j in reversed(range(M.NJ)):
        X = nd.xform(M._rot(M.AXIS[j], m["q0"][j]).T, m["r"][j])
        Ic[M.PARENT[j]] = Ic[M.PARENT[j]] + X.T @ Ic[j + 1] @ X
    return Ic[0]


@functools.lru_cache(maxsize=None)
def chol_cases():
    rng = np.random.default_rng(606)
    rows = []
    for _ in range(4 * N_RANDOM):
        G = rng.uniform(-1, 1, (6, 6))
        Mx = 10.0 ** rng.uniform(-2, 2) * (G @ G.T + 10.0 ** rng.uniform(-1.5, 0) * np.eye(6))
        rows.append(np.concatenate([Mx.reshape(36), _vec(rng, 6), _vec(rng, 6)]))
    for kind in KINDS:
        for _ in range(3):
            rows.append(np.concatenate([base_inertia_q0(kind).reshape(36), _vec(rng, 6), _vec(rng, 6)]))
    inp = _finish(rows, rng, lambda r: rows[0])
    inp.setflags(write=False)
    return inp


def _worst_ratio(res, den):
    """max of res / den; a component whose bound is 0 must have a residual of exactly 0"""
    ok = den > 0
    return np.where(ok, res / np.where(ok, den, 1.0), np.where(res == 0, 0.0, np.inf)).max()


def chol_judge(inp, out):
    """-> (worst factor ratio, worst solve ratio, worst pair-vs-scalar ratio, failures)"""
    fails, wf, ws, wp = [], 0.0, 0.0, 0.0
    for e in range(inp.shape[0]):
        Mx = inp[e, :36].astype(np.float64).reshape(6, 6)
        o = out[e].astype(np.float64)
        L = np.zeros((6, 6))
        for i in range(6):
            L[i, i] = 1.0 / o[15 + i]
            for j in range(i):
                L[i, j] = o[i * (i - 1) // 2 + j]
        LLt, aLLt = L @ L.T, np.abs(L) @ np.abs(L).T
        rf = _worst_ratio(np.abs(LLt - Mx), U * aLLt)
        wf = max(wf, rf)
        if not rf <= CHOL_K_FACTOR:
            fails.append((e, "factor", rf))
        xs = {"b0": (o[21:27], 0), "b1": (o[27:33], 1), "pair0": (o[33:39], 0), "pair1": (o[39:45], 1)}
        for name, (x, h) in xs.items():
            b = inp[e, 36 + 6 * h:42 + 6 * h].astype(np.float64)
            r = _worst_ratio(np.abs(b + LLt @ x), U * (aLLt @ np.abs(x)))
            ws = max(ws, r)
            if not r <= CHOL_K_SOLVE:
                fails.append((e, "solve " + name, r))
        for h in range(2):
            xs_, xp = o[21 + 6 * h:27 + 6 * h], o[33 + 6 * h:39 + 6 * h]
            r = _worst_ratio(np.abs(LLt @ (xp - xs_)), U * (aLLt @ np.abs(xs_)))
            wp = max(wp, r)
            if not r <= CHOL_K_SOLVE:
                fails.append((e, "pair half %d vs scalar" % h, r))
    return float(wf), float(ws), float(wp), fails


# ---------------------------------------------------------------- Philox4x32-10, u01
# Random123's published known-answer vectors (kat_vectors: "philox4x32 10"): counter[4], key[2] -> output[4]
PHILOX_KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox_np(c, k):
    """vectorised Philox4x32-10: c [n,4], k [n,2] uint32 -> [n,4] uint32"""
    c = [c[:, i].astype(np.uint64) for i in range(4)]
    k = [k[:, i].astype(np.uint64) for i in range(2)]
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & m32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & m32, (k[1] + np.uint64(0xBB67AE85)) & m32]
    return np.stack(c, 1).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def philox_cases():
    """[n,7] uint32: counter, key, and the word u01 is given.  The known-answer vectors first; u01 gets 0 and 0xFFFFFFFF."""
    rng = np.random.default_rng(10)
    rows = [list(c) + list(k) + [x] for (c, k, _), x in zip(PHILOX_KAT, (0, 0xFFFFFFFF, 0x00000100))]
    rows += [[0] * 6 + [x] for x in (0xFF, 0x100, 0xFFFFFF00, 0xFFFFFEFF, 0x80000000, 1)]
    rows += rng.integers(0, 2 ** 32, (200, 7)).tolist()
    a = np.array(rows, np.uint32)
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------- lane exchange (device only)
@functools.lru_cache(maxsize=None)
def xchg_cases():
    """[n,30] float32 rows (raw bits): f, u32, i, sv6, abi21; every lane distinct; n even (every lane's partner l ^ 1 is a case) and
    not a multiple of 64"""
    rng = np.random.default_rng(77)
    n = 3002
    a = np.zeros((n, 30), np.float32)
    a[:, 0] = rng.permutation(n).astype(np.float32) * 0.37 + 1.0
    u = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    u[::5] = 0xFFFFFFFF                                              # all 32 bits set
    u[1::5] |= 0x7F800000                                            # NaN / inf patterns as floats
    a[:, 1] = u.view(np.float32)
    i = -(np.arange(n, dtype=np.int64) * 7919 + 1)                   # negative, distinct
    i[2::3] = -i[2::3]
    i[0], i[1] = -1, -2 ** 31
    a[:, 2] = i.astype(np.int32).view(np.float32)
    a[:, 3:] = rng.uniform(0.5, 2.0, (n, 27)) * rng.choice([-1.0, 1.0], (n, 27)) * (1 + np.arange(n))[:, None]
    assert n % 2 == 0 and n % 64 != 0
    a.setflags(write=False)
    return a


def xchg_expected(inp):
    """what lane l must hold after the exchange: lane l ^ 1's row, mirrored where the op mirrors (raw bits as uint32 for the three
    scalar words, float32 values for xchg_sv / xchg_abi)"""
    part = inp[np.arange(inp.shape[0]) ^ 1]
    words = part[:, :3].view(np.uint32)
    sv = (part[:, 3:9].astype(np.float64) * MIRROR).astype(np.float32)
    abi = np.stack([mirror_abi(r) for r in part[:, 9:30]]).astype(np.float32)
    return words, sv, abi
