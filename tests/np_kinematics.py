"""fp64 restatement of the kinematic readout (docs/PHYSICS.md "Kinematic readout"; include/steppingstone.h: ss_kinematics), written from
that text.  TEST INFRASTRUCTURE ONLY.  Built on steppingstone_amd.model.build(kind) / model.fk, tests/np_dynamics.py and
tests/np_contact.py -- NOT on the generated ss_model_tables.hpp, so a wrong constant or frame in the kernel code shows here.

readout(m, st) returns, per output group, the fp64 value and its running error bound B:

  * the VALUES evaluate the text's world-frame formulas on the row as it stands (the base rotation is the text's R(quat) of the stored
    quaternion, which an fp32 row holds to unit length within ~1e-7 only);
  * the BOUNDS come from the same pass, which runs on `Tracked` numbers: a value together with the same formula taken over absolute
    values (|a| + |b| for a sum or a difference, |a||b| for a product).  A body's rotation matrix is the exception: its entries
    carry the bound 1 + (number of joints between the body and the torso) -- the base rotation and every joint rotation add an
    absolute error of the order of one rounding of a unit-size number to each entry, and a product of orthogonal matrices does not
    amplify what it inherits (the entrywise |R_parent| |Rot| of the general rule would grow like 2^depth and bound nothing);
  * every value is CROSS-CHECKED against a construction of its own: poses from model.fk, twists from the body-coordinate recursion of
    np_dynamics (v_b = X v_parent + S qd, turned into the world afterwards), COM / momentum from np_dynamics.com_and_momentum, the
    kinetic energy from the 6x6 spatial inertias (v^T I v / 2 in body coordinates).  The two routes are the same function of the state
    only for an orthogonal base rotation, so they must agree to (1e-9 + 8 | |quat|^2 - 1 |) (1 + B) (asserted).
The carrier comes from np_contact.detect.
A float word of the code under test passes when |got - value| <= k * 2^-24 * B (tests/test_kinematics.py fixes k per group)."""
import numpy as np

import np_contact as npc
import np_dynamics as npd
from steppingstone_amd import model as M

U = 2.0 ** -24
G = 9.8                                  # docs/PHYSICS.md 1
KINDS = ["walker3d", "mike"]
GROUPS = ["body_twist", "com", "com_vel", "ang_mom", "kinetic", "potential", "mass", "corner_pos", "corner_vel", "corner_height"]
MARGIN = 1e-5                            # a corner nearer than this to a bound of a contact set is not judged on its carrier
POS, QUAT, VEL, Q, QD, N = slice(0, 3), slice(3, 7), slice(7, 13), slice(13, 34), slice(34, 55), 59


class Tracked:
    """value v and bound b (arrays of one shape): the same formula over absolute values"""

    def __init__(self, v, b=None):
        self.v = np.asarray(v, np.float64)
        self.b = np.abs(self.v) if b is None else np.asarray(b, np.float64)

    @staticmethod
    def of(x):
        return x if isinstance(x, Tracked) else Tracked(x)

    def __add__(self, o):
        o = Tracked.of(o)
        return Tracked(self.v + o.v, self.b + o.b)

    def __sub__(self, o):
        o = Tracked.of(o)
        return Tracked(self.v - o.v, self.b + o.b)

    def __mul__(self, o):
        o = Tracked.of(o)
        return Tracked(self.v * o.v, self.b * o.b)

    __rmul__ = __mul__

    def __matmul__(self, o):
        o = Tracked.of(o)
        return Tracked(self.v @ o.v, self.b @ o.b)

    def __truediv__(self, s):
        return Tracked(self.v / s, self.b / abs(s))

    def __getitem__(self, i):
        return Tracked(self.v[i], self.b[i])

    @property
    def T(self):
        return Tracked(self.v.T, self.b.T)

    def sum(self):
        return Tracked(self.v.sum(), self.b.sum())


def cross(a, b):
    a, b = Tracked.of(a), Tracked.of(b)
    i, j = [1, 2, 0], [2, 0, 1]
    return Tracked(np.cross(a.v, b.v), a.b[i] * b.b[j] + a.b[j] * b.b[i])


def corner_offsets(m):
    """the eight sole corners in their foot frames, c = 4 * foot + corner (PHYSICS.md 2: the left list is the y-mirror)"""
    out = []
    for f in range(2):
        for k in range(4):
            r = np.array(m["corners"][k], np.float64)
            if f == 1:
                r[1] = -r[1]
            out.append(r)
    return out


def world_pass(m, st):
    """The text's formulas, world frame, Tracked: per body pose and twist, then the sums and the corners."""
    R = [None] * M.NB
    p = [None] * M.NB
    w = [None] * M.NB
    v = [None] * M.NB
    R[0] = Tracked(npd.quat_rot(st[QUAT]), np.ones((3, 3)))
    p[0] = Tracked(st[POS])
    w[0] = R[0] @ Tracked(st[VEL][:3])
    v[0] = R[0] @ Tracked(st[VEL][3:])
    for j in range(M.NJ):
        b, par, ax = j + 1, M.PARENT[j], M.AXIS[j]
        d = R[par] @ Tracked(m["r"][j])
        p[b] = p[par] + d
        R[b] = Tracked(R[par].v @ M._rot(ax, st[Q][j]), R[par].b + 1.0)
        v[b] = v[par] + cross(w[par], d)
        w[b] = w[par] + R[par][:, ax] * Tracked(st[QD][j])
    mass = m["mass"]
    tot = float(mass.sum())
    zero = Tracked(np.zeros(3))
    mc, mv = zero, zero
    c, vc = [None] * M.NB, [None] * M.NB
    for b in range(M.NB):
        d = R[b] @ Tracked(m["com"][b])
        c[b] = p[b] + d
        vc[b] = v[b] + cross(w[b], d)
        mc = mc + c[b] * mass[b]
        mv = mv + vc[b] * mass[b]
    com, com_vel = mc / tot, mv / tot
    L, T = zero, Tracked(0.0)
    for b in range(M.NB):
        cl = Tracked(m["com"][b])
        wl = R[b].T @ w[b]
        wxc = cross(wl, cl)
        spin = Tracked(m["inertia_o"][b]) @ wl - cross(cl, wxc) * mass[b]            # I_c w_l
        L = L + cross(c[b] - com, vc[b] * mass[b]) + R[b] @ spin
        T = T + ((vc[b] * vc[b]).sum() * mass[b] + (wl * spin).sum()) * 0.5
    n = int(np.clip(st[N], 0, 19))
    stone = st[65:185].reshape(20, 6)[n]
    nrm = Tracked(npc.stone_normal(stone), np.ones(3))
    cp, cv, ch = [], [], []
    for i, r in enumerate(corner_offsets(m)):
        fb = npc.FEET[i // 4]
        d = R[fb] @ Tracked(r)
        x = p[fb] + d
        cp.append(x)
        cv.append(v[fb] + cross(w[fb], d))
        ch.append(((x - Tracked(stone[:3])) * nrm).sum())
    stack = lambda xs: Tracked(np.stack([x.v for x in xs]), np.stack([x.b for x in xs]))
    twist = stack([Tracked(np.concatenate([w[b].v, v[b].v]), np.concatenate([w[b].b, v[b].b])) for b in range(M.NB)])
    return dict(body_twist=twist, com=com, com_vel=com_vel, ang_mom=L, kinetic=T, potential=com[2] * (tot * G), mass=Tracked(tot),
                corner_pos=stack(cp), corner_vel=stack(cv), corner_height=stack(ch))


def independent_values(m, st):
    """The same quantities by other routes (module docstring)."""
    pos, quat, v0, q, qd = st[POS], st[QUAT], st[VEL], st[Q], st[QD]
    R, p = M.fk(m, q, pos, npd.quat_rot(quat))
    vb = [None] * M.NB
    vb[0] = np.asarray(v0, np.float64)
    for j in range(M.NJ):
        b, par = j + 1, M.PARENT[j]
        S = np.zeros(6)
        S[M.AXIS[j]] = qd[j]
        vb[b] = npd.xform(M._rot(M.AXIS[j], q[j]).T, m["r"][j]) @ vb[par] + S
    twist = np.stack([np.concatenate([R[b] @ vb[b][:3], R[b] @ vb[b][3:]]) for b in range(M.NB)])
    com, P, L = npd.com_and_momentum(m, pos, quat, v0, q, qd)
    tot = float(m["mass"].sum())
    T = sum(0.5 * vb[b] @ npd.spatial_inertia(m, b) @ vb[b] for b in range(M.NB))
    n = int(np.clip(st[N], 0, 19))
    stone = st[65:185].reshape(20, 6)[n]
    nrm = npc.stone_normal(stone)
    cp, cv, ch = [], [], []
    for i, r in enumerate(corner_offsets(m)):
        fb = npc.FEET[i // 4]
        x = p[fb] + R[fb] @ r
        cp.append(x)
        cv.append(R[fb] @ (vb[fb][3:] + np.cross(vb[fb][:3], r)))
        ch.append(float((x - stone[:3]) @ nrm))
    return dict(body_twist=twist, com=com, com_vel=P / tot, ang_mom=L, kinetic=T, potential=tot * G * com[2], mass=tot,
                corner_pos=np.stack(cp), corner_vel=np.stack(cv), corner_height=np.array(ch))


def carriers(m, st):
    """(carrier [8] int: slot 0 / 1 / 2 of the carrying stone or -1, judged [8] bool: the corner is farther than MARGIN from every bound of
    every active stone's contact set and, where two stones hold it, from their tie) from np_contact.detect and the text of 3.3."""
    n = int(st[N])
    terrain = st[65:185].reshape(20, 6)
    hits = npc.detect(m, st[POS], st[QUAT], st[Q], terrain, n)
    car = np.array([-1 if h is None else h["stone"] - n + 1 for h in hits], np.int32)
    R, p = M.fk(m, st[Q], st[POS], npd.quat_rot(st[QUAT]))
    idx = [max(n - 1, 0), n, min(n + 1, 19)]
    judged = np.ones(8, bool)
    for i, r in enumerate(corner_offsets(m)):
        x = p[npc.FEET[i // 4]] + R[npc.FEET[i // 4]] @ r
        depth = []
        for si in idx:
            s = terrain[si]
            nrm = npc.stone_normal(s)
            d = float((x - s[:3]) @ nrm)
            l = (x - s[:3]) - d * nrm
            u = l[0] * np.cos(s[3]) + l[1] * np.sin(s[3])
            v = l[1] * np.cos(s[3]) - l[0] * np.sin(s[3])
            gaps = [abs(d), abs(d + npc.REACH), abs(abs(u) - npc.PLANK_A), abs(abs(v) - npc.PLANK_B)]
            if min(gaps) <= MARGIN:
                judged[i] = False
            if -npc.REACH < d < 0 and abs(u) < npc.PLANK_A and abs(v) < npc.PLANK_B:
                depth.append(d)
        for a in range(len(depth)):
            for b in range(a + 1, len(depth)):
                if abs(depth[a] - depth[b]) <= MARGIN:
                    judged[i] = False
    return car, judged


def foot_flags(car):
    """the contact flags as np_env.control_step forms them from a detection: bit 0 right, bit 1 left, set by any carried corner"""
    return int((car[:4] >= 0).any()) | (int((car[4:] >= 0).any()) << 1)


def readout(m, st):
    """st: packed state row [186] (any float type) -> {group: (value, B)} in fp64, plus "carrier": (carrier, judged)."""
    st = np.asarray(st, np.float64)
    tr = world_pass(m, st)
    iv = independent_values(m, st)
    tol = 1e-9 + 8.0 * abs(float(st[QUAT] @ st[QUAT]) - 1.0)
    out = {}
    for g in GROUPS:
        val = np.asarray(iv[g], np.float64)
        assert np.all(np.abs(tr[g].v - val) <= tol * (1.0 + tr[g].b)), "the two fp64 routes disagree on %s" % g
        out[g] = (tr[g].v, tr[g].b)
    out["carrier"] = carriers(m, st)
    return out


def split_outputs(o):
    """the three output arrays of ss_kinematics ([n,22,6], [n,12], [n,8,8]; any missing) -> {group: array}, carrier as int32"""
    out = {}
    if "body_twist" in o:
        out["body_twist"] = o["body_twist"]
    if "summary" in o:
        s = o["summary"]
        out.update(com=s[:, 0:3], com_vel=s[:, 3:6], ang_mom=s[:, 6:9], kinetic=s[:, 9], potential=s[:, 10], mass=s[:, 11])
    if "corners" in o:
        c = o["corners"]
        out.update(corner_pos=c[:, :, 0:3], corner_vel=c[:, :, 3:6], corner_height=c[:, :, 6], corner_carrier=c[:, :, 7].astype(np.int32))
    return out


def worst_ratios(got, refs):
    """got: split_outputs of n rows; refs: the n readout() dicts -> {group: max |got - value| / (2^-24 B)}; a word whose B is 0 must be
    exactly 0 (ratio inf otherwise)."""
    worst = {}
    for g in GROUPS:
        if g not in got:
            continue
        w = 0.0
        for e, r in enumerate(refs):
            val, B = r[g]
            err = np.abs(np.asarray(got[g][e], np.float64) - val)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(B > 0, err / (U * np.where(B > 0, B, 1.0)), np.where(err > 0, np.inf, 0.0))
            w = max(w, float(np.max(ratio)))
        worst[g] = w
    return worst
