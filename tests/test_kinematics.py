"""The kinematic readout's code (steppingstone_amd/csrc/ss_kinematics.hpp, compiled for the CPU by tests/kinematics_host_lib.py) against
the fp64 restatement of docs/PHYSICS.md 9 (tests/np_kinematics.py) on the rows of tests/kinematics_cases.py: about 200 states per robot
-- oracle reset states, oracle states after 30 random control steps at curricula 0 and 5, hand-made rows (tilted torso, joints at both
range ends, large rates, corners carried by every stone slot).  Floats: |host - fp64| <= K * 2^-24 * B per output word, K = 4 x the worst
ratio measured on this sample (kinematics_cases.K); the carrier: equal to np_contact.detect's decision wherever the corner is farther
than 1e-5 m from every bound of every active stone's contact set.  The reference is always the restatement, never the kernel."""
import numpy as np
import pytest

import kinematics_cases as kc
import kinematics_host_lib as kh
import np_contact as npc
import np_dynamics as npd
import np_env
import np_kinematics as nk
import render_host_lib as rh
from steppingstone_amd import model as M

pytestmark = pytest.mark.skipif(not rh.hipcc(), reason="needs hipcc")
KINDS = kc.KINDS


@pytest.fixture(scope="module", params=KINDS)
def case(request):
    kind = request.param
    st = kc.sample(kind)
    return kind, st, kc.references(kind), nk.split_outputs(kh.kinematics(KINDS.index(kind), st))


def test_floats_within_their_rounding_bounds(case):
    kind, st, refs, got = case
    assert st.shape[0] >= 200
    worst = nk.worst_ratios(got, refs)
    print("kinematics host %s: n=%d worst err/(2^-24 B) per group: %s" % (kind, st.shape[0], {g: round(w, 4) for g, w in worst.items()}))
    over = {g: (w, kc.K[g]) for g, w in worst.items() if not w <= kc.K[g]}
    assert set(worst) == set(nk.GROUPS) and not over, "%s: groups outside their K: %s" % (kind, over)


def test_carrier_is_the_specified_decision(case):
    kind, st, refs, got = case
    car = np.array([r["carrier"][0] for r in refs])
    judged = np.array([r["carrier"][1] for r in refs])
    left_out = 1.0 - judged.mean()
    print("kinematics host %s: %d of %d corners within 1e-5 m of a bound; carried by slot 0 / 1 / 2: %s" % (
        kind, (~judged).sum(), judged.size, [(car == s).sum() for s in range(3)]))
    assert left_out <= 0.02
    assert all((car[judged] == s).sum() >= 8 for s in (-1, 0, 1, 2)), "the sample must exercise every carrier value"
    bad = np.argwhere((got["corner_carrier"] != car) & judged)
    assert bad.size == 0, "%s: (row, corner) %s: host %s, specification %s" % (
        kind, bad[:6].tolist(), got["corner_carrier"][tuple(bad[:6].T)], car[tuple(bad[:6].T)])
    assert np.isin(got["corner_carrier"], (-1, 0, 1, 2)).all()


@pytest.mark.parametrize("kind", KINDS)
def test_exact_ties_follow_the_tie_rule(kind):
    rows, slot = kc.tie_rows(kind)
    got = nk.split_outputs(kh.kinematics(KINDS.index(kind), rows))["corner_carrier"]
    m = kc.model(kind)
    for r, s, g in zip(rows, slot, got):
        spec, _ = nk.carriers(m, r.astype(np.float64))
        held = spec >= 0
        assert held.sum() >= 4 and (spec[held] == s).all(), "the hand-made row must tie as constructed: %s" % spec
        assert (g == spec).all(), "%s: host %s, tie rule %s" % (kind, g, spec)


def test_corner_positions_are_body_poses_times_corners(case):
    """corner_pos against the pinned ss_body_poses host code: x = p_foot + R_foot r_k, evaluated in fp64 from its fp32 poses; the readout
    forms the same sum in fp32 (at most 3 roundings of terms bounded by |p| + |R||r|, the table constant counts one more: 4)."""
    kind, st, refs, got = case
    poses = rh.body_poses(KINDS.index(kind), st).astype(np.float64)
    m = kc.model(kind)
    for i, r in enumerate(nk.corner_offsets(m)):
        T = poses[:, (8, 13)[i // 4]]
        p, R = T[:, :3], T[:, 3:].reshape(-1, 3, 3)
        want, B = p + R @ r, np.abs(p) + np.abs(R) @ np.abs(r)
        assert (np.abs(got["corner_pos"][:, i] - want) <= 4 * nk.U * B).all()


def test_contact_flags_agree_with_np_env(case):
    """np_env.control_step reports the contact flags of its LAST substep's detection, i.e. of the state three substeps into the control
    step (PHYSICS.md 4.2).  The same three substeps are taken here with np_contact.substep under the same torques, and the readout of
    that state (host code, the row rounded to fp32) must say 'a stone carries a corner of the foot' for exactly the feet np_env flags
    -- on rows where no corner of that state is within the margin.  Rows: the robot standing into a stone, zero action."""
    kind, st, refs, got = case
    m = kc.model(kind)
    rows = st[-30:-6][::3].astype(np.float64)                   # 8 of the 'standing into stone n-1 / n / n+1' rows
    act = np.zeros(21)
    judged_rows, flagged = 0, 0
    for r in rows:
        out = np_env.control_step(m, r, act)
        s3, warm = r.copy(), None
        for _ in range(3):
            sub = npc.substep(m, s3, np.zeros(21), warm=warm)
            warm = sub["warm"]
            s3[:55] = sub["state"]
        s3 = s3.astype(np.float32)
        spec, judged = nk.carriers(m, s3.astype(np.float64))
        if not judged.all():
            continue
        judged_rows += 1
        car = nk.split_outputs(kh.kinematics(KINDS.index(kind), s3[None]))["corner_carrier"][0]
        assert nk.foot_flags(car) == out["flags"], "%s: readout carriers %s, np_env flags %d" % (kind, car, out["flags"])
        flagged += out["flags"] != 0
    assert judged_rows >= 6 and flagged >= 3, (judged_rows, flagged)


def test_total_mass(case):
    kind, st, refs, got = case
    tot = kc.model(kind)["mass"].sum()
    assert (got["mass"] == got["mass"][0]).all()
    assert abs(float(got["mass"][0]) - tot) <= kc.K["mass"] * nk.U * tot


def test_rigid_rows_move_as_one_body(case):
    """All joint rates zero, a pure torso twist: every body's twist is the rigid field of that twist, and the angular momentum and the
    kinetic energy are those of the composite rigid body -- of the restatement to fp64 accuracy, of the host code within its bounds."""
    kind, st, refs, got = case
    m = kc.model(kind)
    rows = range(st.shape[0])[kc.RIGID]
    for e in rows:
        s = st[e].astype(np.float64)
        assert (s[nk.QD] == 0).all()
        R0 = npd.quat_rot(s[nk.QUAT])
        w0, v0 = R0 @ s[nk.VEL][:3], R0 @ s[nk.VEL][3:]
        R, p = M.fk(m, s[nk.Q], s[nk.POS], R0)
        field = np.stack([np.concatenate([w0, v0 + np.cross(w0, p[b] - p[0])]) for b in range(M.NB)])
        com = sum(m["mass"][b] * (p[b] + R[b] @ m["com"][b]) for b in range(M.NB)) / m["mass"].sum()
        I = np.zeros((3, 3))
        for b in range(M.NB):
            c = m["com"][b]
            Ic = m["inertia_o"][b] - m["mass"][b] * (c @ c * np.eye(3) - np.outer(c, c))
            d = p[b] + R[b] @ c - com
            I += R[b] @ Ic @ R[b].T + m["mass"][b] * (d @ d * np.eye(3) - np.outer(d, d))
        vcom = v0 + np.cross(w0, com - p[0])
        L, T = I @ w0, 0.5 * m["mass"].sum() * vcom @ vcom + 0.5 * w0 @ I @ w0
        ortho = 1e-9 + 8.0 * abs(s[nk.QUAT] @ s[nk.QUAT] - 1.0)       # the two are one function only for an orthogonal base rotation
        for g, want in (("body_twist", field), ("ang_mom", L), ("kinetic", T)):
            val, B = refs[e][g]
            assert (np.abs(val - want) <= ortho * (1.0 + B)).all(), g
            assert (np.abs(got[g][e] - want) <= (kc.K[g] * nk.U + ortho) * (1.0 + B)).all(), g
