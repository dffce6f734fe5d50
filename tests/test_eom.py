"""The equation-of-motion readout's code (steppingstone_amd/csrc/ss_eom.hpp, compiled for the CPU by tests/eom_host_lib.py) against the
fp64 restatement of docs/PHYSICS.md 11 (tests/np_eom.py) on the rows of tests/kinematics_cases.py (about 200 states per robot), against
the pinned kinematic readout, and closed against one substep of the step code (the CPU build of ss_forces.hpp).  Floats:
|host - fp64| <= K * 2^-24 * B per output word (eom_cases.K).  The reference is always the restatement, never the kernel."""
import numpy as np
import pytest

import eom_cases as ec
import eom_host_lib as eh
import forces_cases as fc
import forces_host_lib as fh
import kinematics_cases as kc
import kinematics_host_lib as kh
import np_dynamics as npd
import np_eom as ne
import np_kinematics as nk
import render_host_lib as rh

pytestmark = pytest.mark.skipif(not rh.hipcc(), reason="needs hipcc")
KINDS = ec.KINDS
U = ne.U


@pytest.fixture(scope="module", params=KINDS)
def case(request):
    kind = request.param
    st = ec.sample(kind)
    return kind, st, ec.references(kind), ne.split_outputs(eh.eom(KINDS.index(kind), st))


def test_floats_within_their_rounding_bounds(case):
    kind, st, refs, got = case
    assert st.shape[0] >= 200
    beyond = ec.beyond_limit(kind, st[:, 13:34].astype(np.float64))
    moving = beyond & (st[:, 34:55] != 0)
    assert beyond.sum() >= 32 and moving.sum() >= 32, "passive must exercise kl and dl"
    over, worst = ec.outside(got, refs)
    print("eom host %s: n=%d (%d joints beyond a limit) worst err/(2^-24 B) per group: %s" % (
        kind, st.shape[0], beyond.sum(), {g: float("%.4g" % w) for g, w in worst.items()}))
    assert set(worst) == set(ne.GROUPS) and not over, "%s: groups outside their K: %s" % (kind, over)


def test_translation_invariance(case):
    """the rows 15 m out: B holds no |p|, so the same K must hold; here the readout does not read the position at all"""
    kind, st, refs, got = case
    far = ec.shifted(st)
    m = ec.model(kind)
    refs_far = [ne.readout(m, s) for s in far[::8]]
    for a, b in zip(refs_far, refs[::8]):
        for g in ne.GROUPS:
            assert np.array_equal(a[g][1], b[g][1]), "B must not depend on the position"
    moved = ne.split_outputs(eh.eom(KINDS.index(kind), far))
    over, worst = ec.outside(moved, refs)
    print("eom host %s, moved by %s: worst err/(2^-24 B): %s" % (kind, ec.SHIFT.tolist(), {g: float("%.4g" % w) for g, w in worst.items()}))
    assert not over, "%s: groups outside their K after the shift: %s" % (kind, over)


def test_structure(case):
    kind, st, refs, got = case
    m = ec.model(kind)
    Mm = got["mass"]
    assert np.array_equal(Mm, Mm.transpose(0, 2, 1)), "mass == mass^T bit for bit"
    tot = float(m["mass"].sum())
    BM = ec.stack(refs, "mass", 1)
    assert (np.abs(Mm[:, 3:6, 3:6].astype(np.float64) - tot * np.eye(3)) <= ec.K["mass"] * U * BM[:, 3:6, 3:6]).all()
    for e in range(Mm.shape[0]):
        np.linalg.cholesky(Mm[e].astype(np.float64))                # raises unless every pivot is positive
    assert (got["passive"][:, :6] == 0).all()
    R = np.stack([npd.quat_rot(s[3:7].astype(np.float64)) for s in st])
    J = got["corner_jac"].astype(np.float64)
    assert (np.abs(J[:, :, :, 3:6] - R[:, None]) <= ec.K["corner_jac"] * U).all(), "the base's linear columns are the torso rotation"
    gb = np.einsum("nia,a->ni", R.transpose(0, 2, 1), np.array([0.0, 0.0, -ne.G]))          # R^T g
    want = np.einsum("nki,ni->nk", Mm[:, :, 3:6].astype(np.float64), gb)
    tol = ec.K["gravity"] * U * ec.stack(refs, "gravity", 1) + ec.K["mass"] * U * np.einsum("nki,ni->nk", BM[:, :, 3:6], np.abs(gb))
    assert (np.abs(got["gravity"] - want) <= tol).all(), "gravity == mass[:, 3:6] R^T g"


def test_agrees_with_the_kinematic_readout(case):
    kind, st, refs, got = case
    kin = nk.split_outputs(kh.kinematics(KINDS.index(kind), st))
    d = ec.judge_against_kinematics(kind, st, got, kin, refs, kc.references(kind))
    print("eom host %s: largest |T(mass) - kinetic| %.3g J" % (kind, d))


@pytest.mark.parametrize("kind", KINDS)
def test_closes_against_the_substep(kind):
    c = fc.cases(kind)
    ki = KINDS.index(kind)
    step = fh.step_forces(ki, c["st"], c["act"], next_state=False)
    got = ne.split_outputs(eh.eom(ki, c["st"]))
    ec.judge_closing(kind, c["st"], step, got, "eom host")
