"""The reference's SHIPPED actors as the anchor of the policy-facing joint conventions.

The env's source is absent from the reference, but `playground/models/*.pt` were trained IN it, with
`get_mirror_function(env.unwrapped.get_mirror_indices())` (`playground/train.py:160-161`, `common/envs_utils.py:687-740`), so a
shipped actor satisfies  pi(M_o o) ~ M_a pi(o)  for the reference env's TRUE index lists and for no other signed permutation.
`ss_get_mirror_indices` must be those lists: measured here on observations of this repository's env (CPU oracle), for both robots.
The actors' weights are the plain arrays under tests/golden/ (shipped_actor_<kind>.npz, read from those files with the restricted
unpickler by tools/make_golden_policy.py; no reference code runs).
Informational about the ENV's physics (the policies still fall in it: different robot model) -- a pin of the LAYOUT only."""
import os

import numpy as np
import pytest

import oracle_lib as ol
import shipped_actor
from steppingstone_amd import _lib, model

torch = pytest.importorskip("torch")

FILES = [("walker3d", "mocca_envs:Walker3DStepperEnv-v0_latest.pt"), ("mike", "mocca_envs:MikeStepperEnv-v0_latest.pt")]


def _shipped_actor(kind, fname):
    """the deterministic actor of the shipped policy `fname`, from its weights stored under tests/golden/"""
    w = np.load(os.path.join(shipped_actor.GOLD, "shipped_actor_%s.npz" % kind))
    assert str(w["source"]) == fname
    return shipped_actor.load_actor(kind)


def _observations(kind, actor, n=128, steps=24):
    """observations of OUR env (policy coordinates): half under random actions, half under the shipped actor itself"""
    out = []
    for use_policy in (False, True):
        o = ol.OracleEnv(kind, n, seed=5)
        o.set_curriculum(3)
        obs = o.reset()
        for t in range(steps):
            if use_policy:
                with torch.no_grad():
                    a = actor(torch.from_numpy(obs)).numpy()
            else:
                a = o.random_actions(t)
            obs, _, _, _ = o.step(a.astype(np.float32))
            if t % 2 == 1:
                out.append(obs.copy())
        o.close()
    return np.concatenate(out).astype(np.float32)


def _mirror(v, neg, right, left):
    m = v.copy()
    m[:, neg] *= -1
    out = m.copy()
    out[:, right], out[:, left] = m[:, left], m[:, right]
    return out


def _error(actor, O, idx):
    neg_o, right_o, left_o, neg_a, right_a, left_a = idx
    with torch.no_grad():
        a = actor(torch.from_numpy(O)).numpy()
        am = actor(torch.from_numpy(np.ascontiguousarray(_mirror(O, neg_o, right_o, left_o)))).numpy()
    return float(np.abs(am - _mirror(a, neg_a, right_a, left_a)).mean()), float(np.abs(a).mean())


@pytest.mark.parametrize("kind,fname", FILES)
def test_shipped_actor_is_equivariant_under_ss_get_mirror_indices(kind, fname):
    actor = _shipped_actor(kind, fname)
    O = _observations(kind, actor)
    idx = [np.asarray(i, np.int64) for i in _lib.mirror_indices()]
    err, mean_a = _error(actor, O, idx)
    # 1. the lists are (to the accuracy a trained net is symmetric at all) a symmetry of the shipped actor ...
    assert err < 0.25 * mean_a, (err, mean_a)
    # 2. ... every single one of the 42 joint sign bits of the observation, the 21 of the action and the 18 others is confirmed:
    #    negating one more entry (a swapped pair keeps a common bit) makes the actor LESS symmetric
    pair = {}
    for r, l in zip(idx[1], idx[2]):
        pair[int(r)], pair[int(l)] = int(l), int(r)
    worst = np.inf
    for i in range(60):
        if i in pair and pair[i] < i:
            continue
        tog = set(int(x) for x in idx[0]) ^ ({i, pair[i]} if i in pair else {i})
        e2, _ = _error(actor, O, [np.array(sorted(tog), np.int64)] + idx[1:])
        worst = min(worst, e2 - err)
    apair = dict(zip(idx[4].tolist(), idx[5].tolist()))
    for j in range(21):
        if j in apair.values():
            continue
        tog = set(int(x) for x in idx[3]) ^ ({j, apair[j]} if j in apair else {j})
        e2, _ = _error(actor, O, idx[:3] + [np.array(sorted(tog), np.int64)] + idx[4:])
        worst = min(worst, e2 - err)
    assert worst > -1e-3, "toggling one sign bit makes the shipped actor MORE symmetric by %.4f" % -worst
    # 3. the alternative this repository used up to round 3 -- left limbs' x / z joints about the +axis, hence negated by the
    #    mirror -- is rejected by the same actor (it scores like random sign sets)
    xz = [j for j in range(3, 21) if model.AXIS[j] != 1]
    old_neg_o = sorted(set(idx[0].tolist()) | {6 + j for j in xz} | {27 + j for j in xz})
    old_neg_a = sorted(set(idx[3].tolist()) | set(xz))
    err_old, _ = _error(actor, O, [np.array(old_neg_o), idx[1], idx[2], np.array(old_neg_a), idx[4], idx[5]])
    print("%s: shipped actor's mirror-equivariance error %.3f under ss_get_mirror_indices (mean |a| %.3f), %.3f with the left limbs' "
          "x / z joints negated; smallest change from one toggled sign bit %+.4f" % (kind, err, mean_a, err_old, worst))
    assert err_old > 3.0 * err


@pytest.mark.parametrize("kind,fname", FILES)
def test_shipped_actor_couples_action_j_to_inputs_6_plus_j_and_27_plus_j(kind, fname):
    """The observation layout 6 base | 21 joint angles | 21 joint rates | 2 contacts | 10 target (SURVEY 9, M-H confidence; PHYSICS.md 5)
    against the shipped actor's mean Jacobian: a trained controller couples action j most strongly to ITS joint's rate and angle, so
    of all 21-wide windows of the 60 inputs the 21 x 21 block at offset 27 (rates) must be the most diagonal-dominant, offset 6
    (angles) the second, and d a_j / d rate_j negative (damping: action and rate share the sign convention per joint)."""
    actor = _shipped_actor(kind, fname)
    O = torch.from_numpy(_observations(kind, actor, n=64)).requires_grad_(True)
    J = np.zeros((21, 60))
    for j in range(21):
        g, = torch.autograd.grad(actor(O)[:, j].sum(), O)
        J[j] = g.mean(0).numpy()
    ratio = sorted(((float(np.abs(np.diag(J[:, off:off + 21])).mean() / np.abs(J[:, off:off + 21]).mean()), off) for off in range(0, 40)), reverse=True)
    print("%s: diagonal dominance by window offset: %s" % (kind, ", ".join("%d: %.2f" % (o, r) for r, o in ratio[:4])))
    assert [o for _, o in ratio[:2]] == [27, 6] and ratio[0][0] > 3.0 and ratio[1][0] > 2.0 and ratio[2][0] < 1.6
    d_rate = np.diag(J[:, 27:48])
    live = np.abs(d_rate) > 0.02           # (Mike's three abdomen actions do not respond to anything: dead outputs in that file)
    assert live.sum() >= 14 and (d_rate[live] < 0).all()


def test_policy_sign_is_what_the_lists_assume():
    """sigma is ONE physical convention per joint type: equal on both sides for y joints, opposite for x / z joints (the left one is
    measured about the mirrored axis), +1 on the spine; the negated list holds only the spine's z / x joints; every limb joint is
    swapped with its twin (same joint type): together 'the policy sees a mirror-symmetric robot whose left axes are mirrored'."""
    neg_o, right_o, left_o, neg_a, right_a, left_a = [list(map(int, i)) for i in _lib.mirror_indices()]
    assert neg_a == [0, 2] and sorted(neg_o) == [2, 4, 6, 8, 27, 29, 50, 53, 55, 58]
    for r, l in zip(right_a, left_a):
        assert model.JOINT_NAMES[r].replace("right_", "") == model.JOINT_NAMES[l].replace("left_", "")
        assert model.AXIS[r] == model.AXIS[l]
        assert model.POLICY_SIGN[l] == model.POLICY_SIGN[r] * (1 if model.AXIS[l] == 1 else -1)
    assert model.POLICY_SIGN[:3] == [1, 1, 1]
    assert [model.JOINT_NAMES[j] for j in range(21) if model.POLICY_SIGN[j] * (1 if model.AXIS[j] == 1 or "right" in model.JOINT_NAMES[j] or j < 3 else -1) < 0] \
        == ["right_knee", "left_knee"]            # the one joint TYPE measured against the link frame's +axis


def _survival(kind, actor, sign_types, n=128, steps=200):
    """mean episode length (control steps) of the deterministic shipped actor in OUR env (flat terrain, CPU oracle) with the sign
    convention of the listed joint types flipped between env and policy (observation angle + rate, action)"""
    sj = np.ones(21, np.float32)
    for j, name in enumerate(model.JOINT_NAMES):
        if name.replace("right_", "").replace("left_", "") in sign_types:
            sj[j] = -1
    so = np.ones(60, np.float32)
    so[6:27], so[27:48] = sj, sj
    o = ol.OracleEnv(kind, n, seed=9)
    o.set_curriculum(0)
    obs = o.reset()
    lens = []
    for t in range(steps):
        with torch.no_grad():
            a = actor(torch.from_numpy(np.ascontiguousarray(obs * so))).numpy() * sj
        obs, _, d, info = o.step(a.astype(np.float32))
        lens += [float(info["ep_len"][i]) for i in np.nonzero(d)[0]]
    lens += o.get_state()[:, ol.S_ELAPSED].tolist()         # episodes still running count with their current length
    o.close()
    return float(np.mean(lens))


@pytest.mark.parametrize("kind,fname", FILES)
def test_shipped_actor_rejects_the_other_knee_convention(kind, fname):
    """The knee is the one joint type whose sign the shipped policies pin through BEHAVIOUR (per-type signs commute with the mirror, so
    the equivariance test cannot see them): in policy coordinates (knee negative in flexion, POLICY_SIGN = -1) the deterministic
    Walker3D / Mike actors stay up 81 / 58 control steps in our env, with the knee convention flipped back 25 / 10 -- and a control
    flip of a joint type that is right as it is (hip y) makes things worse, not better.  They still fall (the robot model is our own):
    a pin of the CONVENTION, not a parity statement."""
    actor = _shipped_actor(kind, fname)
    ours, knee_back, hip_y = _survival(kind, actor, ()), _survival(kind, actor, ("knee",)), _survival(kind, actor, ("hip_y",))
    print("%s: shipped actor survives %.1f control steps in policy coordinates, %.1f with the knee sign flipped back, %.1f with hip y "
          "flipped" % (kind, ours, knee_back, hip_y))
    assert ours > 2.0 * knee_back and ours > 1.3 * hip_y and ours > 40
