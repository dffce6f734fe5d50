"""The three-helper K-step kernel hands the tail of every substep behind the base's velocity change dv0 to two helper wavefronts
(ss_dynamics.hpp: limb_tail_offload(); ss_kernels.hpp: rollout_kernel_helped): helper 1 sweeps down the arms and integrates the arm
joints, helper 2 integrates the base, behind a sixth barrier (#3r) that every wavefront meets whether or not any of its lanes is in
contact; one more barrier stands in front of the control step's epilogue.  Same functions, same expressions: nothing may move.  The plain
kernel (SS_HELPERS=0), which has no helper and keeps the tail inline, is the reference.  At 33 and 97 envs -- the last workgroup holds one
real env and 31 padding pairs --, both robots (Walker3D at curriculum 0, Mike at curriculum 5), 63 control steps under the benchmark's
Philox actions with auto-reset on,

  * SS_HELPERS = 3 as three 21-step launches and as nine 7-step launches

give obs, rew, done, info and the full state of SS_HELPERS = 0 as 63 single launches, bit for bit (compared as 32-bit words: a zero of
the other sign is a difference).

Events are seeded through the packed state before the run: the step limits and target advances of tests/test_gpu_reset_pose_bits.py
(its SEEDED table, minus the last env), more step limits at the 21-step launches' borders (LIMITS below), and the last env -- alone in
its workgroup -- lifted by LIFT metres, so that its wavefront falls freely, has no lane in contact, skips the contact solve and still has
to meet barrier #3r and hand over a dv0 of zeros.  The test asserts ON THE REFERENCE RUN ALONE, from done, info and the contact flags of
the state per step, that each class occurred:

  (w) a workgroup none of whose envs reports a foot contact in a step (and none of them reset in it)      >= 3 workgroup-steps
  (o) an env with exactly one foot in contact in a step                                                   >= 3 env-steps
  (a) a reset in the first step of a 7-step launch, (a21) of a 21-step launch                            >= 3, >= 1 env-steps
  (b) a reset in the last step of a 7-step launch, (b21) of a 21-step launch                             >= 3, >= 1 env-steps
  (c) target advance and reset in the same step                                                           >= 3 env-steps

(printed by the test: run it with -s)."""
import os

import pytest

import oracle_lib as ol
from test_gpu_reset_pose_bits import LIMIT, SEEDED, same

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

STEPS = 63
SEED = 0
CASES = [("Walker3DStepperEnv-v0", 0), ("MikeStepperEnv-v0", 5)]
LIFT = 0.5                   # metres: about 19 control steps of free fall
# env -> the step in which it reaches the step limit: the last and the first steps of the 21-step launches (20 | 21 and 41 | 42 are the
# last and the first step of a 7-step launch as well)
LIMITS = {}
for _j, _ids in ((20, (33, 34, 35, 36)), (21, (37, 38, 39, 40)), (41, (41, 42, 43, 44)), (42, (45, 46, 47, 48))):
    for _i in _ids:
        LIMITS[_i] = _j


def seed_events(e, n):
    st = e.get_state().clone()
    for i, (over, count, elapsed) in SEEDED.items():
        if i == n - 1:
            continue
        if over:
            st[i, 0] = st[i, 65 + 6]              # x of stone 1, the target of a fresh episode
        st[i, ol.S_COUNT] = float(count)
        st[i, ol.S_ELAPSED] = float(elapsed)
    for i, j in LIMITS.items():
        if i < n - 1:
            st[i, ol.S_ELAPSED] = float(LIMIT - 1 - j)
    st[n - 1, 2] += LIFT                          # the lone env of the last workgroup
    e.set_state(st)


def run(env_id, curriculum, n, helpers, spl):
    """-> (obs, rew, done, info, state) after STEPS control steps; with spl == 1 also done, info.update_terrain and the contact flags of
    every step ([STEPS, n] each; None otherwise: a K-step launch shows only its last step)"""
    from steppingstone_amd.envs import SteppingStoneVecEnv
    old = os.environ.get("SS_HELPERS")
    try:
        os.environ["SS_HELPERS"] = helpers
        e = SteppingStoneVecEnv(env_id, n, seed=SEED, device="cuda:0", return_numpy=False)
        e.update_curriculum(curriculum)
        e.reset()
        seed_events(e, n)
        trace = None
        if spl == 1:
            trace = [[], [], []]
            for t in range(STEPS):
                e.rollout_random(1, t0=t, steps_per_launch=1)
                trace[0].append(e._done.bool().clone())
                trace[1].append(e._info[:, 4].bool().clone())
                trace[2].append(e.get_state()[:, ol.S_FLAGS].to(torch.int32).clone())
            trace = [torch.stack(x).cpu() for x in trace]
        else:
            e.rollout_random(STEPS, t0=0, steps_per_launch=spl)
        torch.cuda.synchronize()
        out = (e._obs.clone(), e._rew.clone(), e._done.clone(), e._info.clone(), e.get_state().clone())
        e.close()
        return out, trace
    finally:
        if old is None:
            os.environ.pop("SS_HELPERS", None)
        else:
            os.environ["SS_HELPERS"] = old


def classes(trace, n):
    done, adv, flags = trace
    steps = torch.arange(STEPS)
    quiet = (flags == 0) & ~done                 # a reset clears the flags: such an env-step says nothing about its contacts
    w = 0
    for first in range(0, n, 32):                # 32 envs per workgroup
        w += int(quiet[:, first:first + 32].all(dim=1).sum())
    o = int((((flags == 1) | (flags == 2)) & ~done).sum())
    return {"w": w, "o": o, "a": int(done[steps % 7 == 0].sum()), "a21": int(done[steps % 21 == 0].sum()),
            "b": int(done[steps % 7 == 6].sum()), "b21": int(done[steps % 21 == 20].sum()), "c": int((done & adv).sum())}


@pytest.mark.parametrize("n", [33, 97])
@pytest.mark.parametrize("env_id,curriculum", CASES)
def test_limb_tail_on_the_helpers_keeps_every_bit(env_id, curriculum, n):
    ref, trace = run(env_id, curriculum, n, "0", 1)            # the plain kernel, 63 single launches
    got = classes(trace, n)
    print("%s %d envs: %d episodes ended; %s" % (env_id, n, int(trace[0].sum()), got))
    for key, least in (("w", 3), ("o", 3), ("a", 3), ("a21", 1), ("b", 3), ("b21", 1), ("c", 3)):
        assert got[key] >= least, "class (%s): %d, at least %d wanted: %s" % (key, got[key], least, got)
    for spl in (21, 7):
        same(ref, run(env_id, curriculum, n, "3", spl)[0], "SS_HELPERS=3, %d launches of %d steps, against SS_HELPERS=0" % (STEPS // spl, spl))
