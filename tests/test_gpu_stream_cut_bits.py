"""The rule of tests/test_gpu_branches.py -- a K-step launch computes the bits of K single launches, and every kernel variant the
bits of the three-helper one -- at the small shapes where the code of the main wavefront's instruction-stream cut differs between
the variants: the half-broadcast rows and the joint-limit forms are shared by all of them, the paired A / C blocks of the spine joints
are the three-helper kernels' alone, and the plain / one-helper kernels are built with another scheduling strategy.

Shapes: 64 envs (three helpers, two workgroups), 70 envs (a partly filled workgroup), 64 envs under SS_HELPERS=1 and SS_HELPERS=0;
both robots, curriculum 5, 12 control steps from reset under the device's random actions.  The seeds are chosen with the CPU oracle
(tests/oracle_lib.py, 12 steps of its random_actions at these shapes): Walker3D seed 3 has feet down from the first step on (19 - 43
envs per step) and 9 - 10 episodes end from step 7 on; Mike seed 11 has 42 - 61 envs in contact per step and two episodes end on
the twelfth step (seeds 0 - 10 end none within 12 steps).  So the twelve steps run the contact solve cold (substep 1) and warm
(substeps 2 - 4) and at least one auto-reset; the test asserts both from the device's own outputs."""
import os

import pytest

import oracle_lib as ol

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

STEPS = 12
CASES = [("Walker3DStepperEnv-v0", 3), ("MikeStepperEnv-v0", 11)]
NAMES = ["obs", "rew", "done", "info", "state"]


def run(env_id, seed, n, helpers, spl):
    from steppingstone_amd.envs import SteppingStoneVecEnv
    old = os.environ.get("SS_HELPERS")
    try:
        if helpers is None:
            os.environ.pop("SS_HELPERS", None)
        else:
            os.environ["SS_HELPERS"] = helpers
        e = SteppingStoneVecEnv(env_id, n, seed=seed, device="cuda:0", return_numpy=False)
        e.update_curriculum(5)
        e.reset()
        # envs with the SAME foot down at the end of two successive control steps: the second step's contact solves start warm
        # (substeps 2 - 4 from the substep before; only single launches show every step's flags)
        contact = torch.zeros(n, dtype=torch.bool, device="cuda:0")
        prev = torch.zeros((n, 2), dtype=torch.bool, device="cuda:0")
        if spl == 1:
            for t in range(STEPS):
                e.rollout_random(1, t0=t, steps_per_launch=1)
                now = (e._obs[:, 48:50] > 0) & ~e._done.bool()[:, None]      # a finished env shows its reset state
                contact |= (now & prev).any(dim=1)
                prev = now
        else:
            e.rollout_random(STEPS, t0=0, steps_per_launch=spl)
        torch.cuda.synchronize()
        out = (e._obs.clone(), e._rew.clone(), e._done.clone(), e._info.clone(), e.get_state().clone())
        e.close()
        return out, contact
    finally:
        if old is None:
            os.environ.pop("SS_HELPERS", None)
        else:
            os.environ["SS_HELPERS"] = old


def same(a, b, what, rows=None):
    for name, x, y in zip(NAMES, a, b):
        if rows is not None:
            x, y = x[:rows], y[:rows]
        assert torch.equal(x, y), "%s: %s differs in %d envs" % (what, name, int((x != y).reshape(x.shape[0], -1).any(dim=1).sum()))


@pytest.mark.parametrize("env_id,seed", CASES)
def test_small_shapes_keep_their_bits_across_launch_forms_and_variants(env_id, seed):
    ref64, contact = run(env_id, seed, 64, None, 1)            # three helpers, twelve single launches
    # what the seed was chosen for: the same foot of an env on the ground in two successive steps, and an episode that ended and was reset
    assert int(contact.sum()) >= 16, "too few envs kept a foot down over two successive steps: %d" % int(contact.sum())
    assert bool((ref64[4][:, ol.S_ELAPSED] < STEPS).any()), "no env was reset within %d steps" % STEPS
    same(ref64, run(env_id, seed, 64, None, STEPS)[0], "64 envs, three helpers: one 12-step launch against 12 launches")
    same(ref64, run(env_id, seed, 64, "1", STEPS)[0], "64 envs: one helper against three")
    same(ref64, run(env_id, seed, 64, "0", STEPS)[0], "64 envs: plain kernel against three helpers")
    ref70, _ = run(env_id, seed, 70, None, 1)
    same(ref70, run(env_id, seed, 70, None, STEPS)[0], "70 envs: one 12-step launch against 12 launches")
    same(ref64, ref70, "the first 64 of 70 envs against 64 envs", rows=64)
