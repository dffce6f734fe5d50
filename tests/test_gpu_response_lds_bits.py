"""The contact response of the three-helper K-step kernel takes the spine + leg joint records and the base factor back from the hand-off
region (ss_dynamics.hpp: response_from_lds(); words 0..92, which the main wavefront itself wrote before barriers #1 and #2) instead of
holding them in registers across the rows and the PGS.  The words read back are the bits that were written, so nothing may move.  The
plain kernel (SS_HELPERS=0) has no hand-off region and cannot be touched by the change: it is the reference.  At 33 and 97 envs -- the
last workgroup holds one real env and 31 padding pairs --, both robots (Walker3D at curriculum 0, Mike at curriculum 5), 21 control
steps under the benchmark's Philox actions with auto-reset on,

  * SS_HELPERS = 3 as three 7-step launches (the kernel that reads the records back; the words must survive from their writer to the
    response of the same substep and across kstep > 0) and as 21 single launches (the one-step kernel, which keeps its registers),
  * SS_HELPERS = 1 both ways (the shared code paths of solve())

give obs, rew, done, info and the full state of SS_HELPERS = 0 as 21 single launches, bit for bit.

The reference run itself must have had at least one env in contact and at least one episode ended: otherwise the response never read
a record and the reset path never ran.  The test asserts on what the device reports in its own run."""
import os

import pytest

import oracle_lib as ol

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

STEPS = 21
SPL = 7                     # three 7-step launches
SEED = 0
CASES = [("Walker3DStepperEnv-v0", 0), ("MikeStepperEnv-v0", 5)]
NAMES = ["obs", "rew", "done", "info", "state"]


def run(env_id, curriculum, n, helpers, spl):
    """-> (obs, rew, done, info, state) after STEPS control steps; with spl == 1 also how many envs were ever in contact and how many
    episodes ended (None, None otherwise: a K-step launch shows only its last step)"""
    from steppingstone_amd.envs import SteppingStoneVecEnv
    old = os.environ.get("SS_HELPERS")
    try:
        os.environ["SS_HELPERS"] = helpers
        e = SteppingStoneVecEnv(env_id, n, seed=SEED, device="cuda:0", return_numpy=False)
        e.update_curriculum(curriculum)
        e.reset()
        contact = ended = None
        if spl == 1:
            contact = torch.zeros(n, dtype=torch.bool, device="cuda:0")
            ended = 0
            for t in range(STEPS):
                e.rollout_random(1, t0=t, steps_per_launch=1)
                contact |= (e._obs[:, 48:50] > 0).any(dim=1) & ~e._done.bool()
                ended += int(e._done.bool().sum())
            contact = int(contact.sum())
        else:
            e.rollout_random(STEPS, t0=0, steps_per_launch=spl)
        torch.cuda.synchronize()
        out = (e._obs.clone(), e._rew.clone(), e._done.clone(), e._info.clone(), e.get_state().clone())
        e.close()
        return out, contact, ended
    finally:
        if old is None:
            os.environ.pop("SS_HELPERS", None)
        else:
            os.environ["SS_HELPERS"] = old


def same(a, b, what):
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), "%s: %s differs in %d envs" % (what, name, int((x != y).reshape(x.shape[0], -1).any(dim=1).sum()))


@pytest.mark.parametrize("n", [33, 97])
@pytest.mark.parametrize("env_id,curriculum", CASES)
def test_response_from_lds_keeps_every_bit(env_id, curriculum, n):
    ref, contact, ended = run(env_id, curriculum, n, "0", 1)            # the plain kernel, 21 single launches
    print("%s %d envs: %d envs in contact at some step, %d episodes ended" % (env_id, n, contact, ended))
    assert contact >= 1, "no env ever had a foot down: the response never read a record"
    assert ended >= 1 and bool((ref[4][:, ol.S_ELAPSED] < STEPS).any()), "no episode ended within %d steps: the reset path never ran" % STEPS
    for helpers in ("3", "1"):
        same(ref, run(env_id, curriculum, n, helpers, SPL)[0], "SS_HELPERS=%s, three %d-step launches, against SS_HELPERS=0" % (helpers, SPL))
        same(ref, run(env_id, curriculum, n, helpers, 1)[0], "SS_HELPERS=%s, %d launches, against SS_HELPERS=0" % (helpers, STEPS))
