"""The joint torques of the four {leg, arm} pairs of joints on packed instructions (the three-helper K-step kernel; every other kernel
keeps the scalar form) change no bit: at 64 envs (two full workgroups) and 70 envs (a workgroup with padding lanes), both robots, 40
control steps under the benchmark's Philox actions with auto-reset on (Walker3D at curriculum 0, Mike at curriculum 5),

  * one 40-step launch computes what 40 single launches compute, in state, obs, rew, done and info;
  * SS_HELPERS = 0, 1 and 3 compute the same;
  * the final state's SHA-256 is the one the library of the commit BEFORE the pair form gives at the same shape: recorded once on an
    MI355X from a build of that commit (PARENT), with this file's final_state_hash().

Forty steps reach contact (cold and warm solves), target advances and resets; the test asserts contact and resets from the device's own
outputs."""
import hashlib
import os

import pytest

import oracle_lib as ol

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

STEPS = 40
SEED = 7
CASES = [("Walker3DStepperEnv-v0", 0), ("MikeStepperEnv-v0", 5)]
NAMES = ["obs", "rew", "done", "info", "state"]
PARENT = "4f0777a"          # the commit whose library gave PARENT_HASH
PARENT_HASH = {
    ("Walker3DStepperEnv-v0", 64): "79261c1c7c3feaaec64391b6f74a4559",
    ("Walker3DStepperEnv-v0", 70): "0c5eb4f4a1ba12b5b0250e1e2f27a323",
    ("MikeStepperEnv-v0", 64): "3bd4318a3a8794ffeade96459d2a8d74",
    ("MikeStepperEnv-v0", 70): "fca36acc2d8f31f4ec6639e5e4ea77a1",
}


def run(env_id, curriculum, n, helpers, spl):
    """-> (obs, rew, done, info, state) after STEPS control steps, how many envs were ever in contact, how many steps ended an episode"""
    from steppingstone_amd.envs import SteppingStoneVecEnv
    old = os.environ.get("SS_HELPERS")
    try:
        if helpers is None:
            os.environ.pop("SS_HELPERS", None)
        else:
            os.environ["SS_HELPERS"] = helpers
        e = SteppingStoneVecEnv(env_id, n, seed=SEED, device="cuda:0", return_numpy=False)
        e.update_curriculum(curriculum)
        e.reset()
        contact = torch.zeros(n, dtype=torch.bool, device="cuda:0")
        ended = 0
        if spl == 1:
            for t in range(STEPS):
                e.rollout_random(1, t0=t, steps_per_launch=1)
                contact |= (e._obs[:, 48:50] > 0).any(dim=1) & ~e._done.bool()
                ended += int(e._done.bool().sum())
        else:
            e.rollout_random(STEPS, t0=0, steps_per_launch=spl)
        torch.cuda.synchronize()
        out = (e._obs.clone(), e._rew.clone(), e._done.clone(), e._info.clone(), e.get_state().clone())
        e.close()
        return out, int(contact.sum()), ended
    finally:
        if old is None:
            os.environ.pop("SS_HELPERS", None)
        else:
            os.environ["SS_HELPERS"] = old


def state_hash(out):
    return hashlib.sha256(out[4].cpu().numpy().tobytes()).hexdigest()[:32]


def final_state_hash(env_id, curriculum, n):
    """what PARENT_HASH holds: the final state of one 40-step launch of the default (three-helper) kernel"""
    return state_hash(run(env_id, curriculum, n, None, STEPS)[0])


def same(a, b, what):
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), "%s: %s differs in %d envs" % (what, name, int((x != y).reshape(x.shape[0], -1).any(dim=1).sum()))


@pytest.mark.parametrize("n", [64, 70])
@pytest.mark.parametrize("env_id,curriculum", CASES)
def test_pair_forms_keep_every_bit(env_id, curriculum, n):
    ref, contact, ended = run(env_id, curriculum, n, "3", 1)            # three helpers, forty single launches
    print("%s %d envs: %d envs in contact at some step, %d episodes ended, final state %s" % (env_id, n, contact, ended, state_hash(ref)))
    assert contact >= n // 2, "too few envs ever had a foot down: %d" % contact
    assert ended >= 1 and bool((ref[4][:, ol.S_ELAPSED] < STEPS).any()), "no env was reset within %d steps" % STEPS
    k3 = run(env_id, curriculum, n, "3", STEPS)[0]
    same(ref, k3, "three helpers: one %d-step launch against %d launches" % (STEPS, STEPS))
    same(ref, run(env_id, curriculum, n, None, STEPS)[0], "the default kernel against SS_HELPERS=3")
    for helpers in ("1", "0"):
        same(ref, run(env_id, curriculum, n, helpers, STEPS)[0], "SS_HELPERS=%s, one launch, against three helpers" % helpers)
        same(ref, run(env_id, curriculum, n, helpers, 1)[0], "SS_HELPERS=%s, %d launches, against three helpers" % (helpers, STEPS))
    assert state_hash(k3) == PARENT_HASH[(env_id, n)], "the final state is not the one commit %s computes: %s" % (PARENT, state_hash(k3))
