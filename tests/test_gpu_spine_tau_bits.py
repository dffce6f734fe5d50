"""In the three-helper K-step kernel helper 1 evaluates the explicit torques and implicit diagonals of the spine joints 0..2 in front of
barrier #1 and hands them to the main wavefront in six hand-off words (ss_dynamics.hpp: spine_tau_offload(), helper_substep); "a joint
is at its limit" has one definition for step_env and step_logic (ss_kernels.hpp: at_joint_limit).  Same functions: nothing may move.
The plain kernel (SS_HELPERS=0), which has no helper and calls joint_tau inline, is the reference.  At 33 and 97 envs -- the last
workgroup holds one real env and 31 padding pairs --, both robots (Walker3D at curriculum 0, Mike at curriculum 5), 63 control steps
under the benchmark's Philox actions with auto-reset on,

  * SS_HELPERS = 3 as three 21-step launches and as nine 7-step launches

give obs, rew, done, info and the full state of SS_HELPERS = 0 as 63 single launches, bit for bit (compared as 32-bit words: a zero of
the other sign is a difference).

Events are seeded through the packed state before the run: those of tests/test_gpu_limb_tail_bits.py (step limits at the launches'
borders, target advances, the lone env of the last workgroup lifted), and six envs that start with one spine joint each OUT (rad) below
its lower or above its upper bound, at rest (SPINE below: the six envs below 33 that the other tables leave alone).  The test asserts ON
THE REFERENCE RUN ALONE, from done and the state per step, that each class occurred:

  (lo0, hi0, lo1, hi1, lo2, hi2) a control step that begins with spine joint j below lo / above hi: the limit terms of
                                 tau and Dadd are live in its first substep                                    >= 1 env-step each
  (l) an env-step that ends, without a reset, with a joint at its limit (|q_norm| > 0.99: at_limit > 0)        >= 3 env-steps
  (a) a reset in the first step of a 7-step launch, (a21) of a 21-step launch                                  >= 3, >= 1 env-steps
  (b) a reset in the last step of a 7-step launch, (b21) of a 21-step launch                                   >= 3, >= 1 env-steps

(printed by the test: run it with -s)."""
import os

import numpy as np
import pytest

import oracle_lib as ol
from test_gpu_limb_tail_bits import seed_events
from test_gpu_reset_pose_bits import same
from test_limit_forms import bounds

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

STEPS = 63
SEED = 0
CASES = [("Walker3DStepperEnv-v0", 0, 0), ("MikeStepperEnv-v0", 5, 1)]      # env id, curriculum, kind of the model tables
OUT = 0.15
# env -> (spine joint, -1: below lo, +1: above hi)
SPINE = {0: (0, -1), 7: (0, +1), 28: (1, -1), 29: (1, +1), 30: (2, -1), 31: (2, +1)}


def seed_spine(e, kind):
    lo, hi = bounds()[kind]
    st = e.get_state().clone()
    for i, (j, sign) in SPINE.items():
        st[i, ol.S_Q.start + j] = float(lo[j]) - OUT if sign < 0 else float(hi[j]) + OUT
        st[i, ol.S_QD.start + j] = 0.0
    e.set_state(st)


def run(env_id, curriculum, kind, n, helpers, spl):
    """-> (obs, rew, done, info, state) after STEPS control steps; with spl == 1 also done of every step [STEPS, n] and the joint angles
    every step BEGINS with and ENDS with [STEPS, n, 21] (None otherwise: a K-step launch shows only its last step)"""
    from steppingstone_amd.envs import SteppingStoneVecEnv
    old = os.environ.get("SS_HELPERS")
    try:
        os.environ["SS_HELPERS"] = helpers
        e = SteppingStoneVecEnv(env_id, n, seed=SEED, device="cuda:0", return_numpy=False)
        e.update_curriculum(curriculum)
        e.reset()
        seed_events(e, n)
        seed_spine(e, kind)
        trace = None
        if spl == 1:
            trace = [[], [], []]
            for t in range(STEPS):
                trace[1].append(e.get_state()[:, ol.S_Q].clone())
                e.rollout_random(1, t0=t, steps_per_launch=1)
                trace[0].append(e._done.bool().clone())
                trace[2].append(e.get_state()[:, ol.S_Q].clone())
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


def classes(trace, kind):
    done, q0, q1 = trace[0], trace[1].numpy(), trace[2].numpy()
    lo, hi = bounds()[kind]
    got = {}
    for j in range(3):
        got["lo%d" % j] = int((q0[:, :, j] < lo[j]).sum())
        got["hi%d" % j] = int((q0[:, :, j] > hi[j]).sum())
    mid, span = np.float32(0.5) * (lo + hi), hi - lo
    at = (np.abs(np.float32(2.0) * (q1 - mid) / span) > np.float32(0.99)).any(axis=2)
    got["l"] = int((at & ~done.numpy()).sum())
    steps = torch.arange(STEPS)
    got.update(a=int(done[steps % 7 == 0].sum()), a21=int(done[steps % 21 == 0].sum()),
               b=int(done[steps % 7 == 6].sum()), b21=int(done[steps % 21 == 20].sum()))
    return got


@pytest.mark.parametrize("n", [33, 97])
@pytest.mark.parametrize("env_id,curriculum,kind", CASES)
def test_spine_torques_on_helper_1_keep_every_bit(env_id, curriculum, kind, n):
    ref, trace = run(env_id, curriculum, kind, n, "0", 1)            # the plain kernel, 63 single launches
    got = classes(trace, kind)
    print("%s %d envs: %d episodes ended; %s" % (env_id, n, int(trace[0].sum()), got))
    for key, least in (("lo0", 1), ("hi0", 1), ("lo1", 1), ("hi1", 1), ("lo2", 1), ("hi2", 1), ("l", 3),
                       ("a", 3), ("a21", 1), ("b", 3), ("b21", 1)):
        assert got[key] >= least, "class (%s): %d, at least %d wanted: %s" % (key, got[key], least, got)
    for spl in (21, 7):
        same(ref, run(env_id, curriculum, kind, n, "3", spl)[0], "SS_HELPERS=3, %d launches of %d steps, against SS_HELPERS=0" % (STEPS // spl, spl))
