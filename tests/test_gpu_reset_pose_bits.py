"""The three-helper K-step kernel takes the joint angles of a reset from twelve LDS words that a helper wavefront drew ahead of time
(ss_dynamics.hpp: reset_pose_offload(); ss_kernels.hpp: reset_pose_half) instead of drawing them on the main wavefront.  The pose is a
function of (seed, env id, Philox counter) and the counter moves only when the env resets or draws a stone, so nothing may move: the
plain kernel (SS_HELPERS=0), which has no helper, is the reference.  At 33 and 97 envs -- the last workgroup holds one real env and 31
padding pairs --, both robots (Walker3D at curriculum 0, Mike at curriculum 5), 63 control steps under the benchmark's Philox actions with
auto-reset on,

  * SS_HELPERS = 3 as three 21-step launches, as nine 7-step launches and as 63 single launches,
  * SS_HELPERS = 1 as nine 7-step launches and as 63 single launches

give obs, rew, done, info and the full state of SS_HELPERS = 0 as 63 single launches, bit for bit (compared as 32-bit words: a zero of
the other sign is a difference).

Events are seeded through the packed state before the run (SEEDED below): an env at elapsed = 999 - j ends at the step limit in step j;
an env standing over its target stone (as in test_rollout_kernel_is_bitwise_equal_to_single_step_launches) with count = 1 - a advances
its target -- and draws a stone, which moves the counter -- in the step in which its foot has been on the stone for a + 1 steps.  The
test asserts ON THE REFERENCE RUN ALONE, from done and info per step, that each class of event occurred:

  (a) a reset in the first step of a 7-step launch                                            >= 3 env-steps
  (b) a reset in the last step of one                                                         >= 3 env-steps
  (c) target advance and reset in the same step: the pose in LDS is stale, the inline draw    >= 3 env-steps
  (d) a target advance in step t and a reset in step t + 1: the pose was drawn again between  >= 3 env-steps
  (e) an env that FALLS twice (done twice, neither at the step limit) inside one 21-step launch  >= 1 env

Seed 0 gives all five in all four cases (printed by the test: run it with -s)."""
import os

import pytest

import oracle_lib as ol

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

STEPS = 63
SEED = 0
CASES = [("Walker3DStepperEnv-v0", 0), ("MikeStepperEnv-v0", 5)]
NAMES = ["obs", "rew", "done", "info", "state"]
LIMIT = 1000                 # SS_MAX_EPISODE_STEPS
# env -> (over its target stone, count, elapsed).  Env 32 is the lone env of the second workgroup at 33 envs.
#
# A robot set down over its stone has a foot carried by it from step 0 or from step 1 on (its feet start a centimetre above the ground
# and the joint noise decides; measured on the reference, about half each), so every (count, elapsed) below gives (c) for one of the
# two and most give (d) for the other:
#                                    foot on the stone from step 0             from step 1
#   A  count 1, elapsed 998          advance 0, limit 1: (d)                   advance 1, limit 1: (c)
#   B  count 0, elapsed 997          advance 1, limit 2: (d)                   advance 2, limit 2: (c)
#   C  count 1, elapsed 999          advance 0, limit 0: (c)                   reset in step 0, nothing
#   D  count 0, elapsed 998          advance 1, limit 1: (c)                   reset in step 1, nothing
#   E  count 1, elapsed 997          advance 0, nothing                        advance 1, limit 2: (d)
SEEDED = {}
for _i in (1, 2, 3):                                      # (a): step limit in step 7
    SEEDED[_i] = (False, 0, LIMIT - 1 - 7)
for _i in (4, 5, 6):                                      # (b): step limit in step 6
    SEEDED[_i] = (False, 0, LIMIT - 1 - 6)
for _ids, _count, _elapsed in (((8, 9, 10, 11, 12, 13, 14), 1, 998), ((15, 16, 17), 0, 997), ((18, 19, 20, 32), 1, 999),
                               ((21, 22, 23), 0, 998), ((24, 25, 26, 27), 1, 997)):
    for _i in _ids:
        SEEDED[_i] = (True, _count, _elapsed)


def seed_events(e):
    st = e.get_state().clone()
    for i, (over, count, elapsed) in SEEDED.items():
        if over:
            st[i, 0] = st[i, 65 + 6]              # x of stone 1, the target of a fresh episode
        st[i, ol.S_COUNT] = float(count)
        st[i, ol.S_ELAPSED] = float(elapsed)
    e.set_state(st)


def run(env_id, curriculum, n, helpers, spl, seed=SEED):
    """-> (obs, rew, done, info, state) after STEPS control steps; with spl == 1 also done, info.bad_transition and
    info.update_terrain of every step ([STEPS, n] each; None otherwise: a K-step launch shows only its last step)"""
    from steppingstone_amd.envs import SteppingStoneVecEnv
    old = os.environ.get("SS_HELPERS")
    try:
        os.environ["SS_HELPERS"] = helpers
        e = SteppingStoneVecEnv(env_id, n, seed=seed, device="cuda:0", return_numpy=False)
        e.update_curriculum(curriculum)
        e.reset()
        seed_events(e)
        trace = None
        if spl == 1:
            trace = [[], [], []]
            for t in range(STEPS):
                e.rollout_random(1, t0=t, steps_per_launch=1)
                trace[0].append(e._done.bool().clone())
                trace[1].append(e._info[:, 2].bool().clone())
                trace[2].append(e._info[:, 4].bool().clone())
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


def classes(trace):
    """the counts of the docstring's classes (a) .. (e) in a reference run"""
    done, bad, adv = trace
    steps = torch.arange(STEPS)
    a = int(done[steps % 7 == 0].sum())
    b = int(done[steps % 7 == 6].sum())
    c = int((done & adv).sum())
    d = int((adv[:-1] & done[1:]).sum())
    fell = done & ~bad                       # natural falls only: a seeded end is at the step limit
    e = torch.zeros(done.shape[1], dtype=torch.bool)
    for w in range(0, STEPS, 21):
        e |= fell[w:w + 21].sum(dim=0) >= 2
    return a, b, c, d, int(e.sum())


def words(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def same(a, b, what):
    for name, x, y in zip(NAMES, a, b):
        x, y = words(x), words(y)
        assert torch.equal(x, y), "%s: %s differs in %d envs" % (what, name, int((x != y).reshape(x.shape[0], -1).any(dim=1).sum()))


@pytest.mark.parametrize("n", [33, 97])
@pytest.mark.parametrize("env_id,curriculum", CASES)
def test_reset_pose_from_lds_keeps_every_bit(env_id, curriculum, n):
    ref, trace = run(env_id, curriculum, n, "0", 1)            # the plain kernel, 63 single launches
    a, b, c, d, e = classes(trace)
    print("%s %d envs: %d episodes ended; (a) %d (b) %d (c) %d (d) %d env-steps, (e) %d envs" % (env_id, n, int(trace[0].sum()), a, b, c, d, e))
    assert a >= 3, "(a) resets in the first step of a 7-step launch: %d" % a
    assert b >= 3, "(b) resets in the last step of a 7-step launch: %d" % b
    assert c >= 3, "(c) target advance and reset in one step: %d" % c
    assert d >= 3, "(d) target advance, reset one step later: %d" % d
    assert e >= 1, "(e) envs that fell twice inside one 21-step launch: %d" % e
    for helpers, spls in (("3", (21, 7, 1)), ("1", (7, 1))):
        for spl in spls:
            same(ref, run(env_id, curriculum, n, helpers, spl)[0],
                 "SS_HELPERS=%s, %d launches of %d steps, against SS_HELPERS=0" % (helpers, STEPS // spl, spl))
