#!/usr/bin/env python3
"""Time per call of the closed-loop look-ahead (ss_lookahead_policy; docs/PHYSICS.md 14) beside what there was before it,
in the same process, with device events, as interleaved series (tools/lookahead_rate.py's method): Walker3D, curriculum 5, auto-reset
off, after 30 random control steps, one branch per env from the envs' states handed in as `states`, the shipped Walker3D actor
(tests/golden/shipped_actor_walker3d.npz, 60 -> 256 x5 -> 21) as the policy.
  fused_us          (a) one ss_lookahead_policy of H steps (act, obs, final_state asked for)
  loop_eager_us     (b) H iterations of: torch actor on the observation, ss_lookahead_states with H = 1 and final_state, chained through
                        its obs and final_state (no observe, no set_state), launched one by one ...
  loop_graph_us         ... and the same H iterations captured once into one torch.cuda.graph and replayed: the honest baseline
  open_loop_us      (c) ss_lookahead_states of H steps on (a)'s reported actions: the physics alone
  pack_us           ss_policy_pack of the actor
loop_vs_fused_max_action_difference_live_rows is a sanity figure, not a tolerance: torch sums the actor in another order, the last bits
of the first action differ, and 16 steps of contact dynamics under a feedback policy grow that in some rows (the tests hold the
fused call's own actions and physics, tests/test_gpu_lookahead_policy.py).

    python tools/policy_lookahead_rate.py [--envs 256,4096,32768] [--horizon 16] [--reps 20]

Prints one JSON line per batch size: median (fastest - slowest) in microseconds."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from forces_rate import timed  # noqa: E402
from lookahead_rate import interleaved  # noqa: E402

DEV = "cuda:0"


def shipped_actor():
    from steppingstone_amd import ppo
    w = np.load(os.path.join(ROOT, "tests", "golden", "shipped_actor_walker3d.npz"))
    actor = ppo.Actor()
    with torch.no_grad():
        for name in ("fc1", "fc2", "fc3", "fc4", "fc5", "out"):
            getattr(actor, name).weight.copy_(torch.from_numpy(w[name + ".weight"]))
            getattr(actor, name).bias.copy_(torch.from_numpy(w[name + ".bias"]))
    return actor.to(DEV).eval()


def measure(n, horizon, reps):
    from steppingstone_amd import _lib
    from steppingstone_amd.envs import SteppingStoneVecEnv, pack_policy
    env = SteppingStoneVecEnv("Walker3DStepperEnv-v0", n, seed=5, device=DEV)
    env.update_curriculum(5)
    env.reset()
    env.rollout_random(30, t0=0, steps_per_launch=1)
    env.set_auto_reset(False)
    be = env.backend
    actor = shipped_actor()
    pol = pack_policy(actor, env)
    start = env.get_state().clone()
    new = lambda *shape: torch.empty((n,) + shape, device=DEV)
    act, obs, rew, fs, work = new(horizon, 21), new(horizon, 60), new(horizon), new(186), new(_lib.LOOK_WORK)
    done = torch.empty((n, horizon), dtype=torch.uint8, device=DEV)

    def fused():
        be.lookahead_policy(None, n, start, horizon, pol.desc, pol.blob, None, act, obs, rew, done, fs, work)

    # (b): the loop the parent can do.  Step s reads the state and the observation step s - 1 wrote; two state buffers alternate.
    # Its outputs are step-major ([H, n, ...]), so that every call writes its rows in place and the loop holds no copy kernels: the
    # actor's launches and the H = 1 look-aheads are all there is.
    o0 = new(60)
    st = [new(186), new(186)]
    step_major = lambda *shape, **kw: torch.empty((horizon, n, 1) + shape, device=DEV, **kw)
    o_t, r_t, d_t = step_major(60), step_major(), step_major(dtype=torch.uint8)
    acts = [None] * horizon

    def loop():
        be.get_obs_states(n, start, o0)
        o, cur = o0, start
        with torch.no_grad():
            for s in range(horizon):
                acts[s] = actor(o)
                nxt = st[s & 1]
                be.lookahead_states(None, n, cur, 1, acts[s], o_t[s], r_t[s], d_t[s], nxt, work)
                o, cur = o_t[s, :, 0], nxt

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        loop()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loop()
    graph.replay()
    fused()
    torch.cuda.synchronize()
    live = ~done.bool().any(1)
    # the loop and the fused call walk the same branches (the actor's float32 sums differ in their last bits, so not bit for bit)
    agree = float((torch.stack(acts, 1)[live] - act[live]).abs().max()) if bool(live.any()) else float("nan")
    frozen_act = act.clone()

    res = dict(rows=n, horizon=horizon, reps=reps, lib=os.environ.get("STEPPINGSTONE_LIB", "shipped"))
    res.update(interleaved(dict(
        fused_us=fused,
        loop_graph_us=graph.replay,
        loop_eager_us=loop,
        open_loop_us=lambda: be.lookahead_states(None, n, start, horizon, frozen_act, obs, rew, done, fs, work)), reps))
    res["pack_us"] = timed(lambda: pol.refresh(), reps)
    res["live_through_horizon"] = round(float(live.float().mean()), 3)
    res["loop_vs_fused_max_action_difference_live_rows"] = agree
    res["fused_faster_than_graph_loop_beyond_spread"] = bool(res["fused_us"][2] < res["loop_graph_us"][1])
    env.close()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--envs", default="256,4096,32768")
    p.add_argument("--horizon", type=int, default=16)
    p.add_argument("--reps", type=int, default=20)
    a = p.parse_args()
    for n in a.envs.split(","):
        print(json.dumps(measure(int(n), a.horizon, a.reps)), flush=True)


if __name__ == "__main__":
    main()
