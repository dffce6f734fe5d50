#!/usr/bin/env python3
"""Time per call of the look-ahead (ss_lookahead; docs/PHYSICS.md 13), with and without the observation rows and the final
state, beside the only route there was before it -- H launches of ss_step on as many envs, which gives one branch per env and overwrites
the envs -- in the same process, with device events: Walker3D, curriculum 5, auto-reset off, after 30 random control steps (the method of
tools/push_rate.py).  One branch per env, bounded random actions (most branches survive the horizon; a finished one keeps its lanes busy
until its wavefront has nothing left).  The il_* figures are three series interleaved in one loop: ss_lookahead, ss_lookahead_states on the
same rows handed in as `states`, and the set_state route that call replaces (save the envs, put the rows in, look ahead, put the envs back).

    python tools/lookahead_rate.py [--envs 4096,32768] [--horizon 16] [--reps 20]
    STEPPINGSTONE_LIB=var/libss_NAME.so python tools/lookahead_rate.py   (another build of the same sources: A/B in a process of its own)

Prints one JSON line per batch size: median (fastest - slowest) in microseconds."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from forces_rate import timed  # noqa: E402


def measure(kind, n, horizon, reps):
    from steppingstone_amd import _lib
    from steppingstone_amd.envs import SteppingStoneVecEnv
    env = SteppingStoneVecEnv("Walker3DStepperEnv-v0" if kind == "walker3d" else "MikeStepperEnv-v0", n, seed=5, device="cuda:0")
    env.update_curriculum(5)
    env.reset()
    env.rollout_random(30, t0=0, steps_per_launch=1)
    env.set_auto_reset(False)
    be = env.backend
    gen = torch.Generator().manual_seed(7)
    act = (0.3 * torch.randn((n, horizon, 21), generator=gen)).to("cuda:0")
    steps = [act[:, s].contiguous() for s in range(horizon)]
    new = lambda *shape: torch.empty((n,) + shape, device="cuda:0")
    obs, rew, fs, work = new(horizon, 60), new(horizon), new(186), new(_lib.LOOK_WORK)
    done = torch.empty((n, horizon), dtype=torch.uint8, device="cuda:0")
    o1, r1 = new(60), new()
    d1, i1 = torch.empty(n, dtype=torch.uint8, device="cuda:0"), torch.empty((n, 6), dtype=torch.int32, device="cuda:0")
    start = env.get_state().clone()

    def real_steps():
        for a in steps:
            be.step(a, o1, r1, d1, i1)

    res = dict(kind=kind, rows=n, horizon=horizon, reps=reps, lib=os.environ.get("STEPPINGSTONE_LIB", "shipped"))
    res["lookahead_all_us"] = timed(lambda: be.lookahead(None, n, horizon, act, obs, rew, done, fs, work), reps)
    res["finished_in_horizon"] = round(float(done[:, -1].float().mean()), 3)
    res["lookahead_obs_us"] = timed(lambda: be.lookahead(None, n, horizon, act, obs, rew, done, None, work), reps)
    res["lookahead_no_obs_us"] = timed(lambda: be.lookahead(None, n, horizon, act, None, rew, done, None, work), reps)
    res["steps_us"] = timed_from(env, start, real_steps, reps)
    res["lookahead_all_again_us"] = timed(lambda: be.lookahead(None, n, horizon, act, obs, rew, done, fs, work), reps)
    # From caller-supplied states (ss_lookahead_states): the rows the env holds, handed in as `states`, so that every series below does
    # the same work per row.  Three series interleaved call by call, each with its own events: ss_lookahead, ss_lookahead_states, and
    # the route the latter replaces -- save the envs, put the rows in, look ahead, put the envs back.
    ids = torch.arange(n, dtype=torch.int32, device="cuda:0")
    saved = torch.empty_like(start)
    env.set_state(start)

    def route():
        be.get_state_envs(ids, saved)
        be.set_state_envs(ids, start)
        be.lookahead(ids, n, horizon, act, obs, rew, done, fs, work)
        be.set_state_envs(ids, saved)

    series = interleaved(dict(
        il_lookahead_us=lambda: be.lookahead(ids, n, horizon, act, obs, rew, done, fs, work),
        il_from_states_us=lambda: be.lookahead_states(ids, n, start, horizon, act, obs, rew, done, fs, work),
        il_set_state_route_us=route), reps)
    res.update(series)
    o0 = new(60)
    res["observe_us"] = timed(lambda: be.get_obs_states(n, start, o0), reps)
    res["bytes_written_per_row"] = 4 * (horizon * 61 + 186) + horizon
    env.close()
    return res


def interleaved(fns, reps):
    """timed() of several calls, one call of each per round, so that drift of the clocks lands on all series alike"""
    import numpy as np
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3)
    return {k: [round(float(np.median(t)), 1), round(float(min(t)), 1), round(float(max(t)), 1)] for k, t in times.items()}


def timed_from(env, start, fn, reps):
    """timed(), with the envs put back into `start` before every call (outside the events)"""
    import numpy as np
    times = []
    for k in range(reps + 3):
        env.set_state(start)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if k >= 3:
            times.append(a.elapsed_time(b) * 1e3)
    return [round(float(np.median(times)), 1), round(float(min(times)), 1), round(float(max(times)), 1)]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--envs", default="4096,32768")
    p.add_argument("--kinds", default="walker3d")
    p.add_argument("--horizon", type=int, default=16)
    p.add_argument("--reps", type=int, default=20)
    a = p.parse_args()
    for kind in a.kinds.split(","):
        for n in a.envs.split(","):
            print(json.dumps(measure(kind, int(n), a.horizon, a.reps)), flush=True)


if __name__ == "__main__":
    main()
