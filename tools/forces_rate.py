#!/usr/bin/env python3
"""Time per call of the force readout (ss_step_forces; docs/PHYSICS.md 10) beside ss_step (one launch per control step) in
the same process, with device events: Walker3D, curriculum 5, after 30 random control steps.

    python tools/forces_rate.py [--envs 4096,32768] [--reps 20]
    STEPPINGSTONE_LIB=var/libss_NAME.so python tools/forces_rate.py        (another build of the same sources: A/B in a process of its own)

Prints one JSON line per batch size: median (fastest - slowest) in microseconds."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return [round(float(np.median(times)), 1), round(float(min(times)), 1), round(float(max(times)), 1)]


def measure(kind, n, reps):
    from steppingstone_amd.envs import SteppingStoneVecEnv
    env = SteppingStoneVecEnv("Walker3DStepperEnv-v0" if kind == "walker3d" else "MikeStepperEnv-v0", n, seed=5, device="cuda:0")
    env.update_curriculum(5)
    env.reset()
    env.rollout_random(30, t0=0, steps_per_launch=1)
    be = env.backend
    act = env.random_actions(1000)
    co = torch.empty((n, 4, 8, 8), device="cuda:0")
    jo = torch.empty((n, 4, 4, 21), device="cuda:0")
    ns = torch.empty((n, 56), device="cuda:0")
    res = dict(kind=kind, envs=n, reps=reps, lib=os.environ.get("STEPPINGSTONE_LIB", "shipped"))
    res["forces_all_us"] = timed(lambda: be.step_forces(None, n, act, co, jo, ns), reps)
    res["forces_contacts_us"] = timed(lambda: be.step_forces(None, n, act, co, None, None), reps)
    res["forces_joints_us"] = timed(lambda: be.step_forces(None, n, act, None, jo, None), reps)
    res["forces_next_state_us"] = timed(lambda: be.step_forces(None, n, act, None, None, ns), reps)
    res["step_us"] = timed(lambda: be.step(act, env._obs, env._rew, env._done, env._info), reps)
    res["ratio"] = round(res["forces_all_us"][0] / res["step_us"][0], 2)
    res["bytes_written_per_env"] = 4 * (4 * 8 * 8 + 4 * 4 * 21 + 56)
    env.close()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--envs", default="4096,32768")
    p.add_argument("--kinds", default="walker3d")
    p.add_argument("--reps", type=int, default=20)
    a = p.parse_args()
    for kind in a.kinds.split(","):
        for n in a.envs.split(","):
            print(json.dumps(measure(kind, int(n), a.reps)), flush=True)


if __name__ == "__main__":
    main()
