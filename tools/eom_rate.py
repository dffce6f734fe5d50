#!/usr/bin/env python3
"""Time per call of the equation-of-motion readout (ss_eom; docs/PHYSICS.md 11) beside ss_kinematics and ss_step_forces in
the same process, with device events: Walker3D, curriculum 5, after 30 random control steps (the method of tools/forces_rate.py).

    python tools/eom_rate.py [--envs 4096,32768] [--reps 20]
    STEPPINGSTONE_LIB=var/libss_NAME.so python tools/eom_rate.py        (another build of the same sources: A/B in a process of its own)

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


def measure(kind, n, reps):
    from steppingstone_amd.envs import SteppingStoneVecEnv
    env = SteppingStoneVecEnv("Walker3DStepperEnv-v0" if kind == "walker3d" else "MikeStepperEnv-v0", n, seed=5, device="cuda:0")
    env.update_curriculum(5)
    env.reset()
    env.rollout_random(30, t0=0, steps_per_launch=1)
    be = env.backend
    act = env.random_actions(1000)
    new = lambda *shape: torch.empty((n,) + shape, device="cuda:0")
    ma, fo, ja = new(27, 27), new(3, 27), new(8, 3, 27)
    bt, sm, cr = new(22, 6), new(12), new(8, 8)
    co, jo, ns = new(4, 8, 8), new(4, 4, 21), new(56)
    res = dict(kind=kind, envs=n, reps=reps, lib=os.environ.get("STEPPINGSTONE_LIB", "shipped"))
    res["eom_all_us"] = timed(lambda: be.eom(None, n, ma, fo, ja), reps)
    res["eom_mass_us"] = timed(lambda: be.eom(None, n, ma, None, None), reps)
    res["eom_forces_us"] = timed(lambda: be.eom(None, n, None, fo, None), reps)
    res["eom_jacobians_us"] = timed(lambda: be.eom(None, n, None, None, ja), reps)
    res["kinematics_all_us"] = timed(lambda: be.kinematics(None, n, bt, sm, cr), reps)
    res["forces_all_us"] = timed(lambda: be.step_forces(None, n, act, co, jo, ns), reps)
    res["eom_all_again_us"] = timed(lambda: be.eom(None, n, ma, fo, ja), reps)
    res["bytes_written_per_env"] = 4 * (27 * 27 + 3 * 27 + 8 * 3 * 27)
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
