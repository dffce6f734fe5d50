#!/usr/bin/env python3
"""Cost of keep_terminal_obs: the per-step time of SteppingStoneVecEnv.step() at 4096 Walker3D envs under random
actions, with and without keep_terminal_obs (the step with auto-reset off plus one reset_masked_kernel launch), timed with device
events in interleaved blocks; and the share of envs that finish per step.

    python tools/reset_rate.py [--envs 4096] [--steps 200] [--reps 15]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/reset_rate.py --reps 2      (kernel times in a run of its own)

Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--envs", type=int, default=4096)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--reps", type=int, default=15)
    a = p.parse_args()
    from steppingstone_amd.envs import SteppingStoneVecEnv
    envs = {"default": SteppingStoneVecEnv("Walker3DStepperEnv-v0", a.envs, seed=1, device="cuda:0"),
            "keep_terminal_obs": SteppingStoneVecEnv("Walker3DStepperEnv-v0", a.envs, seed=1, device="cuda:0", keep_terminal_obs=True)}
    acts = [envs["default"].random_actions(t) for t in range(64)]
    for e in envs.values():
        e.reset()
        for t in range(50):                    # warm-up: code objects loaded, episodes desynchronised
            e.step(acts[t % 64])
    torch.cuda.synchronize()
    us = {k: [] for k in envs}
    finished = 0
    for r in range(a.reps):
        order = list(envs) if r % 2 == 0 else list(envs)[::-1]
        for k in order:
            e = envs[k]
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for t in range(a.steps):
                e.step(acts[t % 64])
            t1.record()
            t1.synchronize()
            us[k].append(1e3 * t0.elapsed_time(t1) / a.steps)
    e = envs["keep_terminal_obs"]
    for t in range(a.steps):                   # reset rate, outside the timed blocks
        _, _, d, _ = e.step(acts[t % 64])
        finished += int(d.sum())
    res = dict(envs=a.envs, steps_per_block=a.steps, blocks=a.reps, finished_per_step=round(finished / a.steps, 1))
    for k, v in us.items():
        res[k] = dict(us_per_step_median=round(float(np.median(v)), 2), min=round(float(min(v)), 2), max=round(float(max(v)), 2))
    res["added_us_per_step_median"] = round(float(np.median(np.array(us["keep_terminal_obs"]) - np.array(us["default"]))), 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
