#!/usr/bin/env python3
"""Rate of the render kernel (docs/RENDER.md; DESIGN.md "Rendering") for the three shapes of the design note, timed with device events:

    (a) 4096 envs,  64 x 64     (b) 256 envs, 128 x 128     (c) 1 env, 640 x 480      RGB + depth + segmentation, shadows on

and the work a frame holds, counted by tests/np_render.py on the same states: ray-primitive tests per pixel (primary: every primitive,
before the kernel's tile culling; shadow: up to the first blocker) and the FP32 share of peak that follows from them.

    python tools/render_rate.py [--shapes a,b,c] [--reps 20]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/render_rate.py --reps 5 --no-count      (kernel times in a run of its own)

Prints one JSON line per shape."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {"a": (4096, 64, 64), "b": (256, 128, 128), "c": (1, 640, 480)}
PEAK_FP32 = 157.3e12          # MI355X vector FP32, FLOP/s (packed FMA counted as 4)
# FP32 operations per ray-primitive test and per pixel (ray set-up, shading, u8 conversion), counted from ss_render.hpp's arithmetic
# (an FMA counts 2): a sphere ~25, a capsule ~60, a three-slab solid ~50 -- 17 robot primitives are 13 capsules, 2 spheres, 2 boxes
FLOP_PER_TEST = (13 * 60 + 2 * 25 + 2 * 50 + 3 * 50) / 20.0
FLOP_PER_PIXEL = 80.0


def measure(kind, shape, reps, count):
    from steppingstone_amd.envs import SteppingStoneVecEnv, make_camera
    n, W, H = SHAPES[shape]
    env = SteppingStoneVecEnv("Walker3DStepperEnv-v0" if kind == "walker3d" else "MikeStepperEnv-v0", n, seed=5, device="cuda:0")
    env.update_curriculum(5)
    env.reset()
    env.rollout_random(30, t0=0, steps_per_launch=1)
    cam = make_camera("track", shadows=True)
    ids = torch.arange(n, dtype=torch.int32, device="cuda:0")
    rgb = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda:0")
    depth = torch.empty((n, H, W), dtype=torch.float32, device="cuda:0")
    seg = torch.empty((n, H, W), dtype=torch.uint8, device="cuda:0")
    for _ in range(3):
        env.backend.render(ids, W, H, cam, rgb, depth, seg)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        env.backend.render(ids, W, H, cam, rgb, depth, seg)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    ms = float(np.median(times))
    res = dict(shape=shape, kind=kind, envs=n, width=W, height=H, ms_per_call=round(ms, 4), ms_min=round(float(min(times)), 4),
               mpix_per_s=round(n * W * H / ms / 1e3, 1), robot_pixels=round(float(((seg >= 1) & (seg <= 22)).float().mean()), 4))
    if count:
        import np_render as nr
        st = env.get_state().cpu().numpy().astype(np.float64)
        cnt = {}
        for i in range(min(n, 8)):
            nr.render(kind, st[i], W, H, dict(nr.DEFAULT_CAMERA, shadows=True), counters=cnt)
        per_px = (cnt["primary"] + cnt.get("shadow", 0)) / cnt["pixels"]
        flop = n * W * H * (per_px * FLOP_PER_TEST + FLOP_PER_PIXEL)
        res.update(tests_per_pixel=round(per_px, 2), primary_per_pixel=round(cnt["primary"] / cnt["pixels"], 2),
                   shadow_per_pixel=round(cnt.get("shadow", 0) / cnt["pixels"], 2), gflop=round(flop / 1e9, 3),
                   fp32_share_of_peak=round(flop / (ms * 1e-3) / PEAK_FP32, 4))
    env.close()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shapes", default="a,b,c")
    p.add_argument("--kinds", default="walker3d")
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--no-count", action="store_true")
    a = p.parse_args()
    for kind in a.kinds.split(","):
        for s in a.shapes.split(","):
            print(json.dumps(measure(kind, s, a.reps, not a.no_count)), flush=True)


if __name__ == "__main__":
    main()
