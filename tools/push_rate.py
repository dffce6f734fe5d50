#!/usr/bin/env python3
"""Time per call of the push (ss_push; docs/PHYSICS.md 12), dry run and applied, beside ss_eom (all outputs) and
ss_kinematics in the same process, and beside the torch route it replaces -- equation_of_motion(mass=True) + torch.linalg.solve +
get_state / set_state, given the right-hand side J^T w for nothing -- with device events: Walker3D, curriculum 5, after 30 random control
steps (the method of tools/eom_rate.py).  Every row pushes a drawn body at a point 0.1 m off its link origin with a mixed wrench.

    python tools/push_rate.py [--envs 4096,32768] [--reps 20]
    STEPPINGSTONE_LIB=var/libss_NAME.so python tools/push_rate.py        (another build of the same sources: A/B in a process of its own)

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
    gen = torch.Generator().manual_seed(7)
    new = lambda *shape: torch.empty((n,) + shape, device="cuda:0")
    body = torch.randint(0, 22, (n,), generator=gen, dtype=torch.int32).to("cuda:0")
    point = (0.1 * torch.nn.functional.normalize(torch.randn((n, 3), generator=gen), dim=1)).to("cuda:0")
    w = torch.randn((n, 6), generator=gen).to("cuda:0")
    small = 1e-3 * w                               # applied 20 times over: the state must stay a walking robot's
    dnu = new(27)
    ma, fo, ja = new(27, 27), new(3, 27), new(8, 3, 27)
    bt, sm, cr = new(22, 6), new(12), new(8, 8)
    rhs = torch.randn((n, 27, 1), generator=gen).to("cuda:0")

    def torch_route():
        M = env.equation_of_motion(mass=True, forces=False, jacobians=False)["mass"]
        d = torch.linalg.solve(M, 1e-3 * rhs)[:, :, 0]
        st = env.get_state()
        st[:, 7:13] += d[:, :6]
        st[:, 34:55] += d[:, 6:]
        env.set_state(st)

    res = dict(kind=kind, envs=n, reps=reps, lib=os.environ.get("STEPPINGSTONE_LIB", "shipped"))
    res["push_dry_us"] = timed(lambda: be.push(None, n, body, point, w, dnu, False), reps)
    res["push_apply_us"] = timed(lambda: be.push(None, n, body, point, small, dnu, True), reps)
    res["push_apply_no_delta_nu_us"] = timed(lambda: be.push(None, n, body, point, small, None, True), reps)
    res["push_torso_com_dry_us"] = timed(lambda: be.push(None, n, None, None, w, dnu, False), reps)
    res["eom_all_us"] = timed(lambda: be.eom(None, n, ma, fo, ja), reps)
    res["kinematics_all_us"] = timed(lambda: be.kinematics(None, n, bt, sm, cr), reps)
    res["torch_route_us"] = timed(torch_route, reps)
    res["push_dry_again_us"] = timed(lambda: be.push(None, n, body, point, w, dnu, False), reps)
    res["bytes_written_per_row"] = 4 * (27 + 27)
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
