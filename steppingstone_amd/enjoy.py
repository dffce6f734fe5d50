"""Run a policy in the GPU env and write what it does as an animation: the counterpart of the reference's `playground/enjoy.py`
(`make_env(env, render=True)`, deterministic actions, "Episode reward:" lines), drawn by the render kernel (docs/RENDER.md).

    python -m steppingstone_amd.enjoy --env Walker3DStepperEnv-v0 --net Walker3D_latest.pt --envs 4 --steps 300 --out walk.gif

--net takes a file written by ppo.save_checkpoint (or a bare ActorCritic state_dict), or a reference legacy .pt checkpoint
(legacy_checkpoint.load_reference_checkpoint).  The K envs are tiled into one frame per control step.  --out ending in .gif is written
with PIL when it is importable; otherwise, and for --out *.npy, the frames are saved as one [T, H, W, 3] uint8 array.

--trace FILE.npz also writes what the frames show as numbers (SteppingStoneVecEnv.kinematics, docs/PHYSICS.md 9), one entry per control
step and env, for the state each step ends in: com [T,K,3], com_vel [T,K,3], corner_height [T,K,8] (sole corners over the target stone's
surface plane), corner_carrier [T,K,8] (the stone slot that carries each corner, -1: none), contact [T,K,2] (the observation's foot
contact flags, right / left), next_step_index [T,K], done [T,K].

--forces (only together with --trace) adds the force readout of every step (SteppingStoneVecEnv.step_forces, docs/PHYSICS.md 10), taken
as a dry run from the state the step STARTS in, with the action the policy chose: contact_force [T,K,4,8,8] (per substep and sole
corner: carrier slot, penetration, force along n / t1 / t2, force as a world vector) and joint_torque [T,K,4,21] (the torque every joint
applied over each substep).

--push STEP:BODY:px,py,pz (repeatable) shoves every env's robot before control step STEP of the walk (SteppingStoneVecEnv.push,
docs/PHYSICS.md 12): a linear impulse (px, py, pz) in N s, world axes, at the centre of mass of BODY (an index or a name of
model.BODY_NAMES).  With --trace the pushes are recorded: push_step [P], push_body [P], push_impulse [P,3], push_delta_nu [P,K,27]."""
import argparse
import math
import os
import sys

import numpy as np
import torch

from . import ppo
from .envs import SteppingStoneVecEnv, make_camera
from .model import BODY_NAMES


def load_policy(path, device):
    """ActorCritic from a ppo.save_checkpoint file, a bare state_dict, or a reference legacy checkpoint."""
    try:
        ck = torch.load(path, map_location="cpu", weights_only=True)
    except Exception:
        from .legacy_checkpoint import load_reference_checkpoint
        return load_reference_checkpoint(path, device=device)
    if isinstance(ck, dict) and "state_dict" in ck:
        return ppo.load_checkpoint(path, device=device)[0]
    ens = len({k.split(".")[1] for k in ck if k.startswith("critics.")}) or 1
    ac = ppo.ActorCritic(num_ensembles=ens)
    ac.load_state_dict(ck)
    return ac.to(device)


def tile(frames):
    """[K, H, W, 3] -> one [rows * H, cols * W, 3] frame, cols = ceil(sqrt(K))."""
    k, h, w, _ = frames.shape
    cols = int(math.ceil(math.sqrt(k)))
    rows = (k + cols - 1) // cols
    out = np.zeros((rows * h, cols * w, 3), np.uint8)
    for i in range(k):
        r, c = divmod(i, cols)
        out[r * h:(r + 1) * h, c * w:(c + 1) * w] = frames[i]
    return out


def parse_push(text):
    """"STEP:BODY:px,py,pz" -> (step, body index, [px, py, pz])"""
    try:
        step, body, imp = text.split(":")
        p = [float(x) for x in imp.split(",")]
        b = BODY_NAMES.index(body) if body in BODY_NAMES else int(body)
        if len(p) != 3 or not 0 <= b < len(BODY_NAMES) or int(step) < 0:
            raise ValueError
    except ValueError:
        raise ValueError("--push takes STEP:BODY:px,py,pz with BODY an index in [0, %d) or one of %s, got %r" % (
            len(BODY_NAMES), ", ".join(BODY_NAMES), text)) from None
    return int(step), b, p


TRACE_KEYS = ("com", "com_vel", "corner_height", "corner_carrier")
FORCE_KEYS = ("contact_force", "joint_torque")


def run(env_id, net, envs=1, steps=300, curriculum=0, seed=1093, size=(320, 240), camera="track", device="cuda:0", out=None,
        log=print, trace=None, forces=False, pushes=()):
    """Roll the policy out deterministically; returns the [T, H, W, 3] uint8 animation (and writes it to `out` if given; the kinematic
    trace of the module docstring to `trace` if given)."""
    if forces and not trace:
        raise ValueError("forces=True needs a trace file to write to")
    pushes = [parse_push(p) if isinstance(p, str) else p for p in pushes]
    pushed = dict(push_step=[], push_body=[], push_impulse=[], push_delta_nu=[])
    ac = load_policy(net, device)
    ac.eval()
    env = SteppingStoneVecEnv(env_id, envs, seed=seed, device=device, return_numpy=False)
    env.update_curriculum(curriculum)
    cam = make_camera(camera)
    W, H = size
    log("Env: {}".format(env_id))
    log("Model: {}".format(os.path.basename(net)))
    frames = []
    rec = {k: [] for k in TRACE_KEYS + ("contact", "next_step_index", "done") + (FORCE_KEYS if forces else ())}
    try:
        obs = env.reset()
        ep_reward = torch.zeros(envs, dtype=torch.float64, device=env.device)
        for t in range(steps):
            for step, body, p in pushes:
                if step == t:
                    dnu = env.push(torch.tensor([p] * envs, dtype=torch.float32), body=body)
                    log("step %d: pushed %s by (%g, %g, %g) N s" % (t, BODY_NAMES[body], *p))
                    for k, v in zip(pushed, (step, body, p, dnu.cpu().numpy())):
                        pushed[k].append(v)
                    obs = env.get_obs()
            frames.append(tile(env.render("rgb_array", width=W, height=H, camera=cam).cpu().numpy()))
            with torch.no_grad():
                _, action, _ = ac.act(obs, deterministic=True)
            if forces:                     # before the step: a dry run of it from the current state
                dry = env.step_forces(action, next_state=False)
                as_np = lambda k: dry[k].cpu().numpy()
                rec["contact_force"].append(np.concatenate([as_np("contact_slot")[..., None].astype(np.float32), as_np("contact_pen")[..., None],
                                                            as_np("contact_force"), as_np("contact_force_world")], -1))
                rec["joint_torque"].append(as_np("joint_torque"))
            obs, rew, done, _ = env.step(action)
            ep_reward += rew.double()
            if trace:
                kin = env.kinematics(twists=False)
                for k in TRACE_KEYS:
                    rec[k].append(kin[k].cpu().numpy())
                rec["contact"].append(obs[:, 48:50].cpu().numpy() > 0.5)
                rec["next_step_index"].append(env.next_step_index)
                rec["done"].append(done.cpu().numpy().astype(bool))
            if bool(done.any()):
                for i in torch.nonzero(done).flatten().tolist():
                    log("Episode reward: {}".format(float(ep_reward[i])) + ("" if envs == 1 else "  (env {})".format(i)))
                    ep_reward[i] = 0
    finally:
        env.close()
    anim = np.stack(frames)
    if trace:
        if not trace.endswith(".npz"):
            trace += ".npz"
        if pushes:
            rec.update(pushed)
        np.savez(trace, **{k: np.stack(v) if v else np.zeros(0) for k, v in rec.items()})
        log("wrote %s (%d steps x %d envs)" % (trace, len(rec["done"]), envs))
    if out:
        save(anim, out, log)
    return anim


def save(anim, out, log=print):
    if out.endswith(".gif"):
        try:
            from PIL import Image
        except ImportError:
            out = out[:-4] + ".npy"
            log("PIL is not importable: writing the frames as %s" % out)
        else:
            imgs = [Image.fromarray(f) for f in anim]
            imgs[0].save(out, save_all=True, append_images=imgs[1:], duration=33, loop=0)
            log("wrote %s (%d frames)" % (out, len(imgs)))
            return out
    if not out.endswith(".npy"):
        out += ".npy"
    np.save(out, anim)
    log("wrote %s %s" % (out, anim.shape))
    return out


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--env", default="Walker3DStepperEnv-v0")
    p.add_argument("--net", required=True, help="ppo.save_checkpoint file, ActorCritic state_dict, or reference legacy .pt")
    p.add_argument("--envs", type=int, default=1)
    p.add_argument("--steps", type=int, default=300)
    p.add_argument("--curriculum", type=int, default=0)
    p.add_argument("--seed", type=int, default=1093)
    p.add_argument("--size", default="320x240", help="WxH, multiples of 4")
    p.add_argument("--camera", choices=("track", "chase"), default="track")
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--out", default="enjoy.gif", help=".gif (needs PIL) or .npy")
    p.add_argument("--trace", default=None, metavar="FILE.npz", help="also write COM, sole-corner heights / carriers, contact flags per step")
    p.add_argument("--forces", action="store_true", help="with --trace: also write contact forces and applied joint torques per substep")
    p.add_argument("--push", action="append", default=[], metavar="STEP:BODY:px,py,pz",
                   help="shove BODY (index or name) of every env by a linear impulse in N s before control step STEP; repeatable")
    a = p.parse_args(argv)
    if a.forces and not a.trace:
        p.error("--forces needs --trace")
    w, h = (int(x) for x in a.size.lower().split("x"))
    run(a.env, a.net, a.envs, a.steps, a.curriculum, a.seed, (w, h), a.camera, a.device, a.out, trace=a.trace, forces=a.forces,
        pushes=a.push)
    return 0


if __name__ == "__main__":
    sys.exit(main())
