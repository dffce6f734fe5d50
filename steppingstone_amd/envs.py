"""Host-side mirror of the reference's env / vec-env protocol for the stepping-stone hot path.

Drop-in surface (names, argument meaning, error behaviour) follows what `playground/train.py` and
`playground/enjoy.py` of the reference consume through `common/envs_utils.py`:

  make_env(env_id)                      common/envs_utils.py:43-45
  make_vec_envs(env_id, seed, n, dir)   common/envs_utils.py:48-56
  VecEnv.reset/step_async/step_wait/step, update_curriculum, update_specialist, update_sample_prob,
  create_temp_states, set_mirror, set_env_params, set_robot_params, close   common/envs_utils.py:542-606

Instead of N worker processes with pipes and shared memory, all N environments live in HBM on one MI355X and one
kernel launch advances them together.  PyTorch is plumbing only (device buffers + current stream); the arithmetic
is in libsteppingstone.so (hand-written HIP).  There is NO CPU implementation in this package.
"""
import ctypes as C
import time
import types

import numpy as np
import torch

from . import _lib
from ._lib import ACT_DIM, GRID, INFO_WORDS, MAX_EPISODE_STEPS, NCELL, NUM_STONES, OBS_DIM, STATE_DIM, SteppingStoneError
from .model import BODY_NAMES

DEG = np.pi / 180.0
ENV_KINDS = {
    "Walker3DStepperEnv-v0": _lib.WALKER3D, "mocca_envs:Walker3DStepperEnv-v0": _lib.WALKER3D,
    "MikeStepperEnv-v0": _lib.MIKE, "mocca_envs:MikeStepperEnv-v0": _lib.MIKE,
}
_EMPTY_INFO = types.MappingProxyType({})


class Box:
    """Minimal stand-in for gym.spaces.Box (gym is not a dependency): shape/dtype/low/high."""

    def __init__(self, low, high, shape, dtype=np.float32):
        self.shape = tuple(shape)
        self.dtype = np.dtype(dtype)
        self.low = np.full(self.shape, low, self.dtype)
        self.high = np.full(self.shape, high, self.dtype)

    def sample(self):
        lo = np.where(np.isfinite(self.low), self.low, -1.0)
        hi = np.where(np.isfinite(self.high), self.high, 1.0)
        return np.random.uniform(lo, hi).astype(self.dtype)

    def __repr__(self):
        return "Box%s" % (self.shape,)


class EnvSpec:
    def __init__(self, env_id):
        self.id = env_id
        self.max_episode_steps = MAX_EPISODE_STEPS


def kind_of(env_id):
    if env_id not in ENV_KINDS:
        raise SteppingStoneError("unknown env id %r (known: %s)" % (env_id, ", ".join(sorted(ENV_KINDS))))
    return ENV_KINDS[env_id]


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class HipBackend:
    """Owns one ss_env handle on one GPU.  All tensor arguments must be contiguous tensors on `self.device`."""

    def __init__(self, kind, num_envs, seed, device, env_id_offset=0):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise SteppingStoneError("no GPU visible to torch: the stepping-stone env runs on MI355X only "
                                     "(there is no CPU fallback)")
        self.device = torch.device(device if device is not None else "cuda:0")
        if self.device.type != "cuda":
            raise SteppingStoneError("device must be a cuda (HIP) device, got %s" % (self.device,))
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        self.n = int(num_envs)
        h = C.c_void_p()
        _lib.check(self.lib.ss_create(C.byref(h), int(kind), self.n, idx, int(seed) & (2 ** 64 - 1), int(env_id_offset)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.ss_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, obs):
        _lib.check(self.lib.ss_reset(self.h, _ptr(obs), _stream(self.device)))

    def step(self, act, obs, rew, done, info):
        _lib.check(self.lib.ss_step(self.h, _ptr(act), _ptr(obs), _ptr(rew), _ptr(done), _ptr(info), _stream(self.device)))

    def rollout_random(self, num_steps, t0, obs, rew, done, info, steps_per_launch=0):
        _lib.check(self.lib.ss_rollout_random(self.h, int(num_steps), int(steps_per_launch), int(t0), _ptr(obs), _ptr(rew),
                                              _ptr(done), _ptr(info), _stream(self.device)))

    def step_packed(self, act, use_random, t, packed, info):
        _lib.check(self.lib.ss_step_packed(self.h, _ptr(act) if act is not None else None, 1 if use_random else 0, int(t),
                                           _ptr(packed), _ptr(info), _stream(self.device)))

    def rollout_random_packed(self, num_steps, t0, packed, info):
        _lib.check(self.lib.ss_rollout_random_packed(self.h, int(num_steps), int(t0), _ptr(packed), _ptr(info), _stream(self.device)))

    def random_actions(self, t, act):
        _lib.check(self.lib.ss_random_actions(self.h, int(t), _ptr(act), _stream(self.device)))

    def set_curriculum(self, level):
        _lib.check(self.lib.ss_set_curriculum(self.h, int(level)))

    def set_specialist(self, level):
        _lib.check(self.lib.ss_set_specialist(self.h, int(level)))

    def set_sample_prob(self, prob, per_env):
        prob = np.ascontiguousarray(prob, np.float64)
        _lib.check(self.lib.ss_set_sample_prob(self.h, prob.ctypes.data_as(C.c_void_p), 1 if per_env else 0))

    def set_sample_prob_device(self, prob, per_env):
        _lib.check(self.lib.ss_set_sample_prob_device(self.h, _ptr(prob), 1 if per_env else 0, _stream(self.device)))

    def set_mirror(self, on):
        _lib.check(self.lib.ss_set_mirror(self.h, 1 if on else 0))

    def set_power(self, power):
        _lib.check(self.lib.ss_set_power(self.h, float(power)))

    def set_auto_reset(self, on):
        _lib.check(self.lib.ss_set_auto_reset(self.h, 1 if on else 0))

    def create_temp_states(self, out):
        _lib.check(self.lib.ss_create_temp_states(self.h, _ptr(out), _stream(self.device)))

    def get_state(self, packed):
        _lib.check(self.lib.ss_get_state(self.h, _ptr(packed), _stream(self.device)))

    def set_state(self, packed):
        _lib.check(self.lib.ss_set_state(self.h, _ptr(packed), _stream(self.device)))

    def get_obs(self, obs):
        _lib.check(self.lib.ss_get_obs(self.h, _ptr(obs), _stream(self.device)))

    def reset_masked(self, mask, obs, terminal=None):
        """mask: uint8 device tensor [N]; obs: None, [N,60] or the [N,62] packed block; terminal: None or [N,60]."""
        opt = lambda t: _ptr(t) if t is not None else None
        stride = OBS_DIM if obs is None else int(obs.stride(0))
        _lib.check(self.lib.ss_reset_masked(self.h, _ptr(mask), opt(obs), stride, opt(terminal), _stream(self.device)))

    def get_state_envs(self, env_ids, packed):
        """env_ids: int32 device tensor [M] of checked ids; packed: [M,186]."""
        _lib.check(self.lib.ss_get_state_envs(self.h, _ptr(env_ids), int(env_ids.numel()), _ptr(packed), _stream(self.device)))

    def set_state_envs(self, env_ids, packed):
        _lib.check(self.lib.ss_set_state_envs(self.h, _ptr(env_ids), int(env_ids.numel()), _ptr(packed), _stream(self.device)))

    def body_poses(self, out):
        _lib.check(self.lib.ss_body_poses(self.h, _ptr(out), _stream(self.device)))

    def kinematics(self, env_ids, m, body_twist, summary, corners):
        """env_ids: int32 device tensor [m], or None for envs 0..m-1 (m == N); body_twist [m,22,6] / summary [m,12] / corners [m,8,8]:
        float32 device tensors or None, not all three (docs/PHYSICS.md 9)."""
        opt = lambda t: _ptr(t) if t is not None else None
        _lib.check(self.lib.ss_kinematics(self.h, opt(env_ids), int(m), opt(body_twist), opt(summary), opt(corners), _stream(self.device)))

    def step_forces(self, env_ids, m, act, contacts, joints, next_state):
        """env_ids: int32 device tensor [m], or None for envs 0..m-1 (m == N); act [m,21]; contacts [m,4,8,8] / joints [m,4,4,21] /
        next_state [m,56]: float32 device tensors or None, not all three (docs/PHYSICS.md 10)."""
        opt = lambda t: _ptr(t) if t is not None else None
        _lib.check(self.lib.ss_step_forces(self.h, opt(env_ids), int(m), _ptr(act), opt(contacts), opt(joints), opt(next_state),
                                           _stream(self.device)))

    def eom(self, env_ids, m, mass, forces, corner_jac):
        """env_ids: int32 device tensor [m], or None for envs 0..m-1 (m == N); mass [m,27,27] / forces [m,3,27] / corner_jac [m,8,3,27]:
        float32 device tensors or None, not all three (docs/PHYSICS.md 11)."""
        opt = lambda t: _ptr(t) if t is not None else None
        _lib.check(self.lib.ss_eom(self.h, opt(env_ids), int(m), opt(mass), opt(forces), opt(corner_jac), _stream(self.device)))

    def push(self, env_ids, m, body, point, impulse, delta_nu, apply):
        """env_ids: int32 device tensor [m], or None for envs 0..m-1 (m == N); body: int32 device tensor [m] or None (the torso);
        point [m,3] or None (the centre of mass); impulse [m,6]; delta_nu [m,27] or None (only with apply): float32 device tensors
        (docs/PHYSICS.md 12)."""
        opt = lambda t: _ptr(t) if t is not None else None
        _lib.check(self.lib.ss_push(self.h, opt(env_ids), int(m), opt(body), opt(point), _ptr(impulse), opt(delta_nu), 1 if apply else 0,
                                    _stream(self.device)))

    def lookahead(self, env_ids, m, horizon, act, obs, rew, done, final_state, work):
        """env_ids: int32 device tensor [m] (repeats welcome), or None for envs 0..m-1 (m == N); act [m,H,21]; obs [m,H,60] or None, rew
        [m,H], final_state [m,186] or None, work [m, LOOK_WORK]: float32 device tensors; done [m,H] uint8 (docs/PHYSICS.md 13)."""
        opt = lambda t: _ptr(t) if t is not None else None
        _lib.check(self.lib.ss_lookahead(self.h, opt(env_ids), int(m), int(horizon), _ptr(act), opt(obs), _ptr(rew), _ptr(done),
                                         opt(final_state), _ptr(work), _stream(self.device)))

    def lookahead_states(self, env_ids, m, states, horizon, act, obs, rew, done, final_state, work):
        """lookahead() with row k starting from states[k] ([m,186] float32 device tensor) instead of env env_ids[k]'s current state
        (docs/PHYSICS.md 13, "Branches from caller-supplied states")."""
        opt = lambda t: _ptr(t) if t is not None else None
        _lib.check(self.lib.ss_lookahead_states(self.h, opt(env_ids), int(m), _ptr(states), int(horizon), _ptr(act), opt(obs), _ptr(rew),
                                                _ptr(done), opt(final_state), _ptr(work), _stream(self.device)))

    def get_obs_states(self, m, states, obs):
        """states [m,186] -> obs [m,60]: float32 device tensors; the observation of each state row (docs/PHYSICS.md 13)."""
        _lib.check(self.lib.ss_get_obs_states(self.h, int(m), _ptr(states), _ptr(obs), _stream(self.device)))

    def policy_pack(self, desc, weights, biases, packed):
        """desc: _lib.PolicyDesc; weights / biases: one contiguous float32 device tensor per layer ([out,in] / [out]); packed: float32
        device tensor of ss_policy_words(desc) words (docs/PHYSICS.md 14).  Stream-ordered: a later change of the weights needs a new call."""
        n = int(desc.layers)
        wp = (C.c_void_p * n)(*[_ptr(w) for w in weights])
        bp = (C.c_void_p * n)(*[_ptr(b) for b in biases])
        _lib.check(self.lib.ss_policy_pack(self.h, C.byref(desc), wp, bp, _ptr(packed), _stream(self.device)))

    def lookahead_policy(self, env_ids, m, states, horizon, desc, packed, offsets, act, obs, rew, done, final_state, work):
        """lookahead() / lookahead_states() (states None / [m,186]) with the actions computed in the launch by the packed MLP; offsets
        [m,H,21] or None is added to them, act [m,H,21] or None receives them (docs/PHYSICS.md 14)."""
        opt = lambda t: _ptr(t) if t is not None else None
        _lib.check(self.lib.ss_lookahead_policy(self.h, opt(env_ids), int(m), opt(states), int(horizon), C.byref(desc), _ptr(packed),
                                                opt(offsets), opt(act), opt(obs), _ptr(rew), _ptr(done), opt(final_state), _ptr(work),
                                                _stream(self.device)))

    def render(self, env_ids, width, height, camera, rgb, depth, seg):
        """env_ids: int32 device tensor [M]; rgb / depth / seg: device tensors or None (docs/RENDER.md)."""
        opt = lambda t: _ptr(t) if t is not None else None
        _lib.check(self.lib.ss_render(self.h, _ptr(env_ids), int(env_ids.numel()), int(width), int(height), C.byref(camera),
                                      opt(rgb), opt(depth), opt(seg), _stream(self.device)))


POLICY_SOURCES = ("a ppo.Actor, a ppo.ActorCritic (its actor), an nn.Sequential of nn.Linear each followed by at most one of nn.ReLU / "
                  "nn.Softsign / nn.Tanh / nn.Identity, or a list of (weight [out,in], bias [out], activation) triples with activation one "
                  "of 'identity', 'relu', 'softsign', 'tanh'; %d -> ... -> %d, at most %d layers, at most %d wide"
                  % (OBS_DIM, ACT_DIM, _lib.POLICY_MAX_LAYERS, _lib.POLICY_MAX_WIDTH))
_POLICY_ACT = {"identity": _lib.POLICY_IDENTITY, "relu": _lib.POLICY_RELU, "softsign": _lib.POLICY_SOFTSIGN, "tanh": _lib.POLICY_TANH}


def _policy_layers(source):
    """source -> list of (weight, bias, activation code); weight / bias: tensors, parameters or arrays, read again by every refresh()"""
    nn = torch.nn
    from . import ppo
    if isinstance(source, ppo.ActorCritic):
        source = source.actor
    if isinstance(source, ppo.Actor):
        s = source
        return [(s.fc1.weight, s.fc1.bias, _lib.POLICY_SOFTSIGN), (s.fc2.weight, s.fc2.bias, _lib.POLICY_SOFTSIGN),
                (s.fc3.weight, s.fc3.bias, _lib.POLICY_SOFTSIGN), (s.fc4.weight, s.fc4.bias, _lib.POLICY_RELU),
                (s.fc5.weight, s.fc5.bias, _lib.POLICY_RELU), (s.out.weight, s.out.bias, _lib.POLICY_TANH)]
    kinds = {nn.ReLU: _lib.POLICY_RELU, nn.Softsign: _lib.POLICY_SOFTSIGN, nn.Tanh: _lib.POLICY_TANH, nn.Identity: _lib.POLICY_IDENTITY}
    if isinstance(source, nn.Sequential):
        out = []
        for mod in source:
            if isinstance(mod, nn.Linear):
                if mod.bias is None:
                    raise ValueError("pack_policy: a Linear without bias is not supported; supported: " + POLICY_SOURCES)
                out.append([mod.weight, mod.bias, None])
            elif type(mod) in kinds and out and out[-1][2] is None:
                out[-1][2] = kinds[type(mod)]
            else:
                raise ValueError("pack_policy: %s at this place is not supported; supported: %s" % (type(mod).__name__, POLICY_SOURCES))
        return [(w, b, _lib.POLICY_IDENTITY if a is None else a) for w, b, a in out]
    if isinstance(source, (list, tuple)) and source and all(isinstance(t, (list, tuple)) and len(t) == 3 for t in source):
        out = []
        for w, b, a in source:
            if not (isinstance(a, str) and a in _POLICY_ACT):
                raise ValueError("pack_policy: activation %r is not supported; supported: %s" % (a, POLICY_SOURCES))
            out.append((w, b, _POLICY_ACT[a]))
        return out
    raise ValueError("pack_policy: %s is not supported; supported: %s" % (type(source).__name__, POLICY_SOURCES))


class PackedPolicy:
    """A frozen MLP in the form the closed-loop look-ahead reads (SteppingStoneVecEnv.lookahead_policy): `desc` (_lib.PolicyDesc) and
    `blob`, a float32 tensor on `device` whose layout is the library's own.  refresh() repacks from the same modules / arrays after their
    values changed (a stream-ordered kernel launch: it can be captured into a graph together with the look-ahead, and a replay then
    repacks from the parameters' current values, provided they are float32 tensors on the device already).  The repack is a call of the
    library on an env's handle: a policy made with a torch device is packed when an env first uses it, one made with an env at once."""

    def __init__(self, source, device):
        env = device if hasattr(device, "backend") or hasattr(device, "vec") else None
        if env is not None:
            env = getattr(env, "vec", env)
            device = env.device
        self.device = torch.device(device)
        self._layers = _policy_layers(source)
        shapes = [(tuple(w.shape), tuple(b.shape)) for w, b, _ in self._layers]
        if any(len(ws) != 2 or bs != (ws[0],) for ws, bs in shapes):
            raise ValueError("pack_policy: a layer is weight [out,in] and bias [out], got %s; supported: %s" % (shapes, POLICY_SOURCES))
        if len(shapes) > _lib.POLICY_MAX_LAYERS or any(shapes[i][0][1] != shapes[i - 1][0][0] for i in range(1, len(shapes))):
            raise ValueError("pack_policy: the layers do not chain: %s; supported: %s" % ([ws for ws, _ in shapes], POLICY_SOURCES))
        d = _lib.PolicyDesc()
        d.layers = len(shapes)
        d.width[0] = shapes[0][0][1]
        for i, ((wo, _), _) in enumerate(shapes):
            d.width[i + 1] = wo
            d.activation[i] = self._layers[i][2]
        words = int(_lib.load().ss_policy_words(C.byref(d)))
        if words < 0:
            raise ValueError("pack_policy: widths %s are not supported; supported: %s" % (list(d.width[:d.layers + 1]), POLICY_SOURCES))
        self.desc = d
        self.blob = torch.zeros(words, dtype=torch.float32, device=self.device)
        self._backend, self._fresh, self._held = None, False, None
        if env is not None:
            self.bind(env.backend)

    def _arrays(self):
        """the layers' current values as contiguous float32 tensors on the device: the parameters themselves where they are that already"""
        give = lambda t: (t.detach() if torch.is_tensor(t) else torch.as_tensor(np.array(t, dtype=np.float32))).to(self.device, torch.float32).contiguous()
        return [give(w) for w, _, _ in self._layers], [give(b) for _, b, _ in self._layers]

    def refresh(self):
        """repack after the weights changed (now if an env has used the policy already, else at its first use)"""
        if self._backend is None:
            self._fresh = False
            return self
        ws, bs = self._arrays()
        self._held = (ws, bs)            # the launch reads them asynchronously
        self._backend.policy_pack(self.desc, ws, bs, self.blob)
        self._fresh = True
        return self

    def bind(self, backend):
        if self._backend is not backend or not self._fresh:
            self._backend = backend
            self.refresh()
        return self


def pack_policy(source, device):
    """PackedPolicy of `source`: """ + POLICY_SOURCES + """.  device: a torch device, or the env that will use the policy."""
    return PackedPolicy(source, device)


CAMERA_MODES = {"track": _lib.CAM_TRACK, "chase": _lib.CAM_CHASE, "fixed": _lib.CAM_FIXED}


def make_camera(mode="track", eye=None, target=None, fov_y_deg=None, far_m=None, shadows=True):
    """An ss_camera (docs/RENDER.md 1): mode "track" (default) / "chase" take eye and target as offsets (target from the torso, eye from
    the target; "chase" turns both by the torso's yaw), "fixed" takes them in world coordinates.  Unset fields keep the defaults."""
    cam = _lib.default_camera()
    cam.mode = CAMERA_MODES[mode] if isinstance(mode, str) else int(mode)
    if eye is not None:
        cam.eye[:] = [float(x) for x in eye]
    if target is not None:
        cam.target[:] = [float(x) for x in target]
    if fov_y_deg is not None:
        cam.fov_y_deg = float(fov_y_deg)
    if far_m is not None:
        cam.far_m = float(far_m)
    cam.flags = _lib.CAM_SHADOWS if shadows else 0
    return cam


class SteppingStoneVecEnv:
    """N stepping-stone environments advanced by one HIP kernel launch per step.

    return_numpy=True reproduces the reference's ShmemVecEnv return types exactly (obs float32 (N,60) ndarray,
    rews float64 (N,), dones bool (N,), infos sequence of N dicts; common/envs_utils.py:555-558) so that
    playground/train.py consumes it unchanged; return_numpy=False keeps everything on the GPU (obs/rew/done
    tensors, infos as a dict of tensors) for a device-resident PPO loop.

    keep_terminal_obs=True keeps auto-reset's results bit for bit and also returns the observation each finished env ended in:
    the kernel steps with its auto-reset off and ss_reset_masked resets the finished envs behind it on the same stream, copying
    their rows out first.  Tensor mode: info["terminal_obs"] [N,60] (rows where done is set are meaningful); numpy mode:
    infos[i]["terminal_observation"], a float32 (60,) array, for the finished envs only (the gymnasium / Stable-Baselines3 keys).
    """

    closed = False

    def __init__(self, env_id, num_envs, seed=0, device=None, env_id_offset=0, return_numpy=False, backend=None, log_dir=None,
                 keep_terminal_obs=False):
        self.env_id = env_id
        self.kind = kind_of(env_id)
        self.num_envs = int(num_envs)
        self.seed_value = int(seed)
        self.return_numpy = bool(return_numpy)
        self.spec = EnvSpec(env_id)
        high = np.inf
        self.observation_space = Box(-high, high, (OBS_DIM,), np.float32)
        self.action_space = Box(-1.0, 1.0, (ACT_DIM,), np.float32)
        # `backend` is a test seam (tests inject an oracle-backed object); the product path is always HIP.
        self.backend = backend if backend is not None else HipBackend(self.kind, num_envs, seed, device, env_id_offset)
        dev = self.backend.device
        self.device = dev
        n = self.num_envs
        self._obs = torch.zeros((n, OBS_DIM), dtype=torch.float32, device=dev)
        self._rew = torch.zeros((n,), dtype=torch.float32, device=dev)
        self._done = torch.zeros((n,), dtype=torch.uint8, device=dev)
        self._info = torch.zeros((n, INFO_WORDS), dtype=torch.int32, device=dev)
        self._act = torch.zeros((n, ACT_DIM), dtype=torch.float32, device=dev)
        self._pending = False
        # numpy drop-in mode on a GPU: pinned staging buffers, one H->D copy of the actions and one D->H copy of the
        # packed [N,62] = obs | rew | done block per step (instead of four pageable copies)
        self._pinned = None
        if self.return_numpy and torch.device(dev).type == "cuda":
            self._pinned = {"act": torch.zeros((n, ACT_DIM), dtype=torch.float32).pin_memory(),
                            "out": torch.zeros((n, OBS_DIM + 2), dtype=torch.float32).pin_memory(),
                            "dev": torch.zeros((n, OBS_DIM + 2), dtype=torch.float32, device=dev),
                            "info": torch.zeros((n, INFO_WORDS), dtype=torch.int32).pin_memory(),
                            "event": torch.cuda.Event()}
        self.keep_terminal_obs = bool(keep_terminal_obs)
        self._terminal = None
        if self.keep_terminal_obs:
            self.backend.set_auto_reset(False)       # step() / step_packed() reset the finished envs behind each step
            self._terminal = torch.zeros((n, OBS_DIM), dtype=torch.float32, device=dev)
        self._tstart = time.time()
        # Monitor's files (common/envs_utils.py:36-38,172-194): <log_dir>/<rank>.monitor.csv per env, a row per finished episode
        self._monitor = None
        if log_dir is not None:
            from .monitor_csv import MonitorFiles
            self._monitor = MonitorFiles(log_dir, self.num_envs, env_id, first_rank=env_id_offset, t_start=self._tstart)
        self.yaw_samples = np.linspace(-20.0, 20.0, GRID) * DEG
        self.pitch_samples = np.linspace(-30.0, 30.0, GRID) * DEG
        self.yaw_sample_size = GRID
        self.pitch_sample_size = GRID
        self._max_episode_steps = MAX_EPISODE_STEPS
        self.curriculum = 0

    # ------------------------------------------------------------------ gym / VecEnv protocol
    def reset(self, env_ids=None):
        """Reset all envs (env_ids=None) and return their observations [N,60], or reset only the envs env_ids names:
          * a host int sequence / ndarray, or an int tensor (checked on the host: one sync for a device tensor) -- returns the
            fresh observations of those envs as [m,60], rows in env_ids order;
          * a mask: a bool or uint8 tensor of shape [N] (e.g. the done of step()) -- never read on the host, so the call does not
            synchronise and can be captured into a graph; returns the [N,60] observations of all envs, the masked rows fresh.
        Out-of-range or duplicate ids and a mask of the wrong shape raise ValueError before anything runs on the GPU.  The env's own
        obs buffer (the tensor step() returns in tensor mode) gets the fresh rows in place.  A reset env starts a new episode from its
        own random stream, exactly as an auto-reset inside step() would.  Resetting an env in mid-episode writes no Monitor row: the
        dropped episode is not reported, as in the reference, where it never finishes."""
        if self._pending:
            print("Called reset() while waiting for the step to complete")
            self.step_wait()
        if env_ids is None:
            self.backend.reset(self._obs)
            return self._out_obs()
        mask, ids = self._env_ids(env_ids, allow_mask=True)
        if mask is not None:
            self.backend.reset_masked(mask, self._obs)
            return self._out_obs()
        dev_ids = torch.from_numpy(ids).to(self.device)
        if ids.size:
            m = np.zeros(self.num_envs, np.uint8)
            m[ids] = 1
            self.backend.reset_masked(torch.from_numpy(m).to(self.device), self._obs)
        rows = self._obs.index_select(0, dev_ids)
        return rows.cpu().numpy() if self.return_numpy else rows

    def set_auto_reset(self, on):
        """on (default): an env that finishes is reset inside step() (the reference's worker, common/envs_utils.py:646-649).  off:
        step() returns the terminal observation of a finished env, which stays finished until reset(done) (or reset(ids)) resets it.
        With keep_terminal_obs=True the envs already reset themselves and return the terminal rows: turning it off raises ValueError."""
        if self.keep_terminal_obs:
            if not on:
                raise ValueError("set_auto_reset(False) on an env made with keep_terminal_obs=True: that env resets its finished envs "
                                 "itself; make it with keep_terminal_obs=False to reset them with reset(done)")
            return
        self.backend.set_auto_reset(bool(on))

    def step_async(self, actions):
        if self._pinned is not None and not torch.is_tensor(actions):
            pb = self._pinned
            a = np.asarray(actions, dtype=np.float32)
            assert a.shape[0] == self.num_envs, "expected %d actions, got %d" % (self.num_envs, a.shape[0])
            pb["act"].numpy()[...] = a.reshape(self.num_envs, ACT_DIM)
            self._act.copy_(pb["act"], non_blocking=True)
            self.backend.step_packed(self._act, False, 0, pb["dev"], self._info)
            if self.keep_terminal_obs:
                self._done.copy_(pb["dev"][:, OBS_DIM + 1])          # the block's done column (0 / 1) as the u8 mask
                self.backend.reset_masked(self._done, pb["dev"], self._terminal)
            pb["out"].copy_(pb["dev"], non_blocking=True)
            pb["info"].copy_(self._info, non_blocking=True)      # the step report travels with the block: no second, synchronous copy
            pb["event"].record()
            self._pending = "pinned"
            return
        if torch.is_tensor(actions):
            a = actions.to(device=self.device, dtype=torch.float32)
        else:
            a = torch.from_numpy(np.ascontiguousarray(actions, dtype=np.float32)).to(self.device)
        assert a.shape[0] == self.num_envs, "expected %d actions, got %d" % (self.num_envs, a.shape[0])
        self._act.copy_(a.reshape(self.num_envs, ACT_DIM))
        self.backend.step(self._act, self._obs, self._rew, self._done, self._info)
        if self.keep_terminal_obs:
            self.backend.reset_masked(self._done, self._obs, self._terminal)
        self._pending = True

    def step_wait(self):
        if self._pending == "pinned":
            self._pending = False
            pb = self._pinned
            pb["event"].synchronize()
            out = pb["out"].numpy()
            obs = out[:, :OBS_DIM].copy()                       # fresh arrays every step, like common/envs_utils.py:619
            rew = out[:, OBS_DIM].astype(np.float64)
            done = out[:, OBS_DIM + 1] > 0.5
            self._info_host = pb["info"].numpy()
            return obs, rew, done, self._terminal_infos(done, self._info_dicts(done, self._info_host))
        self._pending = False
        if not self.return_numpy:
            if self._monitor is not None:      # opt-in (log_dir): the episode rows need the finished envs on the host every step
                self._info_dicts(self._done.cpu().numpy().astype(bool))
            info = self._info_tensors()
            if self.keep_terminal_obs:
                info["terminal_obs"] = self._terminal
            return self._obs, self._rew, self._done.bool(), info
        obs = self._obs.cpu().numpy()
        rew = self._rew.cpu().numpy().astype(np.float64)
        done = self._done.cpu().numpy().astype(bool)
        self._info_host = self._info.cpu().numpy()
        return obs, rew, done, self._terminal_infos(done, self._info_dicts(done, self._info_host))

    def _terminal_infos(self, done, infos):
        """keep_terminal_obs, numpy mode: infos[i]["terminal_observation"] for the finished envs; their rows travel to the host in
        steps where an env finished only."""
        idx = np.nonzero(done)[0]
        if not self.keep_terminal_obs or not idx.size:
            return infos
        rows = self._terminal.index_select(0, torch.from_numpy(idx).to(self.device)).cpu().numpy()
        for k, i in enumerate(idx.tolist()):
            infos[i]["terminal_observation"] = rows[k]
        return infos

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def rollout_random(self, num_steps, t0=0, steps_per_launch=0):
        """BASELINE metric path: num_steps control steps with on-device U(-1,1) actions (Philox stream 1),
        steps_per_launch of them per kernel launch (0: the library default of 1000; 1: one launch per step)."""
        self._no_multi_step()
        self.backend.rollout_random(num_steps, t0, self._obs, self._rew, self._done, self._info, steps_per_launch)
        return self._obs, self._rew, self._done

    def step_packed(self, packed, actions=None, t=0, info=None):
        """One step written into the caller's [N,62] buffer (obs | rew | done): the block ShardedVecEnv all-gathers.
        actions=None draws them from the benchmark Philox stream at index t.  info: optional caller-owned [N,5] int32
        buffer for the per-env step report (default: this env's own).  keep_terminal_obs: the finished envs are reset into the
        block behind the step (their terminal rows: self._terminal)."""
        if actions is not None:
            self._act.copy_(actions.reshape(self.num_envs, ACT_DIM))
        self.backend.step_packed(self._act if actions is not None else None, actions is None, t, packed,
                                 self._info if info is None else info)
        if self.keep_terminal_obs:
            self._done.copy_(packed[:, OBS_DIM + 1])
            self.backend.reset_masked(self._done, packed, self._terminal)
        return packed

    def rollout_random_packed(self, packed, t0=0):
        """packed: [K, N, 62] device buffer; ONE launch advances K control steps and writes step k's obs | rew | done block at
        packed[k] (the multi-GPU rollout ships such a chunk per collective)."""
        assert packed.dim() == 3 and packed.shape[1] == self.num_envs and packed.shape[2] == OBS_DIM + 2 and packed.is_contiguous()
        self._no_multi_step()
        self.backend.rollout_random_packed(packed.shape[0], t0, packed, self._info)
        return packed

    def _no_multi_step(self):
        if self.keep_terminal_obs:
            raise ValueError("keep_terminal_obs=True resets the finished envs behind each step; a multi-step rollout launch has no "
                             "place for that: use step() / step_packed(), or an env made with keep_terminal_obs=False")

    def random_actions(self, t):
        self.backend.random_actions(t, self._act)
        return self._act.clone()

    def close(self):
        if self.closed:
            return
        if self._monitor is not None:
            self._monitor.close()
        self.backend.close()
        self.closed = True

    def render(self, mode="rgb_array", env_ids=None, width=256, height=192, camera=None, depth=False, seg=False, rgb=True):
        """Frames of the envs `env_ids` (default: all) drawn on the GPU (docs/RENDER.md): rgb [M,H,W,3] uint8, depth [M,H,W] float32
        (z-depth, background = far), seg [M,H,W] uint8 (0 background, 1 + body, 23 / 24 / 25 stones n-1 / n / n+1).  Returns the one
        output requested, else a tuple in the order rgb, depth, seg; tensors on the env's device, numpy arrays in numpy mode.
        camera: None (the default TRACK camera), an ss_camera (make_camera) or a dict of make_camera's arguments.  There is no window:
        mode="human" raises NotImplementedError."""
        if mode != "rgb_array":
            raise NotImplementedError("render(mode=%r): only mode='rgb_array' is supported (there is no GUI)" % (mode,))
        if not hasattr(self.backend, "render"):
            raise NotImplementedError("this backend does not render")
        if env_ids is None:
            ids = torch.arange(self.num_envs, dtype=torch.int32, device=self.device)
        else:
            ids = torch.as_tensor(env_ids).reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
        if camera is None:
            camera = make_camera()
        elif isinstance(camera, dict):
            camera = make_camera(**camera)
        m = int(ids.numel())
        out_rgb = torch.empty((m, height, width, 3), dtype=torch.uint8, device=self.device) if rgb else None
        out_depth = torch.empty((m, height, width), dtype=torch.float32, device=self.device) if depth else None
        out_seg = torch.empty((m, height, width), dtype=torch.uint8, device=self.device) if seg else None
        self.backend.render(ids, width, height, camera, out_rgb, out_depth, out_seg)
        outs = [t for t in (out_rgb, out_depth, out_seg) if t is not None]
        if self.return_numpy:
            outs = [t.cpu().numpy() for t in outs]
        return outs[0] if len(outs) == 1 else tuple(outs)

    def get_images(self, width=256, height=192):
        """VecEnv.get_images: one (H, W, 3) uint8 numpy frame per env (default camera)."""
        if not hasattr(self.backend, "render"):
            raise NotImplementedError("this backend does not render")
        frames = self.render("rgb_array", width=width, height=height)
        frames = frames.cpu().numpy() if torch.is_tensor(frames) else frames
        return list(frames)

    def body_poses(self):
        """World pose of every body of every env, [N, 22, 12] float32: position | R row-major (model.fk's frames)."""
        out = torch.empty((self.num_envs, _lib.NUM_BODIES, 12), dtype=torch.float32, device=self.device)
        self.backend.body_poses(out)
        return out.cpu().numpy() if self.return_numpy else out

    def kinematics(self, env_ids=None, twists=True, summary=True, corners=True):
        """Whole-body kinematics of the envs env_ids names (default: all; the forms of get_state()), read on the GPU from the current
        state (docs/PHYSICS.md 9; world frame).  Returns a dict of tensors on the env's device (numpy arrays in numpy mode), m rows in
        env_ids order, holding the groups asked for:
          twists:  body_twist [m,22,6]: angular velocity | velocity of the link frame's origin, per body of body_poses();
          summary: com [m,3], com_vel [m,3], ang_mom [m,3] (about the centre of mass), kinetic [m] (rigid bodies only, no rotor armature),
                   potential [m], mass [m];
          corners: corner_pos [m,8,3], corner_vel [m,8,3], corner_height [m,8] (signed height over the target stone's surface plane,
                   negative below it), corner_carrier [m,8] int32 (0 / 1 / 2: carried by stone n-1 / n / n+1, -1: by none); corner
                   4 * foot + k, foot 0 = right."""
        if not hasattr(self.backend, "kinematics"):
            raise NotImplementedError("this backend has no kinematic readout")
        if not (twists or summary or corners):
            raise ValueError("kinematics: ask for at least one of twists, summary, corners")
        if env_ids is None:
            ids, m = None, self.num_envs
        else:
            _, host_ids = self._env_ids(env_ids, allow_mask=False)
            m = int(host_ids.size)
            ids = torch.from_numpy(host_ids.astype(np.int32)).to(self.device)
        new = lambda *shape: torch.empty((m,) + shape, dtype=torch.float32, device=self.device)
        bt = new(_lib.NUM_BODIES, 6) if twists else None
        sm = new(_lib.KIN_SUMMARY) if summary else None
        co = new(_lib.KIN_CORNER, 8) if corners else None
        if m:
            self.backend.kinematics(ids, m, bt, sm, co)
        out = {}
        if twists:
            out["body_twist"] = bt
        if summary:
            out.update(com=sm[:, 0:3], com_vel=sm[:, 3:6], ang_mom=sm[:, 6:9], kinetic=sm[:, 9], potential=sm[:, 10], mass=sm[:, 11])
        if corners:
            out.update(corner_pos=co[:, :, 0:3], corner_vel=co[:, :, 3:6], corner_height=co[:, :, 6],
                       corner_carrier=co[:, :, 7].to(torch.int32))
        return {k: v.cpu().numpy() for k, v in out.items()} if self.return_numpy else out

    def step_forces(self, actions, env_ids=None, contacts=True, joints=True, next_state=True):
        """Dry run of one control step of the envs env_ids names (default: all; the forms of get_state()) under `actions` ([m,21], row k
        for env env_ids[k]; [N,21] without env_ids; policy coordinates, clipped as in step()): what the four substeps would do, read on
        the GPU from the current state, which stays as it is (docs/PHYSICS.md 10).  Returns a dict of tensors on the env's device
        (numpy arrays in numpy mode), m rows in env_ids order, holding the groups asked for:
          contacts:   contact_slot [m,4,8] int32 (per substep and sole corner 4 * foot + k, foot 0 = right: carried by stone n-1 / n / n+1 =
                      0 / 1 / 2 at the substep's start, -1: by none), contact_pen [m,4,8] (metres), contact_force [m,4,8,3] (newtons along
                      n, t1, t2), contact_force_world [m,4,8,3];
          joints:     joint_q, joint_qd [m,4,21] (start of each substep), joint_tau [m,4,21] (explicit torque), joint_torque [m,4,21] (the
                      torque applied over the substep under the linearly-implicit scheme);
          next_state: next_state [m,55] (words 0:55 of get_state() after the step), next_contact [m,2] bool (right / left foot),
                      next_on_target [m,2] bool."""
        if not hasattr(self.backend, "step_forces"):
            raise NotImplementedError("this backend has no force readout")
        if not (contacts or joints or next_state):
            raise ValueError("step_forces: ask for at least one of contacts, joints, next_state")
        if env_ids is None:
            ids, m = None, self.num_envs
        else:
            _, host_ids = self._env_ids(env_ids, allow_mask=False)
            m = int(host_ids.size)
            ids = torch.from_numpy(host_ids.astype(np.int32)).to(self.device)
        act = torch.as_tensor(actions, dtype=torch.float32).to(self.device).contiguous()
        if act.numel() != m * ACT_DIM:
            raise ValueError("step_forces: %d envs need actions of shape (%d, %d), got %s" % (m, m, ACT_DIM, tuple(act.shape)))
        act = act.reshape(m, ACT_DIM)
        new = lambda *shape: torch.empty((m,) + shape, dtype=torch.float32, device=self.device)
        co = new(_lib.FRC_SUBSTEPS, _lib.KIN_CORNER, _lib.FRC_CONTACT) if contacts else None
        jo = new(_lib.FRC_SUBSTEPS, _lib.FRC_JOINT, ACT_DIM) if joints else None
        ns = new(_lib.FRC_STATE) if next_state else None
        if m:
            self.backend.step_forces(ids, m, act, co, jo, ns)
        out = {}
        if contacts:
            out.update(contact_slot=co[..., 0].to(torch.int32), contact_pen=co[..., 1], contact_force=co[..., 2:5],
                       contact_force_world=co[..., 5:8])
        if joints:
            out.update(joint_q=jo[:, :, 0], joint_qd=jo[:, :, 1], joint_tau=jo[:, :, 2], joint_torque=jo[:, :, 3])
        if next_state:
            flags = ns[:, _lib.FRC_STATE - 1].to(torch.int32)
            out.update(next_state=ns[:, :_lib.FRC_STATE - 1], next_contact=torch.stack([flags & 1, (flags >> 1) & 1], 1).bool(),
                       next_on_target=torch.stack([(flags >> 2) & 1, (flags >> 3) & 1], 1).bool())
        return {k: v.cpu().numpy() for k, v in out.items()} if self.return_numpy else out

    def equation_of_motion(self, env_ids=None, mass=True, forces=True, jacobians=True):
        """The terms of the equation of motion of the envs env_ids names (default: all; the forms of get_state()), read on the GPU from
        the current state (docs/PHYSICS.md 11):  M nu-dot + c = g + [0; tau_m + passive] + sum_c J_c^T f_c  for the generalised velocity
        nu = [w_b (3); v_b (3); qd (21)] = state words 7:13 | 34:55 (base twist in body coordinates; joints in get_state()'s order, about
        the +axis).  Returns a dict of tensors on the env's device (numpy arrays in numpy mode), m rows in env_ids order, holding the
        groups asked for:
          mass:      mass [m,27,27]: joint-space inertia with the rotor armature on the joint diagonal, symmetric bit for bit;
          forces:    bias [m,27] (velocity-product force c), gravity [m,27] (generalised force of gravity g), passive [m,27] (joint
                     springs, dampers and limits in continuous time; 0 on the base);
          jacobians: corner_jac [m,8,3,27]: world velocity of sole corner 4 * foot + k (foot 0 = right) per unit nu."""
        if not hasattr(self.backend, "eom"):
            raise NotImplementedError("this backend has no equation-of-motion readout")
        if not (mass or forces or jacobians):
            raise ValueError("equation_of_motion: ask for at least one of mass, forces, jacobians")
        if env_ids is None:
            ids, m = None, self.num_envs
        else:
            _, host_ids = self._env_ids(env_ids, allow_mask=False)
            m = int(host_ids.size)
            ids = torch.from_numpy(host_ids.astype(np.int32)).to(self.device)
        new = lambda *shape: torch.empty((m,) + shape, dtype=torch.float32, device=self.device)
        ma = new(_lib.EOM_DOF, _lib.EOM_DOF) if mass else None
        fo = new(_lib.EOM_FORCES, _lib.EOM_DOF) if forces else None
        ja = new(_lib.KIN_CORNER, 3, _lib.EOM_DOF) if jacobians else None
        if m:
            self.backend.eom(ids, m, ma, fo, ja)
        out = {}
        if mass:
            out["mass"] = ma
        if forces:
            out.update(bias=fo[:, 0], gravity=fo[:, 1], passive=fo[:, 2])
        if jacobians:
            out["corner_jac"] = ja
        return {k: v.cpu().numpy() for k, v in out.items()} if self.return_numpy else out

    def push(self, impulse, env_ids=None, body=0, point=None, apply=True):
        """Push the envs env_ids names (default: all; the forms of get_state()): a wrench impulse on a body, on the GPU (docs/PHYSICS.md
        12).  impulse: [m,3], a linear impulse p in N s, or [m,6], p | a pure angular impulse L in N m s, world axes, row k for env
        env_ids[k]; body: an index in [0, 22), a name of model.BODY_NAMES, or m of either (default: the torso); point: [m,3] or [3], where p
        acts, in the body's link frame (default: the body's centre of mass).  Returns delta_nu [m,27] = M^-1 J^T w, the change of the
        generalised velocity nu = state words 7:13 | 34:55 (a tensor on the env's device, a numpy array in numpy mode).  apply=True adds
        it to the envs' velocities -- nothing else of the state changes, contacts and joint limits act from the next substep on;
        apply=False is a dry run.  The effect is linear: two pushes on one env are two dry runs added."""
        if not hasattr(self.backend, "push"):
            raise NotImplementedError("this backend has no push")
        if env_ids is None:
            ids, m = None, self.num_envs
        else:
            _, host_ids = self._env_ids(env_ids, allow_mask=False)
            m = int(host_ids.size)
            ids = torch.from_numpy(host_ids.astype(np.int32)).to(self.device)
        w = torch.as_tensor(impulse, dtype=torch.float32).to(self.device)
        if w.numel() not in (3 * m, _lib.PUSH_WRENCH * m) or (m == 0 and w.numel() != 0):
            raise ValueError("push: %d envs need an impulse of shape (%d, 3) or (%d, 6), got %s" % (m, m, m, tuple(w.shape)))
        w = w.reshape(m, -1) if m else w.reshape(0, _lib.PUSH_WRENCH)
        if w.shape[1] == 3:
            w = torch.cat([w, torch.zeros_like(w)], 1)
        w = w.contiguous()
        if isinstance(body, (str, int, np.integer)):
            names = [body] * m
        else:
            if not hasattr(body, "__len__"):
                raise ValueError("push: a body is an index in [0, %d) or a name, got %r" % (_lib.NUM_BODIES, body))
            names = body.tolist() if hasattr(body, "tolist") else list(body)
            if len(names) != m:
                raise ValueError("push: %d envs need one body or %d, got %d" % (m, m, len(names)))
        idx = []
        for b in names:
            if isinstance(b, str):
                if b not in BODY_NAMES:
                    raise ValueError("push: no body named %r (model.BODY_NAMES)" % (b,))
                b = BODY_NAMES.index(b)
            if not (isinstance(b, (int, np.integer)) and 0 <= b < _lib.NUM_BODIES):
                raise ValueError("push: a body is an index in [0, %d) or a name, got %r" % (_lib.NUM_BODIES, b))
            idx.append(int(b))
        bod = None if all(b == 0 for b in idx) else torch.tensor(idx, dtype=torch.int32).to(self.device)
        pt = None
        if point is not None:
            pt = torch.as_tensor(point, dtype=torch.float32).to(self.device)
            if pt.numel() == 3:
                pt = pt.reshape(1, 3).expand(m, 3)
            if pt.numel() != 3 * m:
                raise ValueError("push: point must have shape (3,) or (%d, 3), got %s" % (m, tuple(pt.shape)))
            pt = pt.reshape(m, 3).contiguous()
        out = torch.zeros((m, _lib.EOM_DOF), dtype=torch.float32, device=self.device)
        if m:
            self.backend.push(ids, m, bod, pt, w, out, bool(apply))
        return out.cpu().numpy() if self.return_numpy else out

    def _state_rows(self, states, what):
        """states as a contiguous float32 tensor on the env's device; anything that is no float32 tensor / array is refused"""
        if not (torch.is_tensor(states) or isinstance(states, np.ndarray)):
            raise ValueError("%s: states must be a float32 tensor or array, got %s" % (what, type(states).__name__))
        if states.dtype not in (torch.float32, np.float32):
            raise ValueError("%s: states must be float32, got %s" % (what, states.dtype))
        if states.ndim < 1 or states.shape[-1] != STATE_DIM:
            raise ValueError("%s: a state row has %d words (get_state()), got shape %s" % (what, STATE_DIM, tuple(states.shape)))
        return torch.as_tensor(states).to(self.device).contiguous()

    def observe(self, states):
        """The observation of each packed state row, on the GPU (docs/PHYSICS.md 13): states [m,186] (get_state()'s layout, float32
        tensor or array) -> [m,60], row k what get_obs() gives after set_state(states[k]).  No env is read or written: this is the
        observation at the root of a lookahead(states=...) branch, or of a logged state."""
        if not hasattr(self.backend, "get_obs_states"):
            raise NotImplementedError("this backend has no observation of state rows")
        st = self._state_rows(states, "observe")
        if st.dim() != 2:
            raise ValueError("observe: states must have shape (m, %d), got %s" % (STATE_DIM, tuple(st.shape)))
        m = int(st.shape[0])
        out = torch.zeros((m, OBS_DIM), dtype=torch.float32, device=self.device)
        if m:
            self.backend.get_obs_states(m, st, out)
        return out.cpu().numpy() if self.return_numpy else out

    def lookahead(self, actions, env_ids=None, obs=True, final_state=False, states=None):
        """Dry run of H control steps per action sequence, on the GPU, from the envs' current state, which stays as it is: no state
        word, no terrain row, no RNG counter changes (docs/PHYSICS.md 13).  actions: [m,H,21], row k a BRANCH of env env_ids[k] (ids in
        [0, N), repeats welcome: B branches of an env are B rows with its id; [N,H,21] without env_ids), or [N,B,H,21] without env_ids:
        B branches of every env, and every result below comes back as [N,B,...].  Policy coordinates, clipped as in step().  A branch
        sees the stones, target advances and time limit the env would see under those actions and never resets: after its first done
        step its rewards are 0, its done flags True and its observation repeats.  Returns a dict of tensors on the env's device (numpy
        arrays in numpy mode): rew [m,H], done [m,H] bool, ret [m] (the sum of the branch's rewards), obs [m,H,60] if asked for,
        final_state [m,186] if asked for (the get_state() row the branch ends in: set_state_envs commits it).
        states: [m,186] float32 (get_state()'s layout; [N,B,186] with [N,B,H,21] actions): branch k starts from states[k] instead of
        env env_ids[k]'s current state -- the final_state of an earlier call (a deeper level of a tree search), get_state() with a
        push(apply=False) added, a perturbed or a logged state.  The env still gives its id (the stream its stones are drawn from), its
        probability grid and the curriculum; observe(states) is the observation such a branch starts from."""
        if states is not None and not hasattr(self.backend, "lookahead_states"):
            raise NotImplementedError("this backend has no look-ahead from caller-supplied states")
        if not hasattr(self.backend, "lookahead"):
            raise NotImplementedError("this backend has no look-ahead")
        st = None if states is None else self._state_rows(states, "lookahead")
        act = torch.as_tensor(actions, dtype=torch.float32).to(self.device).contiguous()
        lead = None
        if act.dim() == 4:
            if env_ids is not None or act.shape[0] != self.num_envs or act.shape[3] != ACT_DIM:
                raise ValueError("lookahead: four-dimensional actions are (%d, B, H, %d) without env_ids, got %s"
                                 % (self.num_envs, ACT_DIM, tuple(act.shape)))
            lead = (self.num_envs, int(act.shape[1]))
            host_ids = np.repeat(np.arange(self.num_envs, dtype=np.int64), lead[1])
            act = act.reshape(lead[0] * lead[1], act.shape[2], ACT_DIM)
        elif env_ids is None:
            host_ids = None
        else:
            ids = env_ids.detach().cpu().numpy() if torch.is_tensor(env_ids) else np.asarray(env_ids)
            if ids.size and (ids.ndim > 1 or not np.issubdtype(ids.dtype, np.integer)):
                raise ValueError("env ids must be a one-dimensional sequence of integers, got dtype %s shape %s" % (ids.dtype, ids.shape))
            host_ids = ids.reshape(-1).astype(np.int64)
            if host_ids.size and (host_ids.min() < 0 or host_ids.max() >= self.num_envs):
                raise ValueError("env ids must lie in [0, %d), got %d..%d" % (self.num_envs, host_ids.min(), host_ids.max()))
        m = self.num_envs if host_ids is None else int(host_ids.size)
        if act.dim() != 3 or act.shape[0] != m or act.shape[2] != ACT_DIM:
            raise ValueError("lookahead: %d branches need actions of shape (%d, H, %d), got %s" % (m, m, ACT_DIM, tuple(act.shape)))
        horizon = int(act.shape[1])
        if not 1 <= horizon <= _lib.LOOK_MAX_STEPS:
            raise ValueError("lookahead: the horizon must lie in [1, %d], got %d" % (_lib.LOOK_MAX_STEPS, horizon))
        if st is not None:
            want = lead + (STATE_DIM,) if lead is not None else (m, STATE_DIM)
            if tuple(st.shape) != want:
                raise ValueError("lookahead: these actions need states of shape %s, got %s" % (want, tuple(st.shape)))
            st = st.reshape(m, STATE_DIM)
        ids = None if host_ids is None else torch.from_numpy(host_ids.astype(np.int32)).to(self.device)
        new = lambda *shape: torch.zeros((m,) + shape, dtype=torch.float32, device=self.device)
        rew = new(horizon)
        done = torch.ones((m, horizon), dtype=torch.uint8, device=self.device)
        ob = new(horizon, OBS_DIM) if obs else None
        fs = new(STATE_DIM) if final_state else None
        if m:
            work = torch.empty((m, _lib.LOOK_WORK), dtype=torch.float32, device=self.device)
            if st is None:
                self.backend.lookahead(ids, m, horizon, act, ob, rew, done, fs, work)
            else:
                self.backend.lookahead_states(ids, m, st, horizon, act, ob, rew, done, fs, work)
        out = {"rew": rew, "done": done.bool(), "ret": rew.sum(1)}
        if obs:
            out["obs"] = ob
        if final_state:
            out["final_state"] = fs
        if lead is not None:
            out = {k: v.reshape(lead + tuple(v.shape[1:])) for k, v in out.items()}
        return {k: v.cpu().numpy() for k, v in out.items()} if self.return_numpy else out

    def lookahead_policy(self, policy, horizon, env_ids=None, states=None, offsets=None, obs=True, actions=True, final_state=False):
        """lookahead() with the policy in the loop, in one launch (docs/PHYSICS.md 14): the action of step s of branch k is
        policy(observation after step s - 1) + offsets[k,s], the observation before step 0 being get_obs() of the env (observe(states[k])
        with states).  policy: a PackedPolicy (pack_policy), or anything pack_policy takes (packed on every call then).  Branches: [m] ids
        in env_ids (all N envs in order without), or B per env through offsets [N,B,H,21] / states [N,B,186], every result then [N,B,...].
        offsets: [m,H,21] float32 or None (zeros) -- exploration noise, a planner's perturbations.  Returns lookahead()'s dict plus "act"
        [m,H,21] if actions: the actions applied, unclipped; zeros behind a branch's first done.  Given those actions everything else is
        bit for bit lookahead(act, ...)'s."""
        if not hasattr(self.backend, "lookahead_policy"):
            raise NotImplementedError("this backend has no closed-loop look-ahead")
        horizon = int(horizon)
        if not 1 <= horizon <= _lib.LOOK_MAX_STEPS:
            raise ValueError("lookahead_policy: the horizon must lie in [1, %d], got %d" % (_lib.LOOK_MAX_STEPS, horizon))
        if not isinstance(policy, PackedPolicy):
            policy = PackedPolicy(policy, self.device)
        if policy.device != self.device:
            raise ValueError("lookahead_policy: the policy is packed on %s, the env lives on %s" % (policy.device, self.device))
        st = None if states is None else self._state_rows(states, "lookahead_policy")
        off = None
        if offsets is not None:
            if not (torch.is_tensor(offsets) or isinstance(offsets, np.ndarray)) or offsets.dtype not in (torch.float32, np.float32):
                raise ValueError("lookahead_policy: offsets must be a float32 tensor or array")
            off = torch.as_tensor(offsets).to(self.device).contiguous()
            if off.dim() not in (3, 4) or tuple(off.shape[-2:]) != (horizon, ACT_DIM):
                raise ValueError("lookahead_policy: offsets must have shape (m, %d, %d) or (N, B, %d, %d), got %s"
                                 % (horizon, ACT_DIM, horizon, ACT_DIM, tuple(off.shape)))
        lead = None
        if (off is not None and off.dim() == 4) or (st is not None and st.dim() == 3):
            shape = tuple(off.shape[:2]) if off is not None and off.dim() == 4 else tuple(st.shape[:2])
            if env_ids is not None or shape[0] != self.num_envs:
                raise ValueError("lookahead_policy: B branches per env are (%d, B, ...) without env_ids, got %s" % (self.num_envs, shape))
            if (off is not None and tuple(off.shape[:2]) != shape) or (st is not None and tuple(st.shape[:-1]) != shape):
                raise ValueError("lookahead_policy: offsets and states must both be (%d, %d, ...)" % shape)
            lead = (self.num_envs, int(shape[1]))
            host_ids = np.repeat(np.arange(self.num_envs, dtype=np.int64), lead[1])
        elif env_ids is None:
            host_ids = None
        else:
            ids = env_ids.detach().cpu().numpy() if torch.is_tensor(env_ids) else np.asarray(env_ids)
            if ids.size and (ids.ndim > 1 or not np.issubdtype(ids.dtype, np.integer)):
                raise ValueError("env ids must be a one-dimensional sequence of integers, got dtype %s shape %s" % (ids.dtype, ids.shape))
            host_ids = ids.reshape(-1).astype(np.int64)
            if host_ids.size and (host_ids.min() < 0 or host_ids.max() >= self.num_envs):
                raise ValueError("env ids must lie in [0, %d), got %d..%d" % (self.num_envs, host_ids.min(), host_ids.max()))
        m = self.num_envs if host_ids is None else int(host_ids.size)
        if st is not None:
            if st.numel() != m * STATE_DIM or (lead is None and st.dim() != 2):
                raise ValueError("lookahead_policy: %d branches need states of shape (%d, %d), got %s" % (m, m, STATE_DIM, tuple(st.shape)))
            st = st.reshape(m, STATE_DIM)
        if off is not None:
            if off.numel() != m * horizon * ACT_DIM or (lead is None and off.dim() != 3):
                raise ValueError("lookahead_policy: %d branches need offsets of shape (%d, %d, %d), got %s"
                                 % (m, m, horizon, ACT_DIM, tuple(off.shape)))
            off = off.reshape(m, horizon, ACT_DIM)
        ids = None if host_ids is None else torch.from_numpy(host_ids.astype(np.int32)).to(self.device)
        new = lambda *shape: torch.zeros((m,) + shape, dtype=torch.float32, device=self.device)
        rew = new(horizon)
        done = torch.ones((m, horizon), dtype=torch.uint8, device=self.device)
        ob = new(horizon, OBS_DIM) if obs else None
        ac = new(horizon, ACT_DIM) if actions else None
        fs = new(STATE_DIM) if final_state else None
        if m:
            policy.bind(self.backend)
            work = torch.empty((m, _lib.LOOK_WORK), dtype=torch.float32, device=self.device)
            self.backend.lookahead_policy(ids, m, st, horizon, policy.desc, policy.blob, off, ac, ob, rew, done, fs, work)
        out = {"rew": rew, "done": done.bool(), "ret": rew.sum(1)}
        if obs:
            out["obs"] = ob
        if actions:
            out["act"] = ac
        if final_state:
            out["final_state"] = fs
        if lead is not None:
            out = {k: v.reshape(lead + tuple(v.shape[1:])) for k, v in out.items()}
        return {k: v.cpu().numpy() for k, v in out.items()} if self.return_numpy else out

    @property
    def unwrapped(self):
        return self

    # ------------------------------------------------------------------ curriculum hooks
    def update_curriculum(self, curriculum):
        self.curriculum = int(curriculum)
        self.backend.set_curriculum(min(max(self.curriculum, 0), 5))

    def update_specialist(self, specialist):
        self.curriculum = int(specialist)
        self.backend.set_specialist(min(max(int(specialist), 0), 5))

    def update_sample_prob(self, probs):
        """probs: (N,11,11) one grid per env (playground/train.py:267-271) or a single (11,11) grid.  A torch tensor on
        the env's device takes the stream-ordered path (no host copy, no synchronisation)."""
        if torch.is_tensor(probs) and probs.device.type == "cuda":
            if tuple(probs.shape) not in ((GRID, GRID), (self.num_envs, GRID, GRID)):
                raise ValueError("sample_prob must have shape (%d,%d,%d) or (%d,%d), got %s"
                                 % (self.num_envs, GRID, GRID, GRID, GRID, tuple(probs.shape)))
            p = probs.to(device=self.device, dtype=torch.float32).contiguous()
            self._prob_keepalive = p           # the kernel reads it asynchronously
            self.backend.set_sample_prob_device(p, p.dim() == 3)
            return
        probs = np.asarray(probs.cpu() if torch.is_tensor(probs) else probs, np.float64)
        if probs.shape == (GRID, GRID):
            self.backend.set_sample_prob(probs, False)
        elif probs.shape == (self.num_envs, GRID, GRID):
            same = self.num_envs == 1 or bool(np.all(probs == probs[0]))
            self.backend.set_sample_prob(probs[0] if same else probs, not same)
        else:
            raise ValueError("sample_prob must have shape (%d,%d,%d) or (%d,%d), got %s"
                             % (self.num_envs, GRID, GRID, GRID, GRID, probs.shape))

    _warned_set_mirror = False

    def create_temp_states(self):
        out = torch.empty((self.num_envs, NCELL, OBS_DIM), dtype=torch.float32, device=self.device)
        self.backend.create_temp_states(out)
        return out.cpu().numpy() if self.return_numpy else out

    def set_mirror(self, mirror):
        """common/envs_utils.py:588-590.  Accepted for protocol compatibility only: no effect on Walker3D / Mike (their observation has
        no gait-phase term; include/steppingstone.h ss_set_mirror).  The symmetry itself is get_mirror_indices().
        `use_phase_mirror=True` (playground/train.py:48,109-111) is therefore UNSUPPORTED: set_mirror(True) warns once per process
        instead of silently accepting; the reference's default is False."""
        if mirror and not SteppingStoneVecEnv._warned_set_mirror:
            import warnings
            SteppingStoneVecEnv._warned_set_mirror = True
            warnings.warn("set_mirror(True): phase mirroring (use_phase_mirror, playground/train.py:48,109) is not supported by this env -- the "
                          "call is accepted for protocol compatibility and has no effect; use get_mirror_indices() with mirror "
                          "augmentation (common/envs_utils.py:687-740) instead", RuntimeWarning, stacklevel=2)
        self.backend.set_mirror(bool(mirror))

    def set_env_params(self, params_dict):
        for k, v in dict(params_dict).items():
            if k == "curriculum":
                self.update_curriculum(v)
            else:
                raise KeyError("unsupported env param %r" % (k,))

    def set_robot_params(self, params_dict):
        for k, v in dict(params_dict).items():
            if k == "power":
                self.backend.set_power(float(v))
            else:
                raise KeyError("unsupported robot param %r" % (k,))

    def get_mirror_indices(self):
        return _lib.mirror_indices(self.kind)

    # ------------------------------------------------------------------ state access
    def get_state(self, env_ids=None):
        """Packed state [N,186] (include/steppingstone.h), or [m,186] of the envs env_ids names (the forms of reset(); a mask here
        selects its envs in ascending order), rows in env_ids order."""
        if env_ids is None:
            st = torch.empty((self.num_envs, STATE_DIM), dtype=torch.float32, device=self.device)
            self.backend.get_state(st)
            return st
        _, ids = self._env_ids(env_ids, allow_mask=False)
        st = torch.empty((ids.size, STATE_DIM), dtype=torch.float32, device=self.device)
        if ids.size:
            self.backend.get_state_envs(torch.from_numpy(ids.astype(np.int32)).to(self.device), st)
        return st

    def set_state(self, packed, env_ids=None):
        """Inject the packed state of all envs ([N,186]), or of the envs env_ids names ([m,186], row k -> env env_ids[k]; ids checked
        as in reset(), duplicates rejected)."""
        if env_ids is None:
            st = torch.as_tensor(packed, dtype=torch.float32).to(self.device).contiguous().reshape(self.num_envs, STATE_DIM)
            self.backend.set_state(st)
            return
        _, ids = self._env_ids(env_ids, allow_mask=False)
        st = torch.as_tensor(packed, dtype=torch.float32).to(self.device).contiguous()
        if st.numel() != ids.size * STATE_DIM:
            raise ValueError("set_state: %d env ids need packed of shape (%d, %d), got %s" % (ids.size, ids.size, STATE_DIM, tuple(st.shape)))
        if ids.size:
            self.backend.set_state_envs(torch.from_numpy(ids.astype(np.int32)).to(self.device), st.reshape(ids.size, STATE_DIM))

    def get_obs(self):
        self.backend.get_obs(self._obs)
        return self._out_obs()

    @property
    def terrain_info(self):
        """(N,20,6) x,y,z,phi,x_tilt,y_tilt (playground/enjoy.py:60-64)."""
        return self.get_state()[:, 65:185].reshape(self.num_envs, NUM_STONES, 6).cpu().numpy()

    @property
    def next_step_index(self):
        return self.get_state()[:, 59].cpu().numpy().astype(np.int64)

    # ------------------------------------------------------------------ helpers
    def _env_ids(self, env_ids, allow_mask):
        """Check env_ids on the host before anything indexes with them on the GPU (a device-side index assert is a GPU fault).
        Returns (mask, None) for a bool / uint8 TENSOR of shape [N] when allow_mask (uint8 on the env's device, never read here), else
        (None, ids): a host int64 array of distinct ids in [0, N) (a mask, a numpy bool array included, gives its set envs in order)."""
        n = self.num_envs
        if torch.is_tensor(env_ids) and env_ids.dtype in (torch.bool, torch.uint8) or isinstance(env_ids, np.ndarray) and env_ids.dtype == bool:
            if tuple(env_ids.shape) != (n,):
                raise ValueError("an env mask must have shape (%d,), got %s" % (n, tuple(env_ids.shape)))
            if allow_mask and torch.is_tensor(env_ids):
                mask = env_ids.to(self.device).contiguous()
                return (mask.view(torch.uint8) if mask.dtype == torch.bool else mask), None
            mask = env_ids.cpu().numpy() if torch.is_tensor(env_ids) else env_ids
            return None, np.nonzero(mask)[0].astype(np.int64)
        ids = env_ids.detach().cpu().numpy() if torch.is_tensor(env_ids) else np.asarray(env_ids)    # (a device tensor: one sync)
        if ids.size == 0:
            return None, np.zeros(0, np.int64)
        if ids.ndim > 1 or not np.issubdtype(ids.dtype, np.integer):
            raise ValueError("env ids must be a one-dimensional sequence of integers, got dtype %s shape %s" % (ids.dtype, ids.shape))
        ids = ids.reshape(-1).astype(np.int64)
        if ids.min() < 0 or ids.max() >= n:
            raise ValueError("env ids must lie in [0, %d), got %d..%d" % (n, ids.min(), ids.max()))
        if np.unique(ids).size != ids.size:
            raise ValueError("env ids must be distinct")
        return None, ids

    def _out_obs(self):
        return self._obs.cpu().numpy() if self.return_numpy else self._obs

    def _info_tensors(self):
        fl = self._info.view(torch.float32)
        return {"ep_ret": fl[:, 0], "ep_len": fl[:, 1], "bad_transition": self._info[:, 2],
                "steps_reached": self._info[:, 3], "update_terrain": self._info[:, 4], "ep_ret_lo": fl[:, 5]}

    def _info_dicts(self, done, raw=None):
        """Sequence of N info dicts with the reference's keys (common/envs_utils.py:59-65,131-153).  raw: the [N,6] info words
        on the host already (numpy drop-in mode); else they are fetched when any env finished."""
        infos = [_EMPTY_INFO] * self.num_envs
        idx = np.nonzero(done)[0]
        if idx.size:
            if raw is None:
                raw = self._info.cpu().numpy()
            fl = raw.view(np.float32)
            now = round(time.time() - self._tstart, 6)
            # Monitor.update: eprew = sum(self.rewards) in Python floats, "r": round(eprew, 6) (common/envs_utils.py:134-138); the
            # kernel's (ep_ret, ep_ret_lo) pair is that fp64 sum of the fp32 step rewards.  Columns are pulled out as Python lists
            # once (per-element numpy indexing made this loop 200 us per step at 4096 envs, two thirds of the drop-in mode's step).
            rets = (fl[idx, 0].astype(np.float64) + fl[idx, 5].astype(np.float64)).tolist()
            lens = fl[idx, 1].astype(np.int64).tolist()
            bad, reached = raw[idx, 2].tolist(), raw[idx, 3].tolist()
            for k, i in enumerate(idx.tolist()):
                d = {"episode": {"r": round(rets[k], 6), "l": lens[k], "t": now}, "steps_reached": reached[k]}
                if self._monitor is not None:
                    self._monitor.write_row(i, d["episode"])
                if bad[k]:
                    d["bad_transition"] = True
                infos[i] = d
        return tuple(infos)


class _Robot:
    def __init__(self):
        self.feet_contact = np.zeros(2, np.float32)


class SteppingStoneEnv:
    """Single-env gym-style facade over a 1-env SteppingStoneVecEnv (what `make_env` returns in the reference;
    playground/train.py:96,129-131,231-247 and playground/enjoy.py:101-102,231-235 use these members)."""

    def __init__(self, env_id, seed=0, device=None, render=False, backend_factory=None):
        self._env_id = env_id
        self.render_mode = "rgb_array" if render else None     # there is no window: render=True means frames on request
        self._device = device
        self._backend_factory = backend_factory
        self._make(seed)
        self.robot = _Robot()
        self.update_terrain = False
        self.camera = None

    def _make(self, seed):
        backend = self._backend_factory(kind_of(self._env_id), 1, seed) if self._backend_factory else None
        self.vec = SteppingStoneVecEnv(self._env_id, 1, seed=seed, device=self._device, return_numpy=True, backend=backend)
        self.vec.backend.set_auto_reset(False)
        self.observation_space = self.vec.observation_space
        self.action_space = self.vec.action_space
        self.spec = self.vec.spec
        self.yaw_samples, self.pitch_samples = self.vec.yaw_samples, self.vec.pitch_samples
        self.yaw_sample_size, self.pitch_sample_size = GRID, GRID
        self._max_episode_steps = MAX_EPISODE_STEPS

    @property
    def unwrapped(self):
        return self

    def seed(self, seed=None):
        curriculum = self.vec.curriculum
        self.vec.close()
        self._make(0 if seed is None else int(seed))
        self.vec.update_curriculum(curriculum)
        return [seed]

    def reset(self):
        self.update_terrain = False
        return self.vec.reset()[0]

    def step(self, action):
        obs, rew, done, infos = self.vec.step(np.asarray(action, np.float32).reshape(1, ACT_DIM))
        raw = self.vec._info_host[0]          # the step's info words, already on the host (no second copy)
        self.update_terrain = bool(raw[4])
        self.robot.feet_contact[:] = obs[0, 48:50]
        info = dict(infos[0])
        return obs[0], float(rew[0]), bool(done[0]), info

    def step_forces(self, action):
        """Dry run of step(action) from the current state (SteppingStoneVecEnv.step_forces): the dict without the env axis."""
        out = self.vec.step_forces(np.asarray(action, np.float32).reshape(1, ACT_DIM))
        return {k: v[0] for k, v in out.items()}

    def lookahead(self, actions, obs=True, final_state=False, states=None):
        """Dry run of B action sequences from the current state (SteppingStoneVecEnv.lookahead): actions [B,H,21] (or [H,21]: one
        branch) -> the dict with B rows.  states: [B,186] (or [186] with one branch): branch b starts from states[b] instead."""
        a = np.asarray(actions, np.float32)
        a = a.reshape((-1,) + a.shape[-2:])
        if states is not None:
            states = self.vec._state_rows(states, "lookahead")
            states = states.reshape(1, STATE_DIM) if states.dim() == 1 else states
        return self.vec.lookahead(a, env_ids=np.zeros(a.shape[0], np.int64), obs=obs, final_state=final_state, states=states)

    def lookahead_policy(self, policy, horizon, states=None, offsets=None, obs=True, actions=True, final_state=False, branches=None):
        """Closed-loop dry run from the current state (SteppingStoneVecEnv.lookahead_policy): B branches, B the rows of offsets [B,H,21]
        or of states [B,186] (`branches` without both; default 1) -> the dict with B rows."""
        if states is not None:
            states = self.vec._state_rows(states, "lookahead_policy")
            states = states.reshape(1, STATE_DIM) if states.dim() == 1 else states
        if offsets is not None:
            offsets = np.asarray(offsets.cpu() if torch.is_tensor(offsets) else offsets, np.float32)
            offsets = offsets.reshape((-1,) + offsets.shape[-2:])
        b = offsets.shape[0] if offsets is not None else (int(states.shape[0]) if states is not None else int(branches or 1))
        return self.vec.lookahead_policy(policy, horizon, env_ids=np.zeros(b, np.int64), states=states, offsets=offsets, obs=obs,
                                         actions=actions, final_state=final_state)

    def observe(self, states):
        """The observation of packed state rows (SteppingStoneVecEnv.observe): states [m,186] -> [m,60]; one row [186] -> [60]."""
        st = self.vec._state_rows(states, "observe")
        return self.vec.observe(st.reshape(1, STATE_DIM))[0] if st.dim() == 1 else self.vec.observe(st)

    def equation_of_motion(self, mass=True, forces=True, jacobians=True):
        """The terms of the equation of motion at the current state (SteppingStoneVecEnv.equation_of_motion): the dict without the env axis."""
        out = self.vec.equation_of_motion(mass=mass, forces=forces, jacobians=jacobians)
        return {k: v[0] for k, v in out.items()}

    def push(self, impulse, body=0, point=None, apply=True):
        """Push the robot (SteppingStoneVecEnv.push): impulse [3] or [6]; returns delta_nu [27]."""
        w = np.asarray(impulse, np.float32).reshape(1, -1)
        return self.vec.push(w, body=body, point=None if point is None else np.asarray(point, np.float32).reshape(1, 3), apply=apply)[0]

    def render(self, mode="rgb_array", width=256, height=192, camera=None):
        """One (H, W, 3) uint8 frame of the env (SteppingStoneVecEnv.render); mode="human" raises NotImplementedError."""
        return self.vec.render(mode, width=width, height=height, camera=camera)[0]

    def close(self):
        self.vec.close()

    def update_curriculum(self, curriculum):
        self.vec.update_curriculum(curriculum)

    def update_specialist(self, specialist):
        self.vec.update_specialist(specialist)

    def update_sample_prob(self, prob):
        self.vec.update_sample_prob(np.asarray(prob, np.float64).reshape(GRID, GRID))

    def set_mirror(self, mirror):
        self.vec.set_mirror(mirror)

    def create_temp_states(self):
        return self.vec.create_temp_states()[0]

    def get_mirror_indices(self):
        return self.vec.get_mirror_indices()

    @property
    def terrain_info(self):
        return self.vec.terrain_info[0]

    @property
    def next_step_index(self):
        return int(self.vec.next_step_index[0])


def make_env(env_id, render=False, seed=0, device=None):
    """Counterpart of common/envs_utils.py:43-45."""
    return SteppingStoneEnv(env_id, seed=seed, device=device, render=render)


def make_vec_envs(env_id, seed, num_processes, log_dir=None, device=None, return_numpy=True, env_id_offset=0):
    """Counterpart of common/envs_utils.py:48-56: `num_processes` environments with seeds seed+rank.  The reference
    forks one process per env; here they are lanes of one kernel on `device`.  log_dir: as in make_env_fns (:36-38), env `rank`
    logs its episodes to <log_dir>/<rank>.monitor.csv (steppingstone_amd/monitor_csv.py); None: no files, as in the reference."""
    assert num_processes > 1
    return SteppingStoneVecEnv(env_id, num_processes, seed=seed, device=device, env_id_offset=env_id_offset,
                               return_numpy=return_numpy, log_dir=log_dir)
