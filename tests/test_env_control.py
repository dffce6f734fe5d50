"""Per-env episode control of SteppingStoneVecEnv on the host side: reset(env_ids), set_auto_reset, keep_terminal_obs and the subset
forms of get_state / set_state, driven by a stub backend.  Ids are checked before the backend is called, and rows travel to and from
the right envs.  CPU only (the kernels behind them: tests/test_gpu_env_control.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from steppingstone_amd import _lib
from steppingstone_amd.envs import SteppingStoneVecEnv

N = 6


class StubBackend:
    """HipBackend's call surface on the CPU.  Env e's state is row e of [N,186]: word 0 counts the steps of its episode, word 1 is e,
    word 2 counts its resets; its observation is words 0..59.  A step ends the episodes of the envs in `finish`."""

    def __init__(self, n=N):
        self.device = torch.device("cpu")
        self.n = n
        self.state = torch.zeros((n, 186))
        self.state[:, 1] = torch.arange(n, dtype=torch.float32)
        self.auto_reset = True
        self.finish = set()
        self.calls = []

    def _reset_env(self, e):
        self.state[e, 0] = 0.0
        self.state[e, 2] += 1.0

    def close(self):
        pass

    def set_auto_reset(self, on):
        self.auto_reset = bool(on)

    def set_curriculum(self, level):
        pass

    def reset(self, obs):
        self.calls.append("reset")
        for e in range(self.n):
            self._reset_env(e)
        obs.copy_(self.state[:, :60])

    def _step(self):
        self.state[:, 0] += 1.0
        done = torch.zeros(self.n, dtype=torch.uint8)
        for e in self.finish:
            done[e] = 1
            if self.auto_reset:
                self._reset_env(e)
        return done

    def step(self, act, obs, rew, done, info):
        self.calls.append("step")
        done.copy_(self._step())
        obs.copy_(self.state[:, :60])
        rew.copy_(torch.arange(self.n, dtype=torch.float32))
        info.zero_()

    def step_packed(self, act, use_random, t, packed, info):
        self.calls.append("step_packed")
        d = self._step()
        packed[:, :60] = self.state[:, :60]
        packed[:, 60] = torch.arange(self.n, dtype=torch.float32)
        packed[:, 61] = d.float()
        info.zero_()

    def reset_masked(self, mask, obs, terminal=None):
        self.calls.append(("reset_masked", mask.clone(), terminal is not None))
        assert mask.dtype == torch.uint8 and mask.shape == (self.n,)
        for e in torch.nonzero(mask).flatten().tolist():
            if terminal is not None:
                terminal[e] = obs[e, :60]
            self._reset_env(e)
            if obs is not None:
                obs[e, :60] = self.state[e, :60]

    def get_state(self, packed):
        packed.copy_(self.state)

    def set_state(self, packed):
        self.state.copy_(packed)

    def get_state_envs(self, env_ids, packed):
        self.calls.append("get_state_envs")
        assert env_ids.dtype == torch.int32
        packed.copy_(self.state[env_ids.long()])

    def set_state_envs(self, env_ids, packed):
        self.calls.append("set_state_envs")
        self.state[env_ids.long()] = packed

    def get_obs(self, obs):
        obs.copy_(self.state[:, :60])

    def random_actions(self, t, act):
        act.zero_()


def make(numpy_mode=False, **kw):
    env = SteppingStoneVecEnv("Walker3DStepperEnv-v0", N, return_numpy=numpy_mode, backend=StubBackend(), **kw)
    env.reset()
    return env


@pytest.mark.parametrize("bad", [[0, N], [-1], [2, 2], [[0, 1]], [0.0, 1.0], torch.tensor([1, N]), torch.tensor([3, 3]),
                                 torch.zeros(N + 1, dtype=torch.bool), torch.zeros((N, 1), dtype=torch.uint8),
                                 np.zeros(N - 1, bool)])
def test_invalid_env_ids_raise_before_the_backend_runs(bad):
    env = make()
    before = list(env.backend.calls)
    state = env.backend.state.clone()
    with pytest.raises(ValueError):
        env.reset(bad)
    with pytest.raises(ValueError):
        env.get_state(bad)
    with pytest.raises(ValueError):
        env.set_state(torch.zeros((2, 186)), bad)
    assert env.backend.calls == before and torch.equal(env.backend.state, state)


def test_set_state_subset_checks_the_row_count():
    env = make()
    with pytest.raises(ValueError):
        env.set_state(torch.zeros((3, 186)), [0, 1])
    assert "set_state_envs" not in env.backend.calls


def test_reset_rows_follow_env_ids_order_and_touch_only_those_envs():
    env = make()
    resets = env.backend.state[:, 2].clone()
    for ids in ([4, 0, 2], np.array([4, 0, 2]), torch.tensor([4, 0, 2])):
        rows = env.reset(ids)
        assert rows.shape == (3, 60) and rows[:, 1].tolist() == [4.0, 0.0, 2.0]
    assert (env.backend.state[:, 2] - resets).tolist() == [3, 0, 3, 0, 3, 0]
    mask = env.backend.calls[-1][1]
    assert mask.tolist() == [1, 0, 1, 0, 1, 0]
    # the mask form keeps the batch shape and is handed to the backend as it is (uint8 view of a bool mask)
    m = torch.tensor([0, 1, 0, 0, 0, 1], dtype=torch.bool)
    out = env.reset(m)
    assert out.shape == (N, 60) and out is env._obs
    assert env.backend.calls[-1][1].tolist() == [0, 1, 0, 0, 0, 1]
    ncalls = len(env.backend.calls)
    assert env.reset([]).shape == (0, 60) and len(env.backend.calls) == ncalls
    assert env.reset(np.array([3])).shape == (1, 60)
    np_env = make(numpy_mode=True)
    rows = np_env.reset([5, 1])
    assert isinstance(rows, np.ndarray) and rows[:, 1].tolist() == [5.0, 1.0]


def test_subset_state_rows_follow_env_ids():
    env = make()
    full = env.get_state()
    assert torch.equal(env.get_state([3, 1]), full[[3, 1]])
    assert torch.equal(env.get_state(torch.tensor([False, True, False, True, False, False])), full[[1, 3]])
    rows = torch.full((2, 186), 7.0)
    rows[1] = 9.0
    env.set_state(rows, [5, 0])
    want = full.clone()
    want[5], want[0] = 7.0, 9.0
    assert torch.equal(env.get_state(), want)
    assert env.get_state([]).shape == (0, 186)


def test_set_auto_reset_is_public_and_keep_terminal_obs_refuses_it_off():
    env = make()
    env.set_auto_reset(False)
    assert env.backend.auto_reset is False
    env.set_auto_reset(True)
    assert env.backend.auto_reset is True
    k = make(keep_terminal_obs=True)
    assert k.backend.auto_reset is False            # the kernel steps without its auto-reset; the env resets behind it
    with pytest.raises(ValueError):
        k.set_auto_reset(False)
    k.set_auto_reset(True)
    assert k.backend.auto_reset is False
    with pytest.raises(ValueError):
        k.rollout_random(4)
    with pytest.raises(ValueError):
        k.rollout_random_packed(torch.zeros((2, N, 62)))


def test_terminal_observation_only_in_finished_infos():
    env = make(numpy_mode=True, keep_terminal_obs=True)
    env.backend.finish = {1, 4}
    for _ in range(3):
        obs, rew, done, infos = env.step(np.zeros((N, 21), np.float32))
    assert done.tolist() == [False, True, False, False, True, False]
    for i, info in enumerate(infos):
        if done[i]:
            t = info["terminal_observation"]
            assert t.dtype == np.float32 and t.shape == (60,)
            assert t[0] == 1.0 and t[1] == i         # the row the finished step left: one step into its episode
            assert obs[i, 0] == 0.0                  # ... and the env starts afresh
        else:
            assert "terminal_observation" not in info and obs[i, 0] == 3.0
    steps = [c for c in env.backend.calls if c == "step" or isinstance(c, tuple)]
    assert all(c[0] == "reset_masked" and c[2] for c in steps[1::2])        # every step is followed by the masked reset
    env.backend.finish = set()
    _, _, done, infos = env.step(np.zeros((N, 21), np.float32))
    assert not done.any() and not any("terminal_observation" in i for i in infos)


def test_terminal_obs_in_tensor_mode_and_through_step_packed():
    env = make(keep_terminal_obs=True)
    env.backend.finish = {2}
    env.step(torch.zeros(N, 21))
    obs, rew, done, info = env.step(torch.zeros(N, 21))
    assert done.tolist() == [False, False, True, False, False, False]
    assert info["terminal_obs"].shape == (N, 60) and info["terminal_obs"][2, 0] == 1.0 and obs[2, 0] == 0.0
    packed = torch.zeros((N, 62))
    env.step_packed(packed, actions=torch.zeros(N, 21))
    assert packed[2, 61] == 1.0 and packed[2, 0] == 0.0 and env._terminal[2, 0] == 1.0 and packed[3, 0] == 3.0
    plain = make()
    plain.backend.finish = {2}
    plain.step(torch.zeros(N, 21))
    assert all(not isinstance(c, tuple) for c in plain.backend.calls)      # the default path launches nothing more


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    buf = (C.c_float * 64)()
    assert lib.ss_reset_masked(None, buf, buf, 60, None, None) == -1
    assert lib.ss_get_state_envs(None, buf, 1, buf, None) == -1
    assert lib.ss_set_state_envs(None, buf, 1, buf, None) == -1
