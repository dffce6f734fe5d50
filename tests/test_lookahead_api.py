"""The public surface of the look-ahead, CPU only: the header declares ss_lookahead and its constants under ABI version 4, _lib.py binds
it with matching argument types and the library exports it, SteppingStoneVecEnv.lookahead checks its arguments before anything is
launched, allocates the workspace, reshapes [N,B,H,21] and returns the documented dict (over a fake backend that fills the arrays with
their own flat indices), and over the CPU oracle -- a backend that looks ahead by stepping a saved copy -- a look-ahead predicts the
steps that follow and leaves the env alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle_backend import OracleBackend
from steppingstone_amd import _lib
from steppingstone_amd.envs import SteppingStoneEnv, SteppingStoneVecEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "steppingstone.h")).read()


def test_header_declares_the_entry_point_under_version_4():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name, value in (("SS_LOOK_MAX_STEPS", 1000), ("SS_MAX_EPISODE_STEPS", 1000), ("SS_LOOK_WORK", _lib.LOOK_WORK), ("SS_ABI_VERSION", 4)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), code), name
    decl = re.search(r"int\s+ss_lookahead\s*\(([^)]*)\)\s*;", code)
    assert decl, "ss_lookahead is not declared"
    args = [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",")]
    assert args == ["ss_env* env", "const int32_t* env_ids", "int32_t m", "int32_t horizon", "const float* act", "float* obs", "float* rew",
                    "uint8_t* done", "float* final_state", "float* work", "void* stream"]
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "ss_lookahead" in integration and "lookahead(" in integration


def test_binding_matches_the_declaration_and_a_plain_dlopen_finds_the_symbol():
    lib = _lib.load()
    assert "ss_lookahead" in _lib.SYMBOLS and lib.ss_version() == 4 == _lib.ABI_VERSION
    vp, i32 = C.c_void_p, C.c_int32
    assert lib.ss_lookahead.argtypes == [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    assert (_lib.LOOK_MAX_STEPS, _lib.LOOK_WORK % 4) == (_lib.MAX_EPISODE_STEPS, 0)
    plain = C.CDLL(_lib.LIB_PATH)                     # no prototypes: the bare symbol, as a C client gets it from dlopen / dlsym
    fn = plain.ss_lookahead
    fn.restype = C.c_int
    assert fn(None, None, C.c_int32(0), C.c_int32(1), None, None, None, None, None, None, None) == -1      # a null handle is refused first
    plain.ss_last_error.restype = C.c_char_p
    assert b"null handle" in plain.ss_last_error()


class FakeBackend:
    """HipBackend's call surface as far as lookahead() goes: rew = its flat index, done = 1 from step 2 of every odd row on,
    obs / final_state = their flat indices"""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def close(self):
        pass

    def set_auto_reset(self, on):
        pass

    def lookahead(self, env_ids, m, horizon, act, obs, rew, done, final_state, work):
        assert act.dtype == torch.float32 and act.is_contiguous() and tuple(act.shape) == (m, horizon, 21)
        assert work.dtype == torch.float32 and work.is_contiguous() and tuple(work.shape) == (m, _lib.LOOK_WORK)
        assert rew.dtype == torch.float32 and tuple(rew.shape) == (m, horizon) and rew.is_contiguous()
        assert done.dtype == torch.uint8 and tuple(done.shape) == (m, horizon) and done.is_contiguous()
        assert env_ids is None or (env_ids.dtype == torch.int32 and tuple(env_ids.shape) == (m,))
        self.calls.append((None if env_ids is None else env_ids.clone(), m, horizon, act.clone(), obs is not None, final_state is not None))
        rew.copy_(torch.arange(m * horizon, dtype=torch.float32).reshape(m, horizon))
        done.zero_()
        done[1::2, 2:] = 1
        if obs is not None:
            assert tuple(obs.shape) == (m, horizon, 60) and obs.is_contiguous()
            obs.copy_(torch.arange(obs.numel(), dtype=torch.float32).reshape(obs.shape))
        if final_state is not None:
            assert tuple(final_state.shape) == (m, 186) and final_state.is_contiguous()
            final_state.copy_(torch.arange(final_state.numel(), dtype=torch.float32).reshape(final_state.shape))


@pytest.mark.parametrize("numpy_mode", [False, True])
def test_vecenv_returns_the_documented_dict(numpy_mode):
    be = FakeBackend()
    env = SteppingStoneVecEnv("Walker3DStepperEnv-v0", 5, backend=be, return_numpy=numpy_mode)
    act = np.linspace(-2, 2, 5 * 4 * 21, dtype=np.float32).reshape(5, 4, 21)
    out = env.lookahead(act if numpy_mode else torch.from_numpy(act), final_state=True)
    assert set(out) == {"rew", "done", "ret", "obs", "final_state"}
    as_np = lambda v: v if numpy_mode else v.numpy()
    for k, shape, dt in (("rew", (5, 4), np.float32), ("done", (5, 4), np.bool_), ("ret", (5,), np.float32), ("obs", (5, 4, 60), np.float32),
                         ("final_state", (5, 186), np.float32)):
        assert isinstance(out[k], np.ndarray) == numpy_mode and as_np(out[k]).dtype == dt and as_np(out[k]).shape == shape, k
    ids, m, h, got_act, obs_asked, fs_asked = be.calls[-1]
    assert ids is None and (m, h) == (5, 4) and obs_asked and fs_asked and (got_act.numpy() == act).all()      # unclipped: the kernel clips
    rew = np.arange(20, dtype=np.float32).reshape(5, 4)
    assert (as_np(out["rew"]) == rew).all() and (as_np(out["ret"]) == rew.sum(1)).all()
    assert (as_np(out["done"]) == ((np.arange(5) % 2 == 1)[:, None] & (np.arange(4) >= 2)[None, :])).all()
    assert set(env.lookahead(act, obs=False)) == {"rew", "done", "ret"} and be.calls[-1][4:] == (False, False)


def test_vecenv_takes_branches_per_env_and_repeated_ids():
    be = FakeBackend()
    env = SteppingStoneVecEnv("MikeStepperEnv-v0", 3, backend=be)
    act = torch.arange(3 * 2 * 5 * 21, dtype=torch.float32).reshape(3, 2, 5, 21)
    out = env.lookahead(act, final_state=True)                         # [N, B, H, 21]: B branches of every env
    ids, m, h, got_act, _, _ = be.calls[-1]
    assert ids.tolist() == [0, 0, 1, 1, 2, 2] and (m, h) == (6, 5) and torch.equal(got_act, act.reshape(6, 5, 21))
    assert out["rew"].shape == (3, 2, 5) and out["done"].shape == (3, 2, 5) and out["ret"].shape == (3, 2)
    assert out["obs"].shape == (3, 2, 5, 60) and out["final_state"].shape == (3, 2, 186)
    assert torch.equal(out["rew"], torch.arange(30, dtype=torch.float32).reshape(3, 2, 5))
    assert torch.equal(out["ret"], out["rew"].sum(2))
    out = env.lookahead(act[0, :1].repeat(4, 1, 1), env_ids=[2, 0, 2, 2], obs=False)      # repeated ids are the normal use
    assert be.calls[-1][0].tolist() == [2, 0, 2, 2] and out["rew"].shape == (4, 5)
    out = env.lookahead(act[0], env_ids=torch.tensor([1, 1]))
    assert be.calls[-1][0].tolist() == [1, 1]
    n = len(be.calls)
    assert env.lookahead(torch.zeros((0, 3, 21)), env_ids=[])["rew"].shape == (0, 3) and len(be.calls) == n       # m == 0: no call


def test_bad_arguments_raise_before_anything_is_launched():
    be = FakeBackend()
    env = SteppingStoneVecEnv("Walker3DStepperEnv-v0", 3, backend=be)
    ok = torch.zeros((3, 4, 21))
    for bad in (dict(actions=torch.zeros((3, 0, 21))),                           # horizon 0
                dict(actions=torch.zeros((3, 1001, 21))),                        # beyond SS_LOOK_MAX_STEPS
                dict(actions=torch.zeros((2, 4, 21))),                           # all envs, two rows
                dict(actions=ok, env_ids=[0, 1]),                                # two ids, three rows
                dict(actions=ok, env_ids=[0, 1, 3]),                             # an id out of range
                dict(actions=ok, env_ids=[0, -1, 2]),
                dict(actions=ok, env_ids=[0.5, 1.0, 2.0]),
                dict(actions=torch.zeros((3, 4, 20))),
                dict(actions=torch.zeros((3, 21))),
                dict(actions=torch.zeros((2, 2, 4, 21))),                        # [N,B,H,21] needs N envs
                dict(actions=torch.zeros((3, 2, 4, 21)), env_ids=[0, 1, 2])):    # ... and no env_ids
        with pytest.raises(ValueError):
            env.lookahead(**bad)
    assert be.calls == []
    env.backend = object()
    with pytest.raises(NotImplementedError):
        env.lookahead(ok)
    env.backend = be


def test_single_env_facade_looks_ahead_from_its_one_env():
    made = []

    def factory(kind, n, seed):
        made.append(FakeBackend())
        return made[-1]
    env = SteppingStoneEnv("Walker3DStepperEnv-v0", backend_factory=factory)
    out = env.lookahead(np.zeros((7, 3, 21)), final_state=True)
    assert made[-1].calls[-1][0].tolist() == [0] * 7 and out["rew"].shape == (7, 3) and out["ret"].shape == (7,)
    assert out["obs"].shape == (7, 3, 60) and out["final_state"].shape == (7, 186)
    assert env.lookahead(np.zeros((3, 21)), obs=False)["done"].shape == (1, 3)


class Backend(OracleBackend):
    """the CPU oracle plus lookahead() by stepping a saved copy: for the p-th row of every env one pass of H real steps with auto-reset
    off from the saved state, then the state (RNG counters included) goes back"""
    def __init__(self, kind, n, seed):
        super().__init__(kind, n, seed)
        self.auto = True

    def set_auto_reset(self, on):
        self.auto = bool(on)
        super().set_auto_reset(on)

    def lookahead(self, env_ids, m, horizon, act, obs, rew, done, final_state, work):
        ids = np.arange(m) if env_ids is None else env_ids.numpy()
        saved = self.o.get_state()
        self.o.set_auto_reset(False)
        nth = np.zeros(m, int)
        seen = {}
        for k, i in enumerate(ids):
            nth[k] = seen.get(int(i), 0)
            seen[int(i)] = nth[k] + 1
        for p in range(nth.max() + 1 if m else 0):
            rows = np.nonzero(nth == p)[0]
            envs = ids[rows]
            self.o.set_state(saved)
            a = np.zeros((self.n, 21), np.float32)
            fin = np.zeros(rows.size, bool)
            for s in range(horizon):
                a[envs] = act[rows, s].numpy()
                o, r, d, _ = self.o.step(a)
                st = self.o.get_state().astype(np.float32)
                for j, (k, e) in enumerate(zip(rows, envs)):
                    if fin[j]:
                        rew[k, s], done[k, s] = 0.0, 1
                        if obs is not None:
                            obs[k, s] = obs[k, s - 1]
                        continue
                    rew[k, s], done[k, s] = float(r[e]), int(d[e])
                    if obs is not None:
                        obs[k, s] = torch.from_numpy(o[e])
                    if final_state is not None:
                        final_state[k] = torch.from_numpy(st[e])
                    fin[j] = bool(d[e])
        self.o.set_state(saved)
        self.o.set_auto_reset(self.auto)


def test_a_lookahead_over_the_oracle_predicts_the_steps_and_leaves_the_env_alone():
    n, h = 4, 6
    be = Backend("walker3d", n, 3)
    env = SteppingStoneVecEnv("Walker3DStepperEnv-v0", n, seed=3, backend=be)
    env.set_auto_reset(False)
    env.reset()
    rng = np.random.default_rng(1)
    act = torch.from_numpy(rng.uniform(-1, 1, (n, 2, h, 21)).astype(np.float32))
    before = env.get_state().clone()
    out = env.lookahead(act, final_state=True)
    assert torch.equal(env.get_state(), before), "the look-ahead moved the env"
    for s in range(h):                                 # branch 1 of every env is what really happens next
        obs, rew, done, _ = env.step(act[:, 1, s])
        live = ~out["done"][:, 1, :s].any(1)
        assert torch.equal(out["rew"][live, 1, s], rew[live]) and torch.equal(out["done"][live, 1, s], done.bool()[live])
        assert torch.equal(out["obs"][live, 1, s], obs[live])
    assert live.any() and torch.equal(out["final_state"][live, 1], env.get_state()[live])
    assert not torch.equal(out["rew"][:, 0], out["rew"][:, 1])
    assert torch.allclose(out["ret"], out["rew"].sum(2))
    env.close()
