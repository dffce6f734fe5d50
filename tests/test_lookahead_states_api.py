"""The public surface of the look-ahead from caller-supplied states and of the observation of state rows, CPU only: the header declares
ss_lookahead_states and ss_get_obs_states under ABI version 4 with exactly the documented argument lists, _lib.py binds them with
matching argument types and the library exports them; SteppingStoneVecEnv.lookahead(states=...) and observe() check their arguments
before anything is launched, reshape [N,B,186] next to [N,B,H,21] and return the documented results over a fake backend; without
`states` the nine-argument backend.lookahead of the existing backends is still what is called."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from steppingstone_amd import _lib
from steppingstone_amd.envs import SteppingStoneEnv, SteppingStoneVecEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "steppingstone.h")).read()
LOOK_ARGS = ["ss_env* env", "const int32_t* env_ids", "int32_t m", "const float* states", "int32_t horizon", "const float* act", "float* obs",
             "float* rew", "uint8_t* done", "float* final_state", "float* work", "void* stream"]
OBS_ARGS = ["ss_env* env", "int32_t m", "const float* states", "float* obs", "void* stream"]


def test_header_declares_both_calls_under_version_4():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert re.search(r"#define\s+SS_ABI_VERSION\s+4\b", code) and re.search(r"#define\s+SS_STATE_DIM\s+186\b", code)
    for name, want in (("ss_lookahead_states", LOOK_ARGS), ("ss_get_obs_states", OBS_ARGS)):
        decl = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert decl, "%s is not declared" % name
        assert [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",")] == want, name
    for doc in ("INTEGRATION.md", "README.md", os.path.join("docs", "PHYSICS.md")):
        text = open(os.path.join(ROOT, doc)).read()
        assert "ss_lookahead_states" in text and "ss_get_obs_states" in text, doc


def test_binding_matches_the_declarations_and_a_plain_dlopen_finds_the_symbols():
    lib = _lib.load()
    assert {"ss_lookahead_states", "ss_get_obs_states"} <= set(_lib.SYMBOLS) and lib.ss_version() == 4 == _lib.ABI_VERSION
    vp, i32 = C.c_void_p, C.c_int32
    assert lib.ss_lookahead_states.argtypes == [vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    assert lib.ss_get_obs_states.argtypes == [vp, i32, vp, vp, vp]
    plain = C.CDLL(_lib.LIB_PATH)                     # no prototypes: the bare symbols, as a C client gets them from dlopen / dlsym
    plain.ss_last_error.restype = C.c_char_p
    look, obs = plain.ss_lookahead_states, plain.ss_get_obs_states
    look.restype = obs.restype = C.c_int
    assert look(None, None, C.c_int32(0), None, C.c_int32(1), None, None, None, None, None, None, None) == -1      # a null handle is refused first
    assert b"null handle" in plain.ss_last_error()
    assert obs(None, C.c_int32(0), None, None, None) == -1
    assert b"null handle" in plain.ss_last_error()


class OldBackend:
    """the call surface of the backends that existed before `states`: the nine-argument lookahead and nothing else"""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def close(self):
        pass

    def set_auto_reset(self, on):
        pass

    def lookahead(self, env_ids, m, horizon, act, obs, rew, done, final_state, work):
        self.calls.append(("lookahead", None if env_ids is None else env_ids.tolist(), m, horizon))
        rew.copy_(torch.arange(m * horizon, dtype=torch.float32).reshape(m, horizon))
        done.zero_()


class FakeBackend(OldBackend):
    """... plus the two new calls: rew = its flat index + the first word of the row's state, final_state = the state row + 1,
    obs (observe) = word 1 of the state row in every column"""
    def lookahead_states(self, env_ids, m, states, horizon, act, obs, rew, done, final_state, work):
        assert states.dtype == torch.float32 and states.is_contiguous() and tuple(states.shape) == (m, 186)
        assert act.dtype == torch.float32 and act.is_contiguous() and tuple(act.shape) == (m, horizon, 21)
        assert work.dtype == torch.float32 and work.is_contiguous() and tuple(work.shape) == (m, _lib.LOOK_WORK)
        assert rew.dtype == torch.float32 and tuple(rew.shape) == (m, horizon) and done.dtype == torch.uint8 and tuple(done.shape) == (m, horizon)
        assert env_ids is None or (env_ids.dtype == torch.int32 and tuple(env_ids.shape) == (m,))
        self.calls.append(("lookahead_states", None if env_ids is None else env_ids.tolist(), m, horizon, states.clone(), act.clone(),
                           obs is not None, final_state is not None))
        rew.copy_(torch.arange(m * horizon, dtype=torch.float32).reshape(m, horizon) + states[:, :1])
        done.zero_()
        done[1::2, 2:] = 1
        if obs is not None:
            assert tuple(obs.shape) == (m, horizon, 60) and obs.is_contiguous()
            obs.copy_(torch.arange(obs.numel(), dtype=torch.float32).reshape(obs.shape))
        if final_state is not None:
            assert tuple(final_state.shape) == (m, 186) and final_state.is_contiguous()
            final_state.copy_(states + 1)

    def get_obs_states(self, m, states, obs):
        assert states.dtype == torch.float32 and states.is_contiguous() and tuple(states.shape) == (m, 186)
        assert obs.dtype == torch.float32 and obs.is_contiguous() and tuple(obs.shape) == (m, 60)
        self.calls.append(("get_obs_states", m, states.clone()))
        obs.copy_(states[:, 1:2].expand(m, 60))


def rows(*lead):
    n = int(np.prod(lead))
    return (1000.0 * np.arange(n, dtype=np.float32)[:, None] + np.arange(186, dtype=np.float32)[None, :]).reshape(lead + (186,))


@pytest.mark.parametrize("numpy_mode", [False, True])
def test_vecenv_returns_the_documented_dict(numpy_mode):
    be = FakeBackend()
    env = SteppingStoneVecEnv("Walker3DStepperEnv-v0", 5, backend=be, return_numpy=numpy_mode)
    act = np.linspace(-2, 2, 5 * 4 * 21, dtype=np.float32).reshape(5, 4, 21)
    st = rows(5)
    give = (lambda a: a) if numpy_mode else torch.from_numpy
    out = env.lookahead(give(act), final_state=True, states=give(st))
    assert set(out) == {"rew", "done", "ret", "obs", "final_state"}
    as_np = lambda v: v if numpy_mode else v.numpy()
    for k, shape, dt in (("rew", (5, 4), np.float32), ("done", (5, 4), np.bool_), ("ret", (5,), np.float32), ("obs", (5, 4, 60), np.float32),
                         ("final_state", (5, 186), np.float32)):
        assert isinstance(out[k], np.ndarray) == numpy_mode and as_np(out[k]).dtype == dt and as_np(out[k]).shape == shape, k
    name, ids, m, h, got_st, got_act, obs_asked, fs_asked = be.calls[-1]
    assert name == "lookahead_states" and ids is None and (m, h) == (5, 4) and obs_asked and fs_asked
    assert (got_st.numpy() == st).all() and (got_act.numpy() == act).all()
    rew = np.arange(20, dtype=np.float32).reshape(5, 4) + st[:, :1]
    assert (as_np(out["rew"]) == rew).all() and (as_np(out["ret"]) == rew.sum(1)).all() and (as_np(out["final_state"]) == st + 1).all()
    # a tensor for the one, an array for the other; repeated ids, each row with its own state
    out = env.lookahead(torch.from_numpy(act[:3]), env_ids=[4, 4, 1], obs=False, states=st[[2, 0, 3]])
    assert set(out) == {"rew", "done", "ret"} and be.calls[-1][:4] == ("lookahead_states", [4, 4, 1], 3, 4)
    assert (be.calls[-1][4].numpy() == st[[2, 0, 3]]).all() and be.calls[-1][6:] == (False, False)
    # a non-contiguous view of a final_state tensor is taken as its rows
    wide = torch.from_numpy(np.concatenate([st, st], 1))
    env.lookahead(act, obs=False, states=wide[:, 186:])
    assert (be.calls[-1][4].numpy() == st).all()
    n = len(be.calls)
    assert env.lookahead(np.zeros((0, 3, 21), np.float32), env_ids=[], states=rows(0))["rew"].shape == (0, 3) and len(be.calls) == n


def test_vecenv_reshapes_states_next_to_branches_per_env():
    be = FakeBackend()
    env = SteppingStoneVecEnv("MikeStepperEnv-v0", 3, backend=be)
    act = torch.arange(3 * 2 * 5 * 21, dtype=torch.float32).reshape(3, 2, 5, 21)
    st = rows(3, 2)
    out = env.lookahead(act, final_state=True, states=st)
    name, ids, m, h, got_st, got_act, _, _ = be.calls[-1]
    assert name == "lookahead_states" and ids == [0, 0, 1, 1, 2, 2] and (m, h) == (6, 5)
    assert torch.equal(got_act, act.reshape(6, 5, 21)) and (got_st.numpy() == st.reshape(6, 186)).all()
    assert out["rew"].shape == (3, 2, 5) and out["ret"].shape == (3, 2) and out["obs"].shape == (3, 2, 5, 60)
    assert out["final_state"].shape == (3, 2, 186) and (out["final_state"].numpy() == st + 1).all()


def test_without_states_the_nine_argument_lookahead_is_called():
    for be in (OldBackend(), FakeBackend()):
        env = SteppingStoneVecEnv("Walker3DStepperEnv-v0", 3, backend=be)
        out = env.lookahead(torch.zeros((3, 4, 21)), obs=False)
        assert be.calls == [("lookahead", None, 3, 4)] and out["rew"].shape == (3, 4)
        env.lookahead(torch.zeros((2, 4, 21)), env_ids=[2, 2], obs=False, states=None)
        assert be.calls[-1] == ("lookahead", [2, 2], 2, 4)
    old = SteppingStoneVecEnv("Walker3DStepperEnv-v0", 3, backend=OldBackend())
    with pytest.raises(NotImplementedError):
        old.lookahead(torch.zeros((3, 4, 21)), states=rows(3))
    with pytest.raises(NotImplementedError):
        old.observe(rows(3))
    assert old.backend.calls == []


def test_observe_returns_one_row_per_state():
    be = FakeBackend()
    for numpy_mode in (False, True):
        env = SteppingStoneVecEnv("Walker3DStepperEnv-v0", 2, backend=be, return_numpy=numpy_mode)
        st = rows(7)                                                     # m is the caller's: more rows than envs
        out = env.observe(st if numpy_mode else torch.from_numpy(st))
        assert isinstance(out, np.ndarray) == numpy_mode and tuple(out.shape) == (7, 60) and be.calls[-1][:2] == ("get_obs_states", 7)
        assert (np.asarray(out) == st[:, 1:2]).all()
        n = len(be.calls)
        assert tuple(env.observe(rows(0)).shape) == (0, 60) and len(be.calls) == n      # m == 0: no call


def test_bad_states_raise_before_anything_is_launched():
    be = FakeBackend()
    env = SteppingStoneVecEnv("Walker3DStepperEnv-v0", 3, backend=be)
    ok = torch.zeros((3, 4, 21))
    many = torch.zeros((3, 2, 4, 21))
    for bad in (dict(actions=ok, states=rows(2)),                                  # three branches, two rows
                dict(actions=ok, states=rows(3)[:, :185]),                         # a short row
                dict(actions=ok, states=rows(3).reshape(-1)),                      # flat
                dict(actions=ok, states=rows(3).astype(np.float64)),               # not float32
                dict(actions=ok, states=torch.zeros((3, 186), dtype=torch.int32)),
                dict(actions=ok, states=rows(3).tolist()),                         # neither a tensor nor an array
                dict(actions=ok, states=rows(3, 1)),                               # [N,B,186] needs [N,B,H,21]
                dict(actions=ok, env_ids=[0, 1], states=rows(2)),                  # (the actions do not fit the ids)
                dict(actions=ok[:2], env_ids=[0, 1], states=rows(3)),
                dict(actions=many, states=rows(6)),                                # [N,B,H,21] needs [N,B,186]
                dict(actions=many, states=rows(3, 3)),
                dict(actions=many, states=rows(2, 3))):
        with pytest.raises(ValueError):
            env.lookahead(**bad)
    for bad in (rows(3)[:, :60], rows(3).reshape(-1), rows(3, 2), rows(3).astype(np.float64), rows(3).tolist(), None):
        with pytest.raises(ValueError):
            env.observe(bad)
    assert be.calls == []


def test_single_env_facade_takes_states():
    made = []

    def factory(kind, n, seed):
        made.append(FakeBackend())
        return made[-1]
    env = SteppingStoneEnv("Walker3DStepperEnv-v0", backend_factory=factory)
    st = rows(7)
    out = env.lookahead(np.zeros((7, 3, 21)), final_state=True, states=st)
    call = made[-1].calls[-1]
    assert call[:4] == ("lookahead_states", [0] * 7, 7, 3) and (call[4].numpy() == st).all()
    assert out["rew"].shape == (7, 3) and out["final_state"].shape == (7, 186)
    assert env.lookahead(np.zeros((3, 21)), obs=False, states=st[2])["done"].shape == (1, 3)
    assert (made[-1].calls[-1][4].numpy() == st[2:3]).all()
    assert env.lookahead(np.zeros((3, 21)), obs=False)["done"].shape == (1, 3) and made[-1].calls[-1][0] == "lookahead"
    assert tuple(np.asarray(env.observe(st)).shape) == (7, 60) and tuple(np.asarray(env.observe(st[4])).shape) == (60,)
    assert (np.asarray(env.observe(st[4])) == st[4, 1]).all()
