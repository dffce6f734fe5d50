"""The public surface of the closed-loop look-ahead, CPU only: the header declares ss_policy_words, ss_policy_pack and
ss_lookahead_policy under ABI version 4 with the documented argument lists and _lib.py binds them with matching types; pack_policy takes
the documented sources and refuses everything else with an error that names them; SteppingStoneVecEnv.lookahead_policy checks its
arguments before anything is launched, reshapes the [N,B] forms and returns the documented dict over a fake backend; a backend without
the call raises NotImplementedError."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from steppingstone_amd import _lib, ppo
from steppingstone_amd.envs import PackedPolicy, SteppingStoneEnv, SteppingStoneVecEnv, pack_policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "steppingstone.h")).read()
LOOK_ARGS = ["ss_env* env", "const int32_t* env_ids", "int32_t m", "const float* states", "int32_t horizon", "const ss_policy_desc* d",
             "const float* packed", "const float* act_offset", "float* act", "float* obs", "float* rew", "uint8_t* done", "float* final_state",
             "float* work", "void* stream"]
PACK_ARGS = ["ss_env* env", "const ss_policy_desc* d", "const float* const* weight", "const float* const* bias", "float* packed", "void* stream"]


def test_header_and_binding():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert re.search(r"#define\s+SS_ABI_VERSION\s+4\b", code)
    assert re.search(r"#define\s+SS_POLICY_MAX_LAYERS\s+8\b", code) and re.search(r"#define\s+SS_POLICY_MAX_WIDTH\s+256\b", code)
    assert re.search(r"SS_POLICY_IDENTITY = 0, SS_POLICY_RELU = 1, SS_POLICY_SOFTSIGN = 2, SS_POLICY_TANH = 3", code)
    for name, want in (("ss_lookahead_policy", LOOK_ARGS), ("ss_policy_pack", PACK_ARGS)):
        decl = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert decl, "%s is not declared" % name
        assert [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",")] == want, name
    assert re.search(r"int64_t\s+ss_policy_words\s*\(\s*const ss_policy_desc\* d\s*\)\s*;", code)
    lib = _lib.load()
    vp, i32 = C.c_void_p, C.c_int32
    assert lib.ss_lookahead_policy.argtypes == [vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    assert lib.ss_policy_pack.argtypes == [vp] * 6 and lib.ss_policy_words.restype == C.c_int64
    assert (_lib.POLICY_IDENTITY, _lib.POLICY_RELU, _lib.POLICY_SOFTSIGN, _lib.POLICY_TANH) == (0, 1, 2, 3)
    for doc in ("INTEGRATION.md", "README.md", os.path.join("docs", "PHYSICS.md"), "DESIGN.md"):
        assert "ss_lookahead_policy" in open(os.path.join(ROOT, doc)).read(), doc


class OldBackend:
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def close(self):
        pass

    def set_auto_reset(self, on):
        pass

    def lookahead(self, env_ids, m, horizon, act, obs, rew, done, final_state, work):
        self.calls.append("lookahead")


class FakeBackend(OldBackend):
    def policy_pack(self, desc, weights, biases, packed):
        assert len(weights) == len(biases) == desc.layers and all(w.is_contiguous() and w.dtype == torch.float32 for w in weights + biases)
        self.calls.append(("policy_pack", desc.layers, [tuple(w.shape) for w in weights]))
        packed.fill_(float(sum(float(w.sum()) for w in weights)))

    def lookahead_policy(self, env_ids, m, states, horizon, desc, packed, offsets, act, obs, rew, done, final_state, work):
        assert tuple(rew.shape) == (m, horizon) and done.dtype == torch.uint8 and tuple(work.shape) == (m, _lib.LOOK_WORK)
        assert env_ids is None or (env_ids.dtype == torch.int32 and tuple(env_ids.shape) == (m,))
        assert states is None or (tuple(states.shape) == (m, 186) and states.is_contiguous())
        assert offsets is None or (tuple(offsets.shape) == (m, horizon, 21) and offsets.is_contiguous())
        self.calls.append(("lookahead_policy", None if env_ids is None else env_ids.tolist(), m, horizon, states is not None,
                           offsets is not None, act is not None, obs is not None, final_state is not None, float(packed[0])))
        rew.copy_(torch.arange(m * horizon, dtype=torch.float32).reshape(m, horizon))
        done.zero_()
        if act is not None:
            act.copy_(torch.zeros_like(act) if offsets is None else offsets)
        if final_state is not None:
            final_state.copy_(states + 1 if states is not None else torch.zeros_like(final_state))


def triples(widths=(60, 8, 21), acts=("relu", "tanh")):
    return [(np.full((widths[i + 1], widths[i]), 0.5 + i, np.float32), np.zeros(widths[i + 1], np.float32), acts[i]) for i in range(len(acts))]


def test_pack_policy_sources():
    nn = torch.nn
    ac = ppo.ActorCritic()
    for src, layers, widths in ((ac, 6, [60] + [256] * 5 + [21]), (ac.actor, 6, [60] + [256] * 5 + [21]),
                                (nn.Sequential(nn.Linear(60, 37), nn.Softsign(), nn.Linear(37, 50), nn.Identity(), nn.Linear(50, 21)), 3, [60, 37, 50, 21]),
                                (triples(), 2, [60, 8, 21])):
        p = pack_policy(src, "cpu")
        assert isinstance(p, PackedPolicy) and p.desc.layers == layers and list(p.desc.width[:layers + 1]) == widths
        assert p.blob.dtype == torch.float32 and p.blob.numel() == _lib.load().ss_policy_words(C.byref(p.desc)) and p.blob.data_ptr() % 16 == 0
    assert list(pack_policy(ac, "cpu").desc.activation[:6]) == [2, 2, 2, 1, 1, 3]
    seq = pack_policy(nn.Sequential(nn.Linear(60, 37), nn.Softsign(), nn.Linear(37, 50), nn.Identity(), nn.Linear(50, 21)), "cpu")
    assert list(seq.desc.activation[:3]) == [2, 0, 0]
    for bad in (nn.Linear(60, 21), nn.Sequential(nn.ReLU(), nn.Linear(60, 21)), nn.Sequential(nn.Linear(60, 21), nn.Tanh(), nn.Tanh()),
                nn.Sequential(nn.Linear(60, 21, bias=False)), nn.Sequential(nn.Linear(60, 21), nn.GELU()), triples(acts=("relu", "gelu")),
                triples((59, 8, 21)), triples((60, 8, 22)), triples((60, 300, 21)), [], None, ac.critics[0],
                [(np.zeros((8, 60), np.float32), np.zeros(9, np.float32), "relu"), (np.zeros((21, 8), np.float32), np.zeros(21, np.float32), "tanh")],
                [(np.zeros((8, 60), np.float32), np.zeros(8, np.float32), "relu"), (np.zeros((21, 9), np.float32), np.zeros(21, np.float32), "tanh")]):
        with pytest.raises(ValueError, match="supported"):
            pack_policy(bad, "cpu")


@pytest.mark.parametrize("numpy_mode", [False, True])
def test_vecenv_returns_the_documented_dict(numpy_mode):
    be = FakeBackend()
    env = SteppingStoneVecEnv("Walker3DStepperEnv-v0", 5, backend=be, return_numpy=numpy_mode)
    pol = pack_policy(triples(), "cpu")
    assert be.calls == []                                            # packed at first use
    out = env.lookahead_policy(pol, 4)
    assert be.calls[0][:2] == ("policy_pack", 2) and be.calls[1][:9] == ("lookahead_policy", None, 5, 4, False, False, True, True, False)
    assert set(out) == {"rew", "done", "ret", "obs", "act"}
    as_np = lambda v: v if numpy_mode else v.numpy()
    for k, shape, dt in (("rew", (5, 4), np.float32), ("done", (5, 4), np.bool_), ("ret", (5,), np.float32), ("obs", (5, 4, 60), np.float32),
                         ("act", (5, 4, 21), np.float32)):
        assert isinstance(out[k], np.ndarray) == numpy_mode and as_np(out[k]).dtype == dt and as_np(out[k]).shape == shape, k
    env.lookahead_policy(pol, 4, obs=False)
    assert len(be.calls) == 3, "a packed policy is not packed again"
    first = be.calls[-1][-1]
    pol._layers[0][0][:] = 2.0
    pol.refresh()
    env.lookahead_policy(pol, 4, obs=False, actions=False, final_state=True, env_ids=[4, 4, 1])
    assert be.calls[-2][0] == "policy_pack" and be.calls[-1][1:9] == ([4, 4, 1], 3, 4, False, False, False, False, True)
    assert be.calls[-1][-1] != first, "refresh() repacks from the same arrays"
    off = np.arange(5 * 2 * 4 * 21, dtype=np.float32).reshape(5, 2, 4, 21)
    st = np.arange(5 * 2 * 186, dtype=np.float32).reshape(5, 2, 186)
    out = env.lookahead_policy(pol, 4, offsets=off if numpy_mode else torch.from_numpy(off), states=st, final_state=True)
    assert be.calls[-1][1:6] == ([0, 0, 1, 1, 2, 2, 3, 3, 4, 4], 10, 4, True, True)
    assert as_np(out["act"]).shape == (5, 2, 4, 21) and (as_np(out["act"]) == off).all() and (as_np(out["final_state"]) == st + 1).all()
    assert as_np(out["ret"]).shape == (5, 2)
    n = len(be.calls)
    assert as_np(env.lookahead_policy(pol, 3, env_ids=[])["act"]).shape == (0, 3, 21) and len(be.calls) == n
    env.lookahead_policy(triples(), 2)                                # anything pack_policy takes
    assert be.calls[-2][0] == "policy_pack"


def test_bad_arguments_raise_before_anything_is_launched():
    be = FakeBackend()
    env = SteppingStoneVecEnv("Walker3DStepperEnv-v0", 3, backend=be)
    pol = pack_policy(triples(), "cpu")
    z = lambda *s: np.zeros(s, np.float32)
    for bad in (dict(horizon=0), dict(horizon=1001), dict(horizon=4, offsets=z(3, 5, 21)), dict(horizon=4, offsets=z(2, 4, 21)),
                dict(horizon=4, offsets=z(3, 4, 21).astype(np.float64)), dict(horizon=4, offsets=z(3, 4, 21).tolist()),
                dict(horizon=4, states=z(2, 186)), dict(horizon=4, states=z(3, 185)), dict(horizon=4, states=z(3, 186).astype(np.float64)),
                dict(horizon=4, env_ids=[0, 3]), dict(horizon=4, env_ids=[0.5]), dict(horizon=4, env_ids=[0, 1], offsets=z(3, 4, 21)),
                dict(horizon=4, env_ids=[0, 1], offsets=z(3, 2, 4, 21)), dict(horizon=4, offsets=z(3, 2, 4, 21), states=z(3, 3, 186)),
                dict(horizon=4, offsets=z(2, 2, 4, 21)), dict(horizon=4, states=z(3, 2, 186), offsets=z(3, 4, 21))):
        with pytest.raises(ValueError):
            env.lookahead_policy(pol, **bad)
    with pytest.raises(ValueError, match="supported"):
        env.lookahead_policy("actor", 4)
    assert be.calls == []
    old = SteppingStoneVecEnv("Walker3DStepperEnv-v0", 3, backend=OldBackend())
    with pytest.raises(NotImplementedError):
        old.lookahead_policy(pol, 4)
    assert old.backend.calls == []


def test_single_env_facade():
    made = []

    def factory(kind, n, seed):
        made.append(FakeBackend())
        return made[-1]
    env = SteppingStoneEnv("Walker3DStepperEnv-v0", backend_factory=factory)
    out = env.lookahead_policy(triples(), 3, branches=4)
    assert made[-1].calls[-1][1:4] == ([0] * 4, 4, 3) and out["act"].shape == (4, 3, 21)
    out = env.lookahead_policy(triples(), 3, offsets=np.ones((3, 21), np.float32), states=np.zeros(186, np.float32), final_state=True)
    assert made[-1].calls[-1][1:6] == ([0], 1, 3, True, True) and out["final_state"].shape == (1, 186) and (out["act"] == 1).all()
