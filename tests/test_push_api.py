"""The public surface of the push, CPU only: the header declares ss_push and its constant under ABI version 4, _lib.py binds it with
matching argument types, SteppingStoneVecEnv.push turns its argument forms (impulse [m,3] / [m,6]; body an index, a name or m of them;
point; env_ids; apply) into the call's arrays -- over a fake backend that records them -- and enjoy parses --push."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from steppingstone_amd import _lib, enjoy, model
from steppingstone_amd.envs import SteppingStoneEnv, SteppingStoneVecEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "steppingstone.h")).read()


def test_header_declares_the_entry_point_under_version_4():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert re.search(r"#define\s+SS_PUSH_WRENCH\s+6\b", code) and re.search(r"#define\s+SS_ABI_VERSION\s+4\b", code)
    decl = re.search(r"int\s+ss_push\s*\(([^)]*)\)\s*;", code)
    assert decl, "ss_push is not declared"
    args = [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",")]
    assert args == ["ss_env* env", "const int32_t* env_ids", "int32_t m", "const int32_t* body", "const float* point",
                    "const float* impulse", "float* delta_nu", "int32_t apply", "void* stream"]
    version = HEADER[HEADER.index("#define SS_ABI_VERSION"):HEADER.index("#define SS_MAX_EPISODE_STEPS")]
    assert "ss_push" in version, "the version comment lists what was added under version 4"
    text = HEADER[HEADER.index("Impulse: push body"):HEADER.index("#define SS_PUSH_WRENCH")].lower()
    assert "armature" in text and "dry run" in text and "centre of mass" in text


def test_binding_matches_the_declaration():
    lib = _lib.load()
    assert "ss_push" in _lib.SYMBOLS and lib.ss_version() == 4 == _lib.ABI_VERSION
    vp, i32 = C.c_void_p, C.c_int32
    assert lib.ss_push.argtypes == [vp, vp, i32, vp, vp, vp, vp, i32, vp]
    assert _lib.PUSH_WRENCH == 6
    assert lib.ss_push(None, None, 0, None, None, None, None, 0, None) == -1         # a null handle is refused before anything else
    assert b"null handle" in lib.ss_last_error()


def test_body_names():
    assert len(model.BODY_NAMES) == model.NB == _lib.NUM_BODIES and len(set(model.BODY_NAMES)) == model.NB
    assert model.BODY_NAMES[0] == "torso" and model.BODY_NAMES[model.RIGHT_FOOT_BODY] == "right_foot"
    assert model.BODY_NAMES[model.LEFT_FOOT_BODY] == "left_foot"
    m = model.build("walker3d")
    for b in range(1, model.NB):                 # a massless intermediate link carries its joint's name, every other body its own
        assert (model.BODY_NAMES[b] == model.JOINT_NAMES[b - 1]) == (m["mass"][b] == 0), b


class FakeBackend:
    """HipBackend's call surface as far as push() goes; delta_nu word = its flat index"""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def close(self):
        pass

    def set_auto_reset(self, on):
        pass

    def push(self, env_ids, m, body, point, impulse, delta_nu, apply):
        for t, width, dt in ((env_ids, None, torch.int32), (body, None, torch.int32), (point, 3, torch.float32), (impulse, 6, torch.float32),
                             (delta_nu, 27, torch.float32)):
            if t is not None:
                assert t.dtype == dt and t.is_contiguous() and t.shape[0] == m and (width is None or tuple(t.shape) == (m, width))
        cl = lambda t: None if t is None else t.clone()
        self.calls.append(dict(ids=cl(env_ids), m=m, body=cl(body), point=cl(point), impulse=cl(impulse), apply=apply))
        delta_nu.copy_(torch.arange(delta_nu.numel(), dtype=torch.float32).reshape(delta_nu.shape))


class NoPushBackend:
    device = torch.device("cpu")

    def close(self):
        pass

    def set_auto_reset(self, on):
        pass


@pytest.mark.parametrize("numpy_mode", [False, True])
def test_vecenv_push_argument_forms(numpy_mode):
    be = FakeBackend()
    env = SteppingStoneVecEnv("Walker3DStepperEnv-v0", 5, backend=be, return_numpy=numpy_mode)
    out = env.push(np.arange(15, dtype=np.float32).reshape(5, 3))
    assert (isinstance(out, np.ndarray) if numpy_mode else torch.is_tensor(out)) and tuple(out.shape) == (5, 27)
    assert (np.asarray(out) == np.arange(5 * 27).reshape(5, 27)).all()
    c = be.calls[-1]
    assert c["ids"] is None and c["m"] == 5 and c["body"] is None and c["point"] is None and c["apply"] is True
    assert (c["impulse"][:, :3].numpy() == np.arange(15).reshape(5, 3)).all() and (c["impulse"][:, 3:] == 0).all()
    env.push(torch.ones(3, 6), env_ids=[4, 0, 3], body="left_foot", point=[0.1, 0.0, -0.2], apply=False)
    c = be.calls[-1]
    assert c["ids"].tolist() == [4, 0, 3] and c["m"] == 3 and c["body"].tolist() == [model.LEFT_FOOT_BODY] * 3 and c["apply"] is False
    assert torch.allclose(c["point"], torch.tensor([[0.1, 0.0, -0.2]] * 3)) and (c["impulse"] == 1).all()
    env.push(np.ones((2, 6), np.float32), env_ids=[1, 2], body=["pelvis", 7], point=np.zeros((2, 3)))
    assert be.calls[-1]["body"].tolist() == [3, 7]
    env.push(np.ones((2, 3)), env_ids=[1, 2], body=np.array([0, 0]))
    assert be.calls[-1]["body"] is None, "the torso everywhere is the call's NULL"
    n = len(be.calls)
    assert tuple(env.push(np.zeros((0, 6)), env_ids=[]).shape) == (0, 27) and len(be.calls) == n      # m == 0: nothing is launched
    for kw in (dict(impulse=np.ones((5, 4))), dict(impulse=np.ones((4, 3))), dict(impulse=np.ones((5, 3)), body=22),
               dict(impulse=np.ones((5, 3)), body="tail"), dict(impulse=np.ones((5, 3)), body=[0, 1]),
               dict(impulse=np.ones((5, 3)), body=1.5), dict(impulse=np.ones((5, 3)), point=np.zeros((4, 3))),
               dict(impulse=np.ones((1, 3)), env_ids=[5]), dict(impulse=np.ones((2, 3)), env_ids=[1, 1])):
        with pytest.raises(ValueError):
            env.push(**kw)
    assert len(be.calls) == n


def test_single_env_facade_and_a_backend_without_the_call():
    be = FakeBackend()
    env = SteppingStoneEnv("Walker3DStepperEnv-v0", backend_factory=lambda *a, **k: be)
    out = env.push([0.0, 30.0, 0.0], body="torso", apply=False)
    assert isinstance(out, np.ndarray) and out.shape == (27,)
    c = be.calls[-1]
    assert c["m"] == 1 and c["impulse"].tolist() == [[0.0, 30.0, 0.0, 0.0, 0.0, 0.0]] and c["apply"] is False
    env.push(np.ones(6), body=8, point=[0.0, 0.0, 0.1])
    assert be.calls[-1]["body"].tolist() == [8] and be.calls[-1]["point"].shape == (1, 3)
    bare = SteppingStoneVecEnv("MikeStepperEnv-v0", 2, backend=NoPushBackend())
    with pytest.raises(NotImplementedError):
        bare.push(np.zeros((2, 3)))


def test_enjoy_parses_push():
    assert enjoy.parse_push("120:torso:0,30,0") == (120, 0, [0.0, 30.0, 0.0])
    assert enjoy.parse_push("5:13:-1.5,0,2e1") == (5, 13, [-1.5, 0.0, 20.0])
    for bad in ("torso:0,30,0", "5:tail:0,0,0", "5:22:0,0,0", "5:0:1,2", "-1:0:1,2,3", "x:0:1,2,3"):
        with pytest.raises(ValueError):
            enjoy.parse_push(bad)
