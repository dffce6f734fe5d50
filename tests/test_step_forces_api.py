"""The public surface of the force readout, CPU only: the header declares ss_step_forces and its constants under ABI version 4, _lib.py
binds it with matching argument types, SteppingStoneVecEnv.step_forces turns the three output arrays into the documented dict and passes
env_ids and the actions through (over a fake backend that fills the arrays with their own flat indices), and `enjoy --trace --forces`
writes the readout of the state each step starts in next to today's trace keys."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import forces_host_lib as fh
import kinematics_host_lib as kh
import native_build
import np_kinematics as nk
from oracle_backend import OracleBackend
from steppingstone_amd import _lib, enjoy, ppo
from steppingstone_amd.envs import SteppingStoneEnv, SteppingStoneVecEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "steppingstone.h")).read()
KEYS = {"contact_slot": ((4, 8), torch.int32), "contact_pen": ((4, 8), torch.float32), "contact_force": ((4, 8, 3), torch.float32),
        "contact_force_world": ((4, 8, 3), torch.float32), "joint_q": ((4, 21), torch.float32), "joint_qd": ((4, 21), torch.float32),
        "joint_tau": ((4, 21), torch.float32), "joint_torque": ((4, 21), torch.float32), "next_state": ((55,), torch.float32),
        "next_contact": ((2,), torch.bool), "next_on_target": ((2,), torch.bool)}
GROUP = {k: ("contacts" if k.startswith("contact") else "joints" if k.startswith("joint") else "next_state") for k in KEYS}


def test_header_declares_the_entry_point_under_version_4():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name, value in (("SS_FRC_SUBSTEPS", 4), ("SS_FRC_CONTACT", 8), ("SS_FRC_JOINT", 4), ("SS_FRC_STATE", 56), ("SS_ABI_VERSION", 4)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), code), name
    decl = re.search(r"int\s+ss_step_forces\s*\(([^)]*)\)\s*;", code)
    assert decl, "ss_step_forces is not declared"
    args = [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",")]
    assert args == ["ss_env* env", "const int32_t* env_ids", "int32_t m", "const float* act", "float* contacts", "float* joints",
                    "float* next_state", "void* stream"]
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "ss_step_forces" in integration and "step_forces(" in integration


def test_binding_matches_the_declaration():
    lib = _lib.load()
    assert "ss_step_forces" in _lib.SYMBOLS and lib.ss_version() == 4 == _lib.ABI_VERSION
    vp = C.c_void_p
    assert lib.ss_step_forces.argtypes == [vp, vp, C.c_int32, vp, vp, vp, vp, vp]
    assert (_lib.FRC_SUBSTEPS, _lib.FRC_CONTACT, _lib.FRC_JOINT, _lib.FRC_STATE) == (4, 8, 4, 56)
    assert lib.ss_step_forces(None, None, 0, None, None, None, None, None) == -1         # a null handle is refused before anything else


class FakeBackend:
    """HipBackend's call surface as far as step_forces() goes; every output word = its flat index, the slot word = (index % 4) - 1, the
    flags word = row + 5"""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def close(self):
        pass

    def set_auto_reset(self, on):
        pass

    def step_forces(self, env_ids, m, act, contacts, joints, next_state):
        assert act.dtype == torch.float32 and act.is_contiguous() and tuple(act.shape) == (m, 21)
        self.calls.append((None if env_ids is None else env_ids.clone(), m, act.clone(), contacts is not None, joints is not None,
                           next_state is not None))
        for t in (contacts, joints, next_state):
            if t is not None:
                assert t.dtype == torch.float32 and t.is_contiguous() and t.shape[0] == m
                t.copy_(torch.arange(t.numel(), dtype=torch.float32).reshape(t.shape))
        if contacts is not None:
            assert tuple(contacts.shape[1:]) == (4, 8, 8)
            contacts[..., 0] = (torch.arange(m * 32).reshape(m, 4, 8) % 4 - 1).float()
        if joints is not None:
            assert tuple(joints.shape[1:]) == (4, 4, 21)
        if next_state is not None:
            assert tuple(next_state.shape[1:]) == (56,)
            next_state[:, 55] = torch.arange(m).float() + 5


@pytest.mark.parametrize("numpy_mode", [False, True])
def test_vecenv_returns_the_documented_dict(numpy_mode):
    be = FakeBackend()
    env = SteppingStoneVecEnv("Walker3DStepperEnv-v0", 5, backend=be, return_numpy=numpy_mode)
    act = np.linspace(-2, 2, 105, dtype=np.float32).reshape(5, 21)
    out = env.step_forces(act if numpy_mode else torch.from_numpy(act))
    assert set(out) == set(KEYS)
    for k, (shape, dtype) in KEYS.items():
        v = out[k]
        if numpy_mode:
            assert isinstance(v, np.ndarray) and v.dtype == {torch.int32: np.int32, torch.bool: np.bool_, torch.float32: np.float32}[dtype]
        else:
            assert torch.is_tensor(v) and v.dtype == dtype
        assert tuple(v.shape) == (5,) + shape, k
    ids, m, got_act, *asked = be.calls[-1]
    assert ids is None and m == 5 and asked == [True, True, True] and (got_act.numpy() == act).all()      # unclipped: the kernel clips
    as_np = lambda v: v if numpy_mode else v.numpy()
    co = np.arange(5 * 4 * 8 * 8, dtype=np.float32).reshape(5, 4, 8, 8)
    jo = np.arange(5 * 4 * 4 * 21, dtype=np.float32).reshape(5, 4, 4, 21)
    ns = np.arange(5 * 56, dtype=np.float32).reshape(5, 56)
    assert (as_np(out["contact_slot"]) == (np.arange(160).reshape(5, 4, 8) % 4 - 1)).all()
    assert (as_np(out["contact_pen"]) == co[..., 1]).all() and (as_np(out["contact_force"]) == co[..., 2:5]).all()
    assert (as_np(out["contact_force_world"]) == co[..., 5:8]).all()
    for r, k in enumerate(("joint_q", "joint_qd", "joint_tau", "joint_torque")):
        assert (as_np(out[k]) == jo[:, :, r]).all(), k
    assert (as_np(out["next_state"]) == ns[:, :55]).all()
    flags = np.arange(5) + 5
    assert (as_np(out["next_contact"]) == np.stack([flags & 1, (flags >> 1) & 1], 1).astype(bool)).all()
    assert (as_np(out["next_on_target"]) == np.stack([(flags >> 2) & 1, (flags >> 3) & 1], 1).astype(bool)).all()


def test_vecenv_passes_env_ids_actions_and_the_requested_groups_through():
    be = FakeBackend()
    env = SteppingStoneVecEnv("MikeStepperEnv-v0", 6, backend=be)
    act = torch.arange(63, dtype=torch.float32).reshape(3, 21)
    out = env.step_forces(act, env_ids=[4, 0, 3], contacts=False, next_state=False)
    ids, m, got_act, *asked = be.calls[-1]
    assert ids.dtype == torch.int32 and ids.tolist() == [4, 0, 3] and m == 3 and asked == [False, True, False] and torch.equal(got_act, act)
    assert set(out) == {k for k in KEYS if GROUP[k] == "joints"} and out["joint_torque"].shape == (3, 4, 21)
    mask = torch.tensor([0, 1, 0, 0, 1, 1], dtype=torch.bool)
    out = env.step_forces(act, env_ids=mask, joints=False)
    assert be.calls[-1][0].tolist() == [1, 4, 5] and set(out) == {k for k in KEYS if GROUP[k] != "joints"}
    n = len(be.calls)
    assert env.step_forces(torch.zeros((0, 21)), env_ids=[])["contact_force"].shape == (0, 4, 8, 3) and len(be.calls) == n      # m == 0
    for bad in ([6], [-1], [1, 1]):
        with pytest.raises(ValueError):
            env.step_forces(act[:len(bad)], env_ids=bad)
    with pytest.raises(ValueError):
        env.step_forces(act, env_ids=[1, 2])                       # two envs, three action rows
    with pytest.raises(ValueError):
        env.step_forces(act)                                       # all six envs, three action rows
    with pytest.raises(ValueError):
        env.step_forces(torch.zeros((6, 21)), contacts=False, joints=False, next_state=False)


def test_single_env_facade_drops_the_env_axis():
    env = SteppingStoneEnv("Walker3DStepperEnv-v0", backend_factory=lambda kind, n, seed: FakeBackend())
    out = env.step_forces(np.zeros(21))
    assert set(out) == set(KEYS) and all(tuple(out[k].shape) == shape for k, (shape, _) in KEYS.items())


class Backend(OracleBackend):
    """the CPU oracle plus kinematics() / step_forces() served by the CPU builds of the readouts, and a blank render()"""
    def __init__(self, kind, n, seed):
        super().__init__(kind, n, seed)
        self.kind, self.seen = kind, []

    def render(self, env_ids, width, height, camera, rgb, depth, seg):
        rgb.zero_()

    def kinematics(self, env_ids, m, body_twist, summary, corners):
        out = kh.kinematics(nk.KINDS.index(self.kind), self.o.get_state().astype(np.float32), twists=False)
        summary.copy_(torch.from_numpy(out["summary"]))
        corners.copy_(torch.from_numpy(out["corners"]))

    def step_forces(self, env_ids, m, act, contacts, joints, next_state):
        assert env_ids is None and m == self.n and next_state is None
        st = self.o.get_state().astype(np.float32)
        self.seen.append((st, act.numpy().copy()))
        out = fh.step_forces(nk.KINDS.index(self.kind), st, act.numpy(), next_state=False)
        contacts.copy_(torch.from_numpy(out["contacts"]))
        joints.copy_(torch.from_numpy(out["joints"]))


@pytest.mark.skipif(not native_build.hipcc(), reason="needs hipcc")
def test_enjoy_trace_with_forces(tmp_path, monkeypatch):
    made = []

    def make(env_id, envs, seed=0, device=None, return_numpy=False):
        be = Backend("walker3d", envs, seed)
        made.append(be)
        return SteppingStoneVecEnv(env_id, envs, seed=seed, return_numpy=return_numpy, backend=be)
    monkeypatch.setattr(enjoy, "SteppingStoneVecEnv", make)
    torch.manual_seed(0)
    net = tmp_path / "policy.pt"
    torch.save(ppo.ActorCritic().state_dict(), net)
    T, K = 6, 2
    argv = ["--env", "Walker3DStepperEnv-v0", "--net", str(net), "--envs", str(K), "--steps", str(T), "--size", "16x16", "--device", "cpu",
            "--out", str(tmp_path / "walk.npy")]
    with pytest.raises(SystemExit):
        enjoy.main(argv + ["--forces"])                                   # only together with --trace
    assert enjoy.main(argv + ["--trace", str(tmp_path / "walk"), "--forces"]) == 0
    tr = np.load(tmp_path / "walk.npz")
    shapes = {"com": (T, K, 3), "com_vel": (T, K, 3), "corner_height": (T, K, 8), "corner_carrier": (T, K, 8), "contact": (T, K, 2),
              "next_step_index": (T, K), "done": (T, K), "contact_force": (T, K, 4, 8, 8), "joint_torque": (T, K, 4, 21)}
    assert set(tr.files) == set(shapes)
    for k, s in shapes.items():
        assert tr[k].shape == s, k
    assert tr["contact_force"].dtype == np.float32 and tr["joint_torque"].dtype == np.float32
    be = made[-1]
    assert len(be.seen) == T
    for t, (st, act) in enumerate(be.seen):                               # the readout of the state step t STARTED in, under its action
        want = fh.step_forces(0, st, act, next_state=False)
        assert (tr["contact_force"][t] == want["contacts"]).all() and (tr["joint_torque"][t] == want["joints"][:, :, 3]).all()
    assert (tr["contact_force"][..., 2] > 0).any()                        # it stood on a stone
    # the state of step t + 1's dry run is the state step t ended in: the readout ran BEFORE env.step
    assert (be.seen[1][0][:, 61] == be.seen[0][0][:, 61] + 1).all()
