"""`python -m steppingstone_amd.enjoy --trace FILE.npz` on the CPU: enjoy.run drives a real SteppingStoneVecEnv whose backend is the CPU
oracle (tests/oracle_backend.py) plus a kinematics() served by the CPU build of ss_kinematics.hpp and a blank render().  The file must
hold, per control step and env, exactly what the readout says of the state that step ended in, next to the observation's contact flags,
next_step_index and done."""
import numpy as np
import pytest
import torch

import kinematics_host_lib as kh
import np_kinematics as nk
import render_host_lib as rh
from oracle_backend import OracleBackend
from steppingstone_amd import enjoy, ppo
from steppingstone_amd.envs import SteppingStoneVecEnv

pytestmark = pytest.mark.skipif(not rh.hipcc(), reason="needs hipcc")


class Backend(OracleBackend):
    def __init__(self, kind, n, seed):
        super().__init__(kind, n, seed)
        self.kind, self.seen = kind, []

    def render(self, env_ids, width, height, camera, rgb, depth, seg):
        rgb.zero_()

    def kinematics(self, env_ids, m, body_twist, summary, corners):
        assert env_ids is None and m == self.n and body_twist is None
        st = self.o.get_state().astype(np.float32)
        self.seen.append(st)
        out = kh.kinematics(nk.KINDS.index(self.kind), st, twists=False)
        summary.copy_(torch.from_numpy(out["summary"]))
        corners.copy_(torch.from_numpy(out["corners"]))


def test_trace_file_holds_the_readout_of_every_step(tmp_path, monkeypatch):
    made = []

    def make(env_id, envs, seed=0, device=None, return_numpy=False):
        be = Backend("walker3d", envs, seed)
        made.append(be)
        return SteppingStoneVecEnv(env_id, envs, seed=seed, return_numpy=return_numpy, backend=be)
    monkeypatch.setattr(enjoy, "SteppingStoneVecEnv", make)
    torch.manual_seed(0)
    net = tmp_path / "policy.pt"
    torch.save(ppo.ActorCritic().state_dict(), net)
    T, K = 40, 3
    rc = enjoy.main(["--env", "Walker3DStepperEnv-v0", "--net", str(net), "--envs", str(K), "--steps", str(T), "--size", "16x16",
                     "--device", "cpu", "--out", str(tmp_path / "walk.npy"), "--trace", str(tmp_path / "walk")])
    assert rc == 0
    tr = np.load(tmp_path / "walk.npz")
    shapes = {"com": (T, K, 3), "com_vel": (T, K, 3), "corner_height": (T, K, 8), "corner_carrier": (T, K, 8), "contact": (T, K, 2),
              "next_step_index": (T, K), "done": (T, K)}
    assert set(tr.files) == set(shapes)
    for k, s in shapes.items():
        assert tr[k].shape == s, k
    assert tr["corner_carrier"].dtype == np.int32 and tr["contact"].dtype == bool and tr["done"].dtype == bool
    assert tr["com"].dtype == np.float32 and tr["corner_height"].dtype == np.float32
    states = np.stack(made[0].seen)                                  # [T, K, 186]: the state each step ended in
    assert states.shape == (T, K, 186)
    want = nk.split_outputs(kh.kinematics(0, states.reshape(T * K, 186), twists=False))
    for k in ("com", "com_vel", "corner_height", "corner_carrier"):
        assert (tr[k].reshape((T * K,) + tr[k].shape[2:]) == want[k]).all(), k
    assert (tr["next_step_index"] == states[:, :, 59]).all()
    flags = states[:, :, 64].astype(np.int64)
    assert (tr["contact"][:, :, 0] == (flags & 1).astype(bool)).all() and (tr["contact"][:, :, 1] == ((flags >> 1) & 1).astype(bool)).all()
    assert tr["done"].any() and tr["contact"].any()                  # an untrained policy falls within 40 steps; it stood on a stone first
    assert np.load(tmp_path / "walk.npy").shape == (T, 32, 32, 3)       # 3 envs tile 2 x 2
