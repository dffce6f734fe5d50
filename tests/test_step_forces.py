"""The force readout on the CPU: steppingstone_amd/csrc/ss_forces.hpp compiled for the host (tests/host/forces_host.cpp, lane threads and
the pair exchange of the host harness) on the case set of tests/forces_cases.py.
  * the fp32 oracle agrees with the fp64 oracle on every carried set of the case set (the yardstick leaves nothing out);
  * next_state is, bit for bit, the state hh_step (the host build of step_env) leaves, and the readout changes nothing;
  * cone, zeros and world vector (exact / counted), forces against the fp64 oracle, joint torques against PHYSICS.md 3.1 in fp64."""
import numpy as np
import pytest

import forces_cases as fc
import forces_host_lib as fh
import host_lib
import native_build

pytestmark = pytest.mark.skipif(not native_build.hipcc(), reason="needs hipcc")


@pytest.fixture(scope="module", params=fc.KINDS)
def scene(request):
    kind = request.param
    c = fc.cases(kind)
    out = fh.step_forces(fc.KINDS.index(kind), c["st"], c["act"], state_after=True)
    return kind, c, out


def test_oracle_yardstick_leaves_nothing_out(scene):
    kind, c, out = scene
    y = fc.yardstick(kind)
    print("fp32 oracle against fp64 oracle %s: left out %d, force distance %.3g (%.3g N of %.4g N), pen distance %.3g m" %
          (kind, y["left_out"], y["force"], y["force_abs"], y["fmax"], y["pen"]))
    assert y["left_out"] == 0 and y["force"] > 0 and y["pen"] > 0
    assert y["ref"]["on"].any(2).mean() > 0.5, "most (env, substep) pairs of the case set are in contact"


def test_next_state_is_the_host_step_bit_for_bit_and_nothing_is_written(scene):
    kind, c, out = scene
    assert (out["state"].view(np.int32) == c["st"].view(np.int32)).all(), "the readout changed the state"
    after, _, _, done, _ = host_lib.step(fc.KINDS.index(kind), c["st"], c["act"], seed=5, curriculum=5)
    keep = done == 0              # hh_step resets a finished env in place (auto-reset is on in the harness): its row is the fresh episode's
    assert keep.sum() >= fc.N_ENVS // 2, "most envs of the case set go on"
    ns = out["next_state"]
    assert (ns[keep, :55].view(np.int32) == after[keep, :55].view(np.int32)).all()
    assert ((ns[keep, 55].astype(np.int64) & 3) == after[keep, 64].astype(np.int64)).all()
    j = out["joints"]
    assert (j[:, 0, 0].view(np.int32) == c["st"][:, 13:34].view(np.int32)).all() and (j[:, 0, 1].view(np.int32) == c["st"][:, 34:55].view(np.int32)).all()
    assert np.isfinite(out["contacts"]).all() and np.isfinite(j).all() and np.isfinite(ns).all()


def test_rows_do_not_depend_on_the_request(scene):
    kind, c, out = scene
    ids = [5, 63, 5, 0, 64, -1, 17]                 # a repeated id; 64 and -1 name no env of the 64
    act = c["act"][[i if 0 <= i < 64 else 0 for i in ids]]
    rows = [r for r, i in enumerate(ids) if 0 <= i < 64]
    sub = fh.step_forces(fc.KINDS.index(kind), c["st"], act, env_ids=ids)
    for k in ("contacts", "joints", "next_state"):
        for r, i in enumerate(ids):
            if 0 <= i < 64:
                assert (sub[k][r].view(np.int32) == out[k][i].view(np.int32)).all(), (k, r, i)
            else:
                assert (sub[k][r] == 0).all(), "row %d (id %d) of %s was written" % (r, i, k)
        one = fh.step_forces(fc.KINDS.index(kind), c["st"], act, env_ids=ids, contacts=k == "contacts", joints=k == "joints",
                             next_state=k == "next_state")
        assert set(one) == {k}
        assert (one[k][rows].view(np.int32) == sub[k][rows].view(np.int32)).all(), "%s differs when asked for alone" % k


def test_cone_zeros_and_world_vector(scene):
    kind, c, out = scene
    fc.judge_cone_and_zeros(kind, out["contacts"], c["st"], "host")
    assert (fc.judge_flags(out["contacts"], out["next_state"]) & 3).any()


@pytest.mark.parametrize("kind", fc.KINDS)
def test_tilted_stones(kind):
    c = fc.tilted_cases(kind)
    out = fh.step_forces(fc.KINDS.index(kind), c["st"], c["act"])
    g = fc.split(out["contacts"])
    assert g["on"].sum() >= 64, "carried corner rows on the tilted stones: %d" % g["on"].sum()
    fc.judge_cone_and_zeros(kind, out["contacts"], c["st"], "host, tilted stones")
    fc.judge_flags(out["contacts"], out["next_state"])
    fc.judge_joint_torques(kind, out["joints"], out["next_state"], c["act"], "host, tilted stones")


def test_forces_against_the_fp64_oracle(scene):
    kind, c, out = scene
    fc.judge_against_oracle(kind, out["contacts"], "host")


def test_joint_torques(scene):
    kind, c, out = scene
    fc.judge_joint_torques(kind, out["joints"], out["next_state"], c["act"], "host")
