"""create_temp_states and get_obs on the GPU (docs/PHYSICS.md 5 and 8; temp_states_kernel, obs_kernel) beyond a fresh episode: both robots,
N = 76 envs (more than a wavefront, not a multiple of 64) holding tests/temp_states_cases.py's rows -- every n in 1..19, headings past
+-pi/2, yaw over the whole circle -- against the fp64 reference with the counted K of that module;
  * ss_create_temp_states itself on a pre-filled buffer with a canary tail: every word written, none behind, a misaligned buffer refused,
    the state left as it was;
  * a row's bits do not depend on its position or on the instance size;
  * native states, no set_state before the readout: 64 envs at curriculum 5 after 300 steps under the shipped actor -- turned paths, and
    second episodes whose terrain table still holds the previous episode's stones -- against the reference of the GPU's own get_state()
    rows; a second instance given those rows returns the same bits (stored and provisional stones agree)."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_lib as ol
import shipped_actor as sa
import temp_states_cases as tsc

pytestmark = pytest.mark.gpu
ENVS = {"walker3d": "Walker3DStepperEnv-v0", "mike": "MikeStepperEnv-v0"}
N = tsc.N_CASES
WORDS = tsc.NCELL * tsc.OBS
FILL = 0x5A5A5A5A
TAIL = 64                       # canary words behind the buffer


def _env(kind, n, seed=3, cur=5):
    from steppingstone_amd.envs import SteppingStoneVecEnv
    e = SteppingStoneVecEnv(ENVS[kind], n, seed=seed, device="cuda:0", return_numpy=False)
    e.update_curriculum(cur)
    e.reset()
    return e


def _call(e, fill=FILL, offset=0):
    """ss_create_temp_states itself on a buffer pre-filled with `fill` and a canary tail: -> (rc, int32 bit patterns [n * 7260 + TAIL]);
    offset: bytes added to the pointer"""
    from steppingstone_amd.envs import _stream
    n = e.num_envs
    buf = torch.full((n * WORDS + TAIL + 4,), fill, dtype=torch.int32, device="cuda:0")
    rc = e.backend.lib.ss_create_temp_states(e.backend.h, C.c_void_p(buf.data_ptr() + offset), _stream(e.device))
    torch.cuda.synchronize()
    return rc, buf.cpu().numpy()[:n * WORDS + TAIL]


def _temp(e, fill=FILL):
    """-> int32 bit patterns [n, 121, 60]; the tail checked"""
    rc, buf = _call(e, fill)
    n = e.num_envs
    assert rc == 0
    assert (buf[n * WORDS:] == np.int32(fill)).all(), "the words behind the buffer were written"
    return buf[:n * WORDS].reshape(n, tsc.NCELL, tsc.OBS)


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


@pytest.fixture(scope="module", params=tsc.KINDS)
def scene(request):
    """(kind, env holding cases(kind), its temp states and its get_obs as bit patterns)"""
    kind = request.param
    e = _env(kind, N)
    e.set_state(torch.from_numpy(tsc.cases(kind).copy()))
    temp = _temp(e)
    obs = _bits(e.get_obs().clone())
    yield kind, e, temp, obs
    e.close()


def test_injected_cases_match_the_reference(scene):
    kind, e, temp, obs = scene
    R = tsc.references(kind)
    assert np.array_equal(_bits(e.get_state()), tsc.cases(kind).view(np.int32)), "the env does not hold the rows as they are"
    tsc.judge(obs.view(np.float32), R["obs"], R["obs_tol"], "get_obs device %s" % kind)
    tsc.judge(temp.view(np.float32), R["temp"], R["temp_tol"], "create_temp_states device %s" % kind)
    assert (temp[:, :, :55] == obs[:, None, :55]).all(), "columns 0..54 of every row are the env's get_obs row, bit for bit"
    last = tsc.cases(kind)[:, ol.S_N] == 19
    assert last.sum() >= 4 and (temp[last] == obs[last][:, None, :]).all(), "at n == 19 nothing is re-placed"
    assert torch.equal(e.create_temp_states().view(torch.int32).cpu(), torch.from_numpy(temp.copy())), "the Python surface returns the same words"


def test_every_word_is_written_and_none_behind(scene):
    kind, e, temp, obs = scene
    before = _bits(e.get_state())
    assert np.array_equal(_temp(e, fill=0), temp), "the result depends on what the buffer held"
    rc, buf = _call(e, offset=4)
    assert rc == -1 and b"aligned" in e.backend.lib.ss_last_error()             # SS_ERR_INVALID, nothing launched
    assert (buf == np.int32(FILL)).all()
    assert e.backend.lib.ss_create_temp_states(e.backend.h, None, None) == -1
    assert np.array_equal(_temp(e), temp)
    assert np.array_equal(_bits(e.get_state()), before), "the call changed the state"


def test_rows_do_not_depend_on_position_or_instance_size(scene):
    kind, e, temp, obs = scene
    rows = tsc.cases(kind)
    for r in (30, 75):                                            # n = 8: re-placed; n = 19: not
        batch = rows.copy()
        where = [0, 63, 64, 75]
        batch[where] = rows[r]
        for n2, src, pos in ((N, batch, where), (1, rows[r:r + 1], [0])):
            e2 = _env(kind, n2, seed=11, cur=0)
            e2.set_state(torch.from_numpy(src.copy()))
            got = _temp(e2)
            got_obs = _bits(e2.get_obs().clone())
            e2.close()
            for p in pos:
                assert np.array_equal(got[p], temp[r]) and np.array_equal(got_obs[p], obs[r]), "row %d at position %d of %d envs" % (r, p, n2)
            if n2 == N:
                rest = [i for i in range(N) if i not in where]
                assert np.array_equal(got[rest], temp[rest])


@pytest.mark.parametrize("kind", tsc.KINDS)
def test_native_states_match_the_reference(kind):
    """no set_state before the readout: I_PROV and the terrain table are what the step kernel left"""
    n, steps = 64, 300
    e = _env(kind, n, seed=31)
    actor = sa.load_actor(kind, "cuda:0")
    obs = e.reset()
    episodes = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    for t in range(steps):
        with torch.no_grad():
            a = actor(obs)
        obs, _, done, _ = e.step(a)
        episodes += done.long()
    later = episodes.cpu().numpy() > 0
    temp = _temp(e)
    obs_bits = _bits(e.get_obs().clone())
    st = e.get_state()
    rows = st.cpu().numpy()
    k, phi, _ = (np.array(x) for x in zip(*(tsc.heading(r) for r in rows)))
    turned, stale, later_on = (k >= 3) & (np.abs(phi) > 0.05), later & (k == 1), later & (k >= 2)
    print("%s native: %d envs with n >= 3 on a turned path, %d in a later episode at n == 1, %d in a later episode at n >= 2; n up to %d"
          % (kind, turned.sum(), stale.sum(), later_on.sum(), k.max()))
    assert turned.sum() >= 8 and stale.sum() >= 8 and later_on.sum() >= 8
    R = tsc.judged(kind, rows)
    tsc.judge(obs_bits.view(np.float32), R["obs"], R["obs_tol"], "get_obs device %s, native" % kind)
    tsc.judge(temp.view(np.float32), R["temp"], R["temp_tol"], "create_temp_states device %s, native" % kind)
    assert (temp[:, :, :55] == obs_bits[:, None, :55]).all()
    twin = _env(kind, n, seed=7, cur=0)
    twin.set_state(st)
    assert np.array_equal(_temp(twin), temp), "stored and provisional stones disagree"
    twin.close()
    e.close()
