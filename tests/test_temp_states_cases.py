"""tests/temp_states_cases.py on the CPU, the reference alone: the fp64 oracle agrees with it on the synthetic rows, the rows cover what
they claim to, and the tolerance tells each plausible slip of temp_states_kernel (a wrong index, slot or sign) from the truth by a
factor of 100.  The kernels are judged on the same rows in tests/test_gpu_temp_states.py."""
import numpy as np
import pytest

import np_env
import oracle_lib as ol
import temp_states_cases as tsc

KINDS = tsc.KINDS
POWER = 100.0


@pytest.mark.parametrize("kind", KINDS)
def test_f64_oracle_agrees_with_the_reference(kind):
    rows = tsc.cases(kind)
    R = tsc.references(kind)
    ref, oref = R["temp"], R["obs"]
    o = ol.OracleEnv(kind, tsc.N_CASES, seed=2, prec="f64")
    o.set_curriculum(5)
    o.reset()
    o.set_state(rows.astype(np.float64))
    assert np.array_equal(o.get_state(), rows.astype(np.float64)), "the oracle does not hold the rows as they are"
    tmp, obs = o.create_temp_states(), o.get_obs()
    clipped = float((np.abs(oref[:, :50]) == 5.0).mean())
    w_tmp, w_obs = np.abs(tmp - ref).max(), np.abs(obs - oref).max()
    print("%s: f64 oracle against the reference on %d rows: create_temp_states %.1e, get_obs %.1e; %.1f %% of obs[:50] clipped"
          % (kind, rows.shape[0], w_tmp, w_obs, 100 * clipped))
    last = rows[:, ol.S_N] == 19
    assert np.array_equal(obs[~last, :55], tmp[~last, 60, :55]) and np.array_equal(obs[last], tmp[last, 7])
    assert w_tmp < 1e-6 and w_obs < 1e-6                      # the oracle returns float32 from its fp64 evaluation
    assert clipped > 0.02


@pytest.mark.parametrize("kind", KINDS)
def test_reference_is_np_env_observation_of_the_moved_stone(kind):
    """reference() against the whole observation of a state whose terrain row n + 1 holds the re-placed stone, on a few cells of every row"""
    import np_terrain as npt
    m = tsc.model(kind)
    ref = tsc.references(kind)["temp"]
    for e, row in enumerate(tsc.cases(kind)):
        st = row.astype(np.float64)
        n, flags = int(st[ol.S_N]), int(st[ol.S_FLAGS])
        terrain = st[ol.S_TERRAIN].reshape(20, 6)
        for i, j in ((0, 0), (3, 9), (10, 2), (e % 11, (e // 11) % 11)):
            s2 = st.copy()
            if n <= 18:
                phi, pitch, dr = terrain[n][3] + npt.YAW[i], npt.PITCH[j], st[ol.S_NNDR]
                s2[ol.S_TERRAIN].reshape(20, 6)[n + 1][:3] = terrain[n][:3] + dr * np.array(
                    [np.cos(pitch) * np.cos(phi), np.cos(pitch) * np.sin(phi), np.sin(pitch)])
            assert np.abs(ref[e, i * 11 + j] - np_env.observation(m, s2, flags, n)).max() < 1e-13


@pytest.mark.parametrize("kind", KINDS)
def test_cases_cover_what_the_kernel_branches_on(kind):
    rows = tsc.cases(kind)
    R = tsc.references(kind)
    ref, tol = R["temp"], R["temp_tol"]
    assert rows.shape == (76, 186) and rows.dtype == np.float32
    n, phi, yaw = (np.array(x) for x in zip(*(tsc.heading(r) for r in rows)))
    assert all((n == k).sum() >= 4 for k in range(1, 20)) and n.min() == 1 and n.max() == 19
    assert ((np.abs(phi) > 1) & (n <= 18)).sum() >= 8
    assert np.abs(phi).max() > np.pi / 2
    assert (np.abs(yaw) > 2).sum() >= 8
    assert all(set(rows[n == k, ol.S_FLAGS].astype(int)) == {0, 1, 2, 3} for k in range(1, 20))
    dr = rows[:, ol.S_NNDR]
    assert dr.min() >= 0.65 and dr.max() <= 1.25
    assert (np.abs(ref[:, 0, 27:48]) == 5.0).any() and np.abs(ref[:, 0, 0]).max() <= 5.0
    assert np.abs(rows[:, 0:3]).max() > 8.0                   # positions of several metres: the tolerance must scale with them
    last = n == 19
    assert (ref[last] == ref[last][:, :1]).all() and (ref[last][:, :, 55:60] == ref[last][:, :, 50:55]).all()
    assert (ref[~last][:, 1:, :55] == ref[~last][:, :1, :55]).all()
    assert (R["obs"][:, :55] == ref[:, 0, :55]).all() and (R["obs_tol"][:, :55] == tol[:, 0, :55]).all()
    assert all(np.isfinite(t).all() and (t >= 0).all() for t in (tol, R["obs_tol"]))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mutation", tsc.MUTATIONS)
def test_tolerance_tells_a_wrong_kernel_from_the_reference(kind, mutation):
    """every restated slip is off by more than 100 x the tolerance in some word of every case with 2 <= n <= 18"""
    rows = tsc.cases(kind)
    R = tsc.references(kind)
    ref, tol = R["temp"], R["temp_tol"]
    weakest = np.inf
    for e, row in enumerate(rows):
        if not 2 <= int(row[ol.S_N]) <= 18:
            continue
        wrong = tsc.reference(kind, row, mutate=mutation)
        r = tsc.ratios(wrong, ref[e], tol[e]).max()
        weakest = min(weakest, r)
        assert r > POWER, "%s: row %d (n = %d) is off by only %.3g x its tolerance" % (mutation, e, int(row[ol.S_N]), r)
    print("%s, %s: the least telling row is off by %.3g x its tolerance" % (kind, mutation, weakest))
