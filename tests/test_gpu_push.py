"""ss_push on the GPU (docs/PHYSICS.md 12): both robots, N = 70 envs (more than a wavefront, less than two, not a multiple of the 8 rows
of a workgroup or of the 64-env padding), curriculum 5 after 30 random control steps, one drawn push per env (push_cases.draw).
  * the dry run against the fp64 restatement with the K of tests/push_cases.py; the share of words bit-equal to the host build; an applied
    push changes words 7:13 | 34:55 of the listed envs to nu + delta_nu and nothing else;
  * a row's bits do not depend on the instance size, its position, the ids' order, `apply` or delta_nu being asked for;
  * rows of invalid ids or bodies and everything at m == 0 write nothing; bad host arguments answer SS_ERR_INVALID;
  * ss_kinematics before and after an applied push: the momentum changes by the impulse, the pushed point by J delta_nu;
  * a pushed env steps like an injected one; ss_push + ss_step replay from a captured graph like the eager pair."""
import ctypes as C

import numpy as np
import pytest
import torch

import kinematics_cases as kc
import np_dynamics as npd
import np_kinematics as nk
import np_push as npp
import push_cases as pc
import push_host_lib as ph
from steppingstone_amd import model as M

pytestmark = pytest.mark.gpu
ENVS = {"walker3d": "Walker3DStepperEnv-v0", "mike": "MikeStepperEnv-v0"}
N = 70
D = 27
FILL = 0x5A5A5A5A
TAIL = 64                       # canary words behind delta_nu
U = pc.U
NU = list(range(7, 13)) + list(range(34, 55))          # the state words of nu
REST = [i for i in range(186) if i not in NU]


def _env(kind, n, seed=3, steps=30):
    from steppingstone_amd.envs import SteppingStoneVecEnv
    e = SteppingStoneVecEnv(ENVS[kind], n, seed=seed, device="cuda:0", return_numpy=False)
    e.update_curriculum(5)
    e.reset()
    if steps:
        e.rollout_random(steps, t0=0, steps_per_launch=1)
    return e


def _dev(a, dtype):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to("cuda:0")


def _call(e, ids, m, body, point, impulse, apply, want=True):
    """ss_push itself, delta_nu pre-filled with a canary tail: -> (rc, int32 bit pattern [m * 27 + TAIL] or None)"""
    from steppingstone_amd.envs import _ptr, _stream
    buf = torch.full((max(m, 0) * D + TAIL,), FILL, dtype=torch.int32, device="cuda:0") if want else None
    args = [_dev(ids, torch.int32), _dev(body, torch.int32), _dev(point, torch.float32), _dev(impulse, torch.float32)]
    p = [None if a is None else _ptr(a) for a in args]
    rc = e.backend.lib.ss_push(e.backend.h, p[0], m, p[1], p[2], p[3], _ptr(buf) if want else None, apply, _stream(e.device))
    torch.cuda.synchronize()
    return rc, buf.cpu().numpy() if want else None


def _rows(buf, m):
    assert (buf[m * D:] == FILL).all(), "the words behind delta_nu were written"
    return buf[:m * D].reshape(m, D)


def _push(e, ids, rows, c, apply, want=True):
    """pushes c[rows[k]] on env ids[k]: the rows whose point is NULL in one call, the others in a second (the pointer is per call);
    -> delta_nu bits [len(ids), 27] (None unless want)"""
    ids, rows = np.asarray(ids), np.asarray(rows)
    out = np.full((len(ids), D), FILL, np.int32)
    for null in (True, False):
        sel = np.nonzero((c["mode"][rows] == 0) == null)[0]
        if sel.size:
            r = rows[sel]
            rc, buf = _call(e, ids[sel], sel.size, c["body"][r], None if null else c["point"][r], c["impulse"][r], apply, want)
            assert rc == 0
            if want:
                out[sel] = _rows(buf, sel.size)
    return out if want else None


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def _added(st, dnu_bits, rows=None):
    """the packed rows st (float32 array) with delta_nu (bit patterns) added to the words of nu, in fp32"""
    out = np.array(st, np.float32)
    sel = slice(None) if rows is None else rows
    out[sel, 7:13] = out[sel, 7:13] + dnu_bits.view(np.float32)[:, :6]
    out[sel, 34:55] = out[sel, 34:55] + dnu_bits.view(np.float32)[:, 6:]
    return out


@pytest.fixture(scope="module", params=pc.KINDS)
def scene(request):
    """(kind, env, packed rows [70,186] as numpy, the drawn pushes, the dry run's delta_nu of all rows as bit patterns): the env holds
    the rows through set_state, as every instance they are compared with does"""
    kind = request.param
    e = _env(kind, N)
    st = e.get_state().clone()
    e.set_state(st)
    c = pc.draw(N, 40 + pc.KINDS.index(kind), zeros=8)
    pc.check_counts(c, per_body=3, zeros=8)
    full = _push(e, np.arange(N), np.arange(N), c, 0)
    assert torch.equal(e.get_state().view(torch.int32), st.view(torch.int32)), "a dry run changes nothing"
    yield kind, e, st.cpu().numpy(), c, full
    e.close()


def test_dry_run_matches_the_restatement_and_apply_adds_it(scene):
    kind, e, st, c, full = scene
    assert not (full == FILL).any(), "a word of a valid row was not written"
    dnu = full.view(np.float32)
    refs = pc.references(kind, st, c)
    om = pc.omegas(refs, dnu)
    print("push device %s: worst omega %.4g x 2^-24 (median %.3g; K %.4g)" % (kind, om.max(), np.median(om), pc.K))
    assert (om <= pc.K).all(), "%s: rows over K: %s" % (kind, {int(i): float(om[i]) for i in np.nonzero(~(om <= pc.K))[0]})
    zero = ~(c["impulse"] != 0).any(axis=1)
    assert zero.sum() >= 8 and (dnu[zero] == 0).all()
    host = ph.push_modes(pc.KINDS.index(kind), st, c["body"], c["mode"], c["point"], c["impulse"])
    print("push device-vs-host %s: share of bit-equal words %.3f" % (kind, float((host.view(np.int32) == full).mean())))
    # an applied push on some of the envs
    listed = np.array([i for i in range(N) if i % 5])
    e2 = _env(kind, N, seed=11, steps=0)
    e2.set_state(torch.from_numpy(st).to("cuda:0"))
    got = _push(e2, listed, listed, c, 1)
    assert (got == full[listed]).all(), "delta_nu does not depend on apply"
    after = _bits(e2.get_state())
    want = _added(st, full[listed], listed).view(np.int32)
    assert (after[:, NU] == want[:, NU]).all(), "words 7:13 | 34:55 of the listed envs become nu + delta_nu"
    assert (after[:, REST] == st.view(np.int32)[:, REST]).all(), "no other word changes"
    assert (after[::5] == st.view(np.int32)[::5]).all(), "no other env changes"
    e2.close()
    # the Python surface returns the same words
    rows = [r for r in range(N) if c["mode"][r] != 0][:9]
    d = e.push(c["impulse"][rows], env_ids=rows, body=[M.BODY_NAMES[b] for b in c["body"][rows]], point=c["point"][rows], apply=False)
    assert (_bits(d) == full[rows]).all()


def test_rows_do_not_depend_on_batch_position_apply_or_requested_output(scene):
    kind, e, st, c, full = scene
    rng = np.random.default_rng(5)
    layouts = [(1, [37], [0]), (1, [69], [0]), (64, list(range(69, 5, -1)), list(range(64))), (130, list(range(N)), list(range(60, 130)))]
    for n2, src, pos in layouts:
        e2 = _env(kind, n2, seed=11, steps=0)
        inject = lambda: e2.set_state(torch.from_numpy(st[src]).to("cuda:0"), env_ids=pos)
        inject()
        order = rng.permutation(len(pos))
        ids, want = np.asarray(pos)[order], np.asarray(src)[order]
        assert (_push(e2, ids, want, c, 0) == full[want]).all(), "a dry run differs in a %d-env instance" % n2
        assert (_push(e2, ids, want, c, 1) == full[want]).all(), "an applied push differs in a %d-env instance" % n2
        state = _bits(e2.get_state(env_ids=ids.tolist()))
        assert (state == _added(st[want], full[want]).view(np.int32)).all()
        inject()
        _push(e2, ids, want, c, 1, want=False)
        assert (_bits(e2.get_state(env_ids=ids.tolist())) == state).all(), "the state differs when delta_nu is not asked for"
        e2.close()


def test_rows_of_invalid_ids_or_bodies_and_everything_at_m_0_stay_untouched(scene):
    kind, e, st, c, full = scene
    e2 = _env(kind, N, seed=11, steps=0)
    e2.set_state(torch.from_numpy(st).to("cuda:0"))
    ids = [3, -1, 64, N, 69, -1, N + 1000, 0]
    body = [0, 5, 22, 1, 7, 3, 2, -1]
    good = [0, 4]
    w = np.tile(np.array([1.0, -2.0, 3.0, 0.5, 0.25, -1.0], np.float32), (len(ids), 1))
    pt = np.tile(np.array([0.1, 0.0, -0.1], np.float32), (len(ids), 1))
    rc, buf = _call(e2, ids, len(ids), body, pt, w, 1)
    assert rc == 0
    rows = _rows(buf, len(ids))
    for r in range(len(ids)):
        assert (rows[r] == FILL).all() == (r not in good), "row %d (id %d, body %d)" % (r, ids[r], body[r])
    after = _bits(e2.get_state())
    want = _added(st, rows[good], [ids[r] for r in good]).view(np.int32)
    assert (after == want).all(), "only the envs of the valid rows change"
    for null_ids in (False, True):
        rc, buf = _call(e2, None if null_ids else [], 0, None if null_ids else [], None, w[:0], 1)
        assert rc == 0 and (buf == FILL).all()
    assert (_bits(e2.get_state()) == after).all()
    e2.close()


def test_bad_arguments_are_refused(scene):
    from steppingstone_amd.envs import _ptr, _stream
    kind, e, st, c, full = scene
    lib, h, s = e.backend.lib, e.backend.h, _stream(e.device)
    ids = torch.arange(4, dtype=torch.int32, device="cuda:0")
    w = torch.ones((N, 6), device="cuda:0")
    buf = torch.full((N * D + TAIL,), FILL, dtype=torch.int32, device="cuda:0")
    p = _ptr(buf)
    off = C.c_void_p(buf.data_ptr() + 4)
    assert lib.ss_push(h, _ptr(ids), 4, None, None, None, p, 1, s) == -1                # NULL impulse
    assert lib.ss_push(h, _ptr(ids), 4, None, None, _ptr(w), None, 0, s) == -1          # a dry run without delta_nu
    assert lib.ss_push(h, _ptr(ids), 4, None, None, _ptr(w), off, 1, s) == -1           # a misaligned delta_nu
    assert lib.ss_push(h, None, 4, None, None, _ptr(w), p, 1, s) == -1                  # NULL ids with m != N
    assert lib.ss_push(h, None, N + 1, None, None, _ptr(w), p, 1, s) == -1
    assert lib.ss_push(h, _ptr(ids), -1, None, None, _ptr(w), p, 1, s) == -1            # m < 0
    assert b"ss_push" in lib.ss_last_error()
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == FILL).all(), "nothing was launched"
    assert (_bits(e.get_state()) == st.view(np.int32)).all()


def test_momentum_and_point_velocity_through_the_kinematic_readout(scene):
    """ss_kinematics before and after an applied push of every env.  M_total d(com_vel) against p and d(ang_mom) against (x - com) x p +
    L, within both readouts' K 2^-24 B (kinematics_cases.K) plus test 1's bound for the six base rows, turned into the world and moved
    to the centre of mass as in tests/test_push.py.  The pushed point's world velocity change, from body_twist, against J times the
    change of nu the state shows."""
    kind, e, st, c, full = scene
    m = pc.model(kind)
    tot = float(m["mass"].sum())
    e2 = _env(kind, N, seed=11, steps=0)
    e2.set_state(torch.from_numpy(st).to("cuda:0"))
    np_ = lambda d: {k: v.cpu().numpy().astype(np.float64) for k, v in d.items()}
    k0 = np_(e2.kinematics(corners=False))
    dnu = _push(e2, np.arange(N), np.arange(N), c, 1).view(np.float32)
    k1 = np_(e2.kinematics(corners=False))
    st1 = e2.get_state().cpu().numpy()
    e2.close()
    refs = pc.references(kind, st, c)
    kK = kc.K
    worst = [0.0, 0.0, 0.0]
    for i in range(N):
        r0, r1 = nk.readout(m, st[i]), nk.readout(m, st1[i])
        s = st[i].astype(np.float64)
        R0 = npd.quat_rot(s[3:7])
        R, p = M.fk(m, s[13:34], s[0:3], R0)
        b = int(c["body"][i])
        d = R[b] @ npp.point_of(m, b, pc.point_arg(c, i))
        com = r0["com"][0]
        w = refs[i]["w"]
        tol = pc.K * U * npp.residual(refs[i], dnu[i])[1][:6]
        tol_p = np.abs(R0) @ tol[3:6]
        ac = np.abs(com - s[0:3])
        tol_l = np.abs(R0) @ tol[0:3] + np.array([ac[1] * tol_p[2] + ac[2] * tol_p[1], ac[2] * tol_p[0] + ac[0] * tol_p[2],
                                                  ac[0] * tol_p[1] + ac[1] * tol_p[0]])
        tol_p = tol_p + tot * kK["com_vel"] * U * (r0["com_vel"][1] + r1["com_vel"][1])
        tol_l = tol_l + kK["ang_mom"] * U * (r0["ang_mom"][1] + r1["ang_mom"][1])
        dp = tot * (k1["com_vel"][i] - k0["com_vel"][i]) - w[:3]
        dl = (k1["ang_mom"][i] - k0["ang_mom"][i]) - (np.cross(p[b] + d - com, w[:3]) + w[3:])
        worst[0] = max(worst[0], float((np.abs(dp) / tol_p).max()))
        worst[1] = max(worst[1], float((np.abs(dl) / tol_l).max()))
        assert (np.abs(dp) <= tol_p).all(), "%s env %d: linear momentum off by %s (tolerance %s)" % (kind, i, dp, tol_p)
        assert (np.abs(dl) <= tol_l).all(), "%s env %d: angular momentum off by %s (tolerance %s)" % (kind, i, dl, tol_l)
        # the pushed point: v + w x d from body_twist, before and after, against J (nu_after - nu_before)
        tw0, tw1 = k0["body_twist"][i, b], k1["body_twist"][i, b]
        B0, B1 = r0["body_twist"][1][b], r1["body_twist"][1][b]
        ad = np.abs(d)
        cross_abs = lambda a: np.array([a[1] * ad[2] + a[2] * ad[1], a[2] * ad[0] + a[0] * ad[2], a[0] * ad[1] + a[1] * ad[0]])
        dv = (tw1[3:] + np.cross(tw1[:3], d)) - (tw0[3:] + np.cross(tw0[:3], d))
        applied = np.concatenate([st1[i, 7:13], st1[i, 34:55]]).astype(np.float64) - np.concatenate([s[7:13], s[34:55]])
        tol_v = kK["body_twist"] * U * (B0[3:] + B1[3:] + cross_abs(B0[:3] + B1[:3]))
        err = dv - refs[i]["J"][:3] @ applied
        worst[2] = max(worst[2], float((np.abs(err) / tol_v).max()))
        assert (np.abs(err) <= tol_v).all(), "%s env %d: the pushed point's velocity change is off by %s (tolerance %s)" % (kind, i, err, tol_v)
    print("push device %s: through ss_kinematics, worst |error| / tolerance: linear momentum %.3g, angular momentum %.3g, point velocity "
          "%.3g" % (kind, *worst))


@pytest.mark.parametrize("kind", pc.KINDS)
def test_a_pushed_env_steps_like_an_injected_one_eagerly_and_from_a_graph(kind):
    """push(apply) then step(act) on one instance against set_state(rows with nu + delta_nu) then step(act) on a second: obs, rew, done
    and state bit for bit.  Then ss_push + ss_step captured into one graph and replayed once on the first instance, from the same
    start, against that eager pair."""
    a, b = _env(kind, N), _env(kind, N)
    st = a.get_state().clone()
    c = pc.draw(N, 50 + pc.KINDS.index(kind), zeros=8)
    w = torch.from_numpy(c["impulse"]).to("cuda:0")
    body = torch.from_numpy(c["body"]).to("cuda:0")
    pt = torch.from_numpy(c["point"]).to("cuda:0")
    dnu = torch.zeros((N, D), device="cuda:0")
    act = (torch.rand((N, 21), generator=torch.Generator().manual_seed(9)) * 2 - 1).to("cuda:0")
    a.backend.push(None, N, body, pt, w, dnu, True)
    pushed = a.get_state().clone()
    assert not torch.equal(pushed, st)
    rows = torch.from_numpy(_added(st.cpu().numpy(), _bits(dnu))).to("cuda:0")
    assert torch.equal(rows.view(torch.int32), pushed.view(torch.int32))
    b.set_state(rows)
    outs = []
    for e in (a, b):
        obs, rew, done, _ = e.step(act)
        outs.append((obs.clone(), rew.clone(), done.clone(), e.get_state().clone()))
    same = lambda x, y: torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
    for x, y in zip(*outs):
        assert same(x, y)
    b.close()
    # the captured pair
    obs, rew = torch.zeros((N, 60), device="cuda:0"), torch.zeros(N, device="cuda:0")
    done, info = torch.zeros(N, dtype=torch.uint8, device="cuda:0"), torch.zeros((N, 6), dtype=torch.int32, device="cuda:0")
    dnu2 = torch.zeros((N, D), device="cuda:0")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                     # (warm-up outside the capture, as torch asks for)
        a.backend.push(None, N, body, pt, w, dnu2, False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    a.set_state(st)
    with torch.cuda.graph(g):
        a.backend.push(None, N, body, pt, w, dnu2, True)
        a.backend.step(act, obs, rew, done, info)
    a.set_state(st)
    dnu2.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert same(dnu2, dnu)
    for x, y in zip((obs, rew, done.to(outs[0][2].dtype), a.get_state()), outs[0]):
        assert same(x, y)
    a.close()


def test_enjoy_push_on_the_device(tmp_path):
    """--push over the HIP backend: the walk is the unpushed one up to the push and another one after it; the trace records the push"""
    from steppingstone_amd import enjoy, ppo
    torch.manual_seed(0)
    net = tmp_path / "policy.pt"
    torch.save(ppo.ActorCritic().state_dict(), net)
    tr = []
    for name, pushes in (("a", []), ("b", ["3:torso:0,30,0"])):
        enjoy.run("Walker3DStepperEnv-v0", str(net), envs=2, steps=6, size=(32, 32), trace=str(tmp_path / (name + ".npz")),
                  log=lambda *a: None, pushes=pushes)
        tr.append(np.load(tmp_path / (name + ".npz")))
    plain, pushed = tr
    assert "push_step" not in plain.files
    assert pushed["push_step"].tolist() == [3] and pushed["push_body"].tolist() == [0] and pushed["push_impulse"].tolist() == [[0.0, 30.0, 0.0]]
    d = pushed["push_delta_nu"]
    assert d.shape == (1, 2, 27) and np.isfinite(d).all() and (np.abs(d[0, :, 3:6]).max(axis=1) > 0.3).all()      # 30 N s on 32 kg
    assert np.array_equal(plain["com_vel"][:3], pushed["com_vel"][:3]) and np.abs(plain["com_vel"][3] - pushed["com_vel"][3]).max() > 0.1
