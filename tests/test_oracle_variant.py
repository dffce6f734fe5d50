"""The oracle's study variant and robot model belong to ONE env (oracle/ss_oracle.c: sso_variant, sso_create_model): a fresh env
judges the written specification, whatever another env of the process was told, in either precision build.  CPU only."""
import os
import re
import sys

import numpy as np
import pytest

import np_contact as npc
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 8


def run(o, steps, t0=0):
    """every output of `steps` random-action steps"""
    out = []
    for t in range(t0, t0 + steps):
        obs, rew, done, info = o.step(o.random_actions(t))
        out.append((obs, rew, done, info, o.get_state()))
    return out


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def fresh(prec="f32", seed=3, **kw):
    o = ol.OracleEnv("walker3d", N, seed=seed, prec=prec, **kw)
    o.set_curriculum(5)
    o.reset()
    return o


def test_a_fresh_env_judges_the_specification():
    tables = open(os.path.join(ROOT, "oracle", "ss_model_tables.h")).read()
    plank = {k: float(np.float32(re.search(r"#define SSO_PLANK_HALF_%s (\S+?)f\s" % k, tables).group(1))) for k in ("LENGTH", "WIDTH")}
    # PHYSICS.md 3.4: 5 sweeps, warm-started, ERP 0.2, Jacobi between the feet; 3.3: the plank; 6: dr = 0.65 + 0.6 u c/5; 4: on target
    # through a corner that stone n carries
    written = dict(iters=5, warm=1, seq_feet=0, target_carried=1, erp=0.2, plank_a=plank["LENGTH"], plank_b=plank["WIDTH"], stone_r=0.0,
                   dr_lo=0.65, dr_span=0.6, target_r=0.0)
    assert abs(plank["LENGTH"] - 0.30) < 1e-7 and abs(plank["WIDTH"] - 0.54) < 1e-7
    for prec in ("f32", "f64"):
        assert ol.spec_variant(prec) == written
        assert ol.OracleEnv("walker3d", N, prec=prec).variant() == written
        assert ol.OracleEnv("mike", 1, prec=prec).variant() == written


def test_variants_do_not_leak_between_envs_or_builds():
    steps = 30
    alone = {prec: run(fresh(prec), steps) for prec in ("f32", "f64")}
    envs = {}
    for prec in ("f32", "f64"):
        envs[prec, "spec"] = fresh(prec)
        envs[prec, "solver"] = fresh(prec, variant=dict(iters=8, warm=0, erp=0.9))
        envs[prec, "disc"] = fresh(prec)
        envs[prec, "disc"].set_variant(stone_r=0.25, target_carried=0)
    got = {k: [] for k in envs}
    for t in range(steps):
        for k in sorted(envs, key=lambda k: (k[1], k[0])):           # interleaved: variant envs step between the spec env's steps
            got[k] += run(envs[k], 1, t)
    for prec in ("f32", "f64"):
        for t in range(steps):
            assert same(got[prec, "spec"][t], alone[prec][t]), (prec, t)
        for name in ("solver", "disc"):
            assert not all(same(a, b) for a, b in zip(got[prec, name], alone[prec])), (prec, name)
        assert envs[prec, "spec"].variant() == ol.spec_variant()
        assert envs[prec, "solver"].variant() == dict(ol.spec_variant(), iters=8, warm=0, erp=0.9)
        assert envs[prec, "disc"].variant() == dict(ol.spec_variant(), stone_r=0.25, target_carried=0)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_set_variant_without_fields_returns_to_the_specification(prec):
    spec, live = fresh(prec), fresh(prec)
    run(spec, 6)
    saved = spec.get_state()
    want = run(spec, 3, 6)
    live.set_variant(iters=16, warm=0, seq_feet=1, dr_lo=0.5, dr_span=0.3)
    under = run(live, 6)
    assert not np.array_equal(under[-1][4], saved)
    live.set_variant()
    assert live.variant() == ol.spec_variant()
    live.set_state(saved)
    got = run(live, 3, 6)
    assert all(same(a, b) for a, b in zip(got, want))


def test_the_model_belongs_to_the_env():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import sysid_policy as sp
    finally:
        sys.path.pop(0)
    from steppingstone_amd import model
    kind = "walker3d"
    want = run(fresh(), 10)
    st = fresh().get_state()[0].astype(np.float64)
    tau = np.linspace(-20, 20, 21)
    aba0, fk0 = ol.debug_aba(kind, st, tau), ol.debug_fk(kind, st)
    m = model.build(kind)
    assert all(same(a, b) for a, b in zip(run(fresh(model=sp.pack_model(m)), 10), want))     # the mirror IS the compiled-in table
    m["torque"] = np.asarray(m["torque"], float) * 0.5
    m["damping"] = np.asarray(m["damping"], float) * 2.0
    weak = fresh(model=sp.pack_model(m))
    assert same(ol.debug_aba(kind, st, tau), aba0) and same(ol.debug_fk(kind, st), fk0)
    after = fresh()                                     # created without a model while `weak` lives
    got_weak, got_after = [], []
    for t in range(10):
        got_weak += run(weak, 1, t)
        got_after += run(after, 1, t)
    assert same(ol.debug_aba(kind, st, tau), aba0) and same(ol.debug_fk(kind, st), fk0)
    assert all(same(a, b) for a, b in zip(got_after, want))
    assert not all(same(a, b) for a, b in zip(got_weak, want))


def test_plank_fields_are_independent():
    """A robot set 0.1 m forward and so far into a flat stone 0 that its (pitched) soles are under the surface has all eight sole
    corners in contact with the specification's plank.  Narrowing ONLY the plank's width drops exactly the corners beyond the new
    width (their |v| lies between the two widths), narrowing ONLY its length exactly those beyond the new length: the field that
    was not named keeps the specification's value."""
    kind = "walker3d"
    spec = ol.spec_variant()
    one = ol.OracleEnv(kind, 1, seed=0, prec="f64")
    one.reset()
    st = one.get_state()
    st[0, ol.S_POS] += [0.1, 0.0, -0.075]
    pos, rot = ol.debug_fk(kind, st[0])
    corners = np.asarray(npc.rounded_model(kind)["corners"], float)
    P = np.array([pos[b] + rot[b] @ (c * [1, sgn, 1]) for b, sgn in ((8, 1), (13, -1)) for c in corners])   # tap order: right 0-3, left 0-3
    u, v = np.abs(P[:, 0]), np.abs(P[:, 1])                        # stone 0: at the origin, heading 0, flat
    assert (P[:, 2] < 0).all() and (P[:, 2] > -0.10).all() and (u < spec["plank_a"]).all() and (v < spec["plank_b"]).all()

    def active(**fields):
        one.set_variant(**fields)
        one.set_state(st)
        return one.debug_contact(0, np.zeros(21))["active"].astype(bool)

    assert active().all()
    narrow_b, narrow_a = 0.5 * (v.min() + v.max()), 0.5 * (u.min() + u.max())
    assert 0 < (v < narrow_b).sum() < 8 and 0 < (u < narrow_a).sum() < 8 and narrow_b < spec["plank_b"] and narrow_a < spec["plank_a"]
    assert np.array_equal(active(plank_b=narrow_b), v < narrow_b)
    assert one.variant() == dict(spec, plank_b=narrow_b)
    assert np.array_equal(active(plank_a=narrow_a), u < narrow_a)
    assert one.variant() == dict(spec, plank_a=narrow_a)
    assert np.array_equal(active(plank_a=narrow_a, plank_b=narrow_b), (u < narrow_a) & (v < narrow_b))


def test_step_margins_is_step_ex_asked_for_margins_alone():
    a, b, c = fresh(), fresh(), fresh()
    for t in range(12):
        act = a.random_actions(t)
        plain = a.step(act)
        obs, rew, done, info, margins = b.step_margins(act)
        ex = c.step_ex(act, tol=1e-5)
        assert same((obs, rew, done, info), plain)
        assert np.array_equal(margins, ex["margins"]) and margins.shape == (N, 2) and (margins >= 0).all()
        assert set(c.step_ex(act, margins=True)) == {"obs", "rew", "done", "info", "margins"}
        c.set_state(b.get_state())
