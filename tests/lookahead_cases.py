"""The case set of the look-ahead (ss_lookahead, docs/PHYSICS.md 13), shared by tests/test_lookahead.py (the CPU build of
ss_lookahead.hpp against the CPU build of step_env) and tests/test_gpu_lookahead.py (the kernel against ss_step).

Per robot 64 (state, action sequence) pairs with H = 24, held as a fixture (tests/golden/lookahead_cases_<kind>.npz: st [64,186] f32,
act [64,24,21] f32), because the recipe below runs a torch actor whose last bits may differ between machines while every test here is
bitwise.  `python tests/lookahead_cases.py` rewrites the fixtures.  The recipe (make):
  rows 0..39   the reference's shipped actor (tests/golden/shipped_actor_<kind>.npz) walks 40 envs of the fp32 oracle at curriculum 3,
               seed 21, for WALK[kind] control steps; the state then, and as actions the actor's own, closed loop over 24 steps of the CPU
               build of step_env with auto-reset off -- so that the branches advance their targets, draw stones and touch new ones.
               Row 0 has elapsed = 997 (the time limit ends it in its third step), row 1 a NaN action in its sixth step, rows 2 and 3 the
               terrain rows and the target index shifted so that the stone ahead is the last one (an advance onto stone 19: no draw).
  rows 40..63  24 envs of the same oracle after a reset and three steps of random actions, under 24 further random action rows scaled by
               1, 2 or 3 (the clip makes the large ones bang-bang): the falls.
SEED and CURRICULUM are what a test instantiates its env with; the set is judged (test_lookahead.py) by what the CPU build of step_env
sees on it: advances with and without a draw, first-touch bonuses, falls, the time limit, the NaN and survivors."""
import functools
import os

import numpy as np

KINDS = ("walker3d", "mike")
ENV_IDS = {"walker3d": "Walker3DStepperEnv-v0", "mike": "MikeStepperEnv-v0"}
N_CASES, H = 64, 24
SEED, CURRICULUM = 21, 3
WALK = {"walker3d": 90, "mike": 60}
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
S_N, S_COUNT, S_ELAPSED = 59, 60, 61


def path(kind):
    return os.path.join(GOLD, "lookahead_cases_%s.npz" % kind)


@functools.lru_cache(maxsize=None)
def cases(kind):
    """-> dict: st [64,186] float32, act [64,24,21] float32 (read-only)"""
    z = np.load(path(kind))
    st, act = z["st"].astype(np.float32), z["act"].astype(np.float32)
    assert st.shape == (N_CASES, 186) and act.shape == (N_CASES, H, 21)
    st.setflags(write=False)
    act.setflags(write=False)
    return dict(st=st, act=act)


def tile(kind, n):
    """the case set tiled onto n envs: env e holds case e % 64 -> (st [n,186], act [n,24,21])"""
    c = cases(kind)
    idx = np.arange(n) % N_CASES
    return c["st"][idx].copy(), c["act"][idx].copy()


def step_reference(kind, st, act, seed=SEED, curriculum=CURRICULUM):
    """The CPU build of step_env, auto-reset off, stepped act.shape[1] times from st [N,186] under act [N,H,21] -> dict: obs [N,H,60], rew
    [N,H], done [N,H] bool, info [N,H] (host_lib.INFO_DTYPE), state [H,N,186] (the packed state after every step)"""
    import lookahead_host_lib as lh
    k = KINDS.index(kind)
    n, h = act.shape[:2]
    out = dict(obs=np.zeros((n, h, 60), np.float32), rew=np.zeros((n, h), np.float32), done=np.zeros((n, h), bool),
               info=np.zeros((n, h), lh.INFO_DTYPE), state=np.zeros((h, n, 186), np.float32))
    cur = np.ascontiguousarray(st, np.float32)
    for s in range(h):
        cur, o, r, d, i = lh.step(k, cur, act[:, s], seed=seed, curriculum=curriculum, auto_reset=False)
        out["obs"][:, s], out["rew"][:, s], out["done"][:, s], out["info"][:, s], out["state"][s] = o, r, d != 0, i, cur
    return out


def events(kind, st, act):
    """what the CPU build of step_env sees on (st, act) up to each row's first done -> dict of counts"""
    ref = step_reference(kind, st, act)
    n, h = act.shape[:2]
    done = ref["done"]
    first = np.where(done.any(1), done.argmax(1), h)                       # index of the first done step, h: none
    live = np.arange(h)[None, :] <= first[:, None]                        # steps up to and including it
    before = np.concatenate([np.asarray(st, np.float32)[None], ref["state"][:-1]], 0).transpose(1, 0, 2)      # [N,H,186]
    after = ref["state"].transpose(1, 0, 2)
    adv = (ref["info"]["update_terrain"] != 0) & live
    touch = (before[..., S_COUNT] == 0) & (after[..., S_COUNT] == 1) & live
    nan_row = np.isnan(act).any((1, 2))
    ended = first < h
    limit = ended & (after[np.arange(n), np.minimum(first, h - 1), S_ELAPSED] >= 1000)
    return dict(draws=int((adv & (after[..., S_N] <= 18)).sum()), last_stone=int((adv & (after[..., S_N] == 19)).sum()),
                touches=int(touch.sum()), falls=int((ended & ~limit & ~nan_row & (first < h - 1)).sum()), time_limit=int(limit.sum()),
                nan=int((ended & nan_row).sum()), alive=int((~ended).sum()), first=first)


def make(kind):
    import torch
    import lookahead_host_lib as lh
    import oracle_lib as ol
    import shipped_actor as sa
    k = KINDS.index(kind)
    actor = sa.load_actor(kind)
    o = ol.OracleEnv(kind, 40, seed=SEED)
    o.set_curriculum(CURRICULUM)
    obs = o.reset()
    for t in range(WALK[kind]):
        with torch.no_grad():
            obs, _, _, _ = o.step(actor(torch.from_numpy(obs)).numpy())
    walk = o.get_state().astype(np.float32)
    o.close()
    walk[0, S_ELAPSED] = 997
    for e in (2, 3):                                   # stones n-1, n, n+1 become 17, 18, 19; the stones behind them lie on n-1
        n = int(walk[e, S_N])
        terr = walk[e, 65:185].reshape(20, 6).copy()
        new = np.repeat(terr[n - 1:n], 20, 0)
        new[17:20] = terr[n - 1:n + 2]
        walk[e, 65:185] = new.reshape(120)
        walk[e, S_N] = 18
    wact = np.zeros((40, H, 21), np.float32)
    cur = walk.copy()
    o = ol.OracleEnv(kind, 40, seed=SEED)              # get_obs of a packed state
    o.set_curriculum(CURRICULUM)
    o.reset()
    for s in range(H):
        o.set_state(cur)
        with torch.no_grad():
            wact[:, s] = actor(torch.from_numpy(o.get_obs())).numpy()
        cur = lh.step(k, cur, wact[:, s], seed=SEED, curriculum=CURRICULUM, auto_reset=False)[0]
    o.close()
    wact[1, 5, 7] = np.nan
    o = ol.OracleEnv(kind, 24, seed=SEED + 1)
    o.set_curriculum(CURRICULUM)
    o.reset()
    for t in range(3):
        o.step(o.random_actions(t))
    fall = o.get_state().astype(np.float32)
    fact = np.stack([o.random_actions(100 + s) for s in range(H)], 1).astype(np.float32) * (1 + np.arange(24) % 3)[:, None, None]
    o.close()
    return np.concatenate([walk, fall]), np.concatenate([wact, fact.astype(np.float32)])


if __name__ == "__main__":
    for kind in KINDS:
        st, act = make(kind)
        ev = events(kind, st, act)
        print(kind, {k: v for k, v in ev.items() if k != "first"}, "first done:", ev["first"].tolist())
        np.savez_compressed(path(kind), st=st, act=act)
