"""Independent numpy (float64) restatement of docs/RENDER.md: camera, scene, shading and outputs of one env's frame.

TEST INFRASTRUCTURE: it shares no code with the HIP renderer (steppingstone_amd/csrc/ss_render.hpp); the robot's shapes and kinematics
come from the specification itself (steppingstone_amd/model.py: visual_geoms, build, fk).  tests/test_render_numpy.py checks it on
analytic scenes, tests/test_render_host.py and tests/test_gpu_render.py compare the kernel's frames with it."""
import numpy as np

from steppingstone_amd import model

SEG_STONE = 23
TRACK, CHASE, FIXED = 0, 1, 2
STONE_THICKNESS = 0.10                                        # PHYSICS.md 3.3: -0.10 < d < 0
GROUP_ALBEDO = np.array([[0.80, 0.45, 0.25], [0.75, 0.50, 0.30], [0.70, 0.42, 0.28], [0.25, 0.45, 0.75],
                         [0.30, 0.58, 0.82], [0.20, 0.24, 0.32], [0.85, 0.66, 0.35], [0.92, 0.78, 0.48]])
STONE_ALBEDO = np.array([[0.58, 0.57, 0.53], [0.86, 0.32, 0.28], [0.58, 0.57, 0.53]])
LIGHT = np.array([-0.4, -0.6, 1.0]) / np.linalg.norm([-0.4, -0.6, 1.0])
AMBIENT, DIFFUSE = 0.30, 0.70
HORIZON, ZENITH = np.array([0.86, 0.89, 0.93]), np.array([0.32, 0.52, 0.82])
SHADOW_BIAS = 1e-3
DEFAULT_CAMERA = dict(mode=TRACK, eye=(-0.9, -2.3, 0.45), target=(0.4, 0.0, -0.5), fov_y_deg=45.0, far_m=20.0, shadows=True)


def quat_matrix(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def body_poses(kind, state):
    """[22, 12]: position | R row-major of every body (model.fk of the packed state)."""
    state = np.asarray(state, np.float64)
    R, p = model.fk(model.build(kind), state[13:34], state[0:3], quat_matrix(state[3:7]))
    return np.array([np.concatenate([p[b], R[b].reshape(-1)]) for b in range(model.NB)])


def stone_normal(phi, xt, yt):
    def rx(a):
        return np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])

    def ry(a):
        return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])

    def rz(a):
        return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    return (rz(phi) @ ry(yt) @ rx(xt))[:, 2]


def scene(kind, state):
    """The primitives of one env, in closest-hit order: the robot's (model.visual_geoms), then the stones n-1, n, n+1.  Each is a dict:
    type "capsule" (a, b, r) | "sphere" (a, r) | "slabs" (a, w [3,3], lo, hi), seg, albedo."""
    state = np.asarray(state, np.float64)
    poses = body_poses(kind, state)
    groups = model.body_groups(kind)
    prims = []
    for b, t, prm in model.visual_geoms(kind):
        p, R = poses[b, :3], poses[b, 3:].reshape(3, 3)
        alb = GROUP_ALBEDO[model.MASS_GROUPS.index(groups[b])]
        if t == "capsule":
            prims.append(dict(type="capsule", a=p + R @ prm["p0"], b=p + R @ prm["p1"], r=float(prm["r"]), seg=1 + b, albedo=alb))
        elif t == "sphere":
            prims.append(dict(type="sphere", a=p + R @ prm["c"], r=float(prm["r"]), seg=1 + b, albedo=alb))
        else:
            prims.append(dict(type="slabs", a=p + R @ prm["c"], w=R.T.copy(), lo=-prm["half"], hi=prm["half"].copy(), seg=1 + b,
                              albedo=alb))
    ec = model.env_constants()
    half_l, half_w = ec["stone_plank_half_length"], ec["stone_plank_half_width"]
    terr = state[65:185].reshape(20, 6)
    n = int(state[59])
    for sl, k in enumerate((max(n - 1, 0), n, min(n + 1, 19))):
        s, phi, xt, yt = terr[k, :3], terr[k, 3], terr[k, 4], terr[k, 5]
        nn = stone_normal(phi, xt, yt)
        hu, hv = np.array([np.cos(phi), np.sin(phi), 0.0]), np.array([-np.sin(phi), np.cos(phi), 0.0])
        w = np.array([nn, hu - (nn @ hu) * nn, hv - (nn @ hv) * nn])
        prims.append(dict(type="slabs", a=s, w=w, lo=np.array([-STONE_THICKNESS, -half_l, -half_w]),
                          hi=np.array([0.0, half_l, half_w]), seg=SEG_STONE + sl, albedo=STONE_ALBEDO[sl]))
    return prims


def camera(cam, state):
    """eye, f, r, u (docs/RENDER.md 1)."""
    mode, eye_o, tgt_o = cam["mode"], np.asarray(cam["eye"], float), np.asarray(cam["target"], float)
    if mode == FIXED:
        tgt, eye = tgt_o, eye_o
    else:
        pos = np.asarray(state[0:3], float) if state is not None else np.zeros(3)
        c, s = 1.0, 0.0
        if mode == CHASE and state is not None:
            w, x, y, z = np.asarray(state[3:7], float)
            A, B = 1 - 2 * (y * y + z * z), 2 * (w * z + x * y)
            if A * A + B * B > 1e-30:
                c, s = A / np.hypot(A, B), B / np.hypot(A, B)
        rot = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
        tgt = pos + rot @ tgt_o
        eye = tgt + rot @ eye_o
    f = (tgt - eye) / np.linalg.norm(tgt - eye)
    r = np.cross(f, [0, 0, 1.0])
    if r @ r < 1e-12:
        r = np.cross(f, [1.0, 0, 0])
    r /= np.linalg.norm(r)
    return eye, f, r, np.cross(r, f)


def rays(cam, W, H, eye, f, r, u):
    ky = np.tan(np.deg2rad(cam["fov_y_deg"]) / 2)
    kx = ky * W / H
    j, i = np.meshgrid(np.arange(W), np.arange(H))
    sx, sy = 2 * (j + 0.5) / W - 1, 1 - 2 * (i + 0.5) / H
    d = f + (sx * kx)[..., None] * r + (sy * ky)[..., None] * u
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def intersect(p, o, d):
    """Nearest entering t > 0 of rays o + t d (o [K,3] or [3], d [K,3] unit) with primitive p, NaN for a miss; unit normals [K,3]."""
    o = np.broadcast_to(o, d.shape)
    K = d.shape[0]
    t = np.full(K, np.nan)
    cen = np.zeros((K, 3))
    with np.errstate(all="ignore"):
        if p["type"] == "sphere":
            oc = o - p["a"]
            b = np.einsum("ij,ij->i", oc, d)
            h = b * b - (np.einsum("ij,ij->i", oc, oc) - p["r"] ** 2)
            tt = -b - np.sqrt(h)
            ok = (h >= 0) & (tt > 0)
            t[ok] = tt[ok]
            cen[:] = p["a"]
        elif p["type"] == "capsule":
            ba, oa = p["b"] - p["a"], o - p["a"]
            baba, bard, baoa = ba @ ba, d @ ba, oa @ ba
            rdoa, oaoa = np.einsum("ij,ij->i", d, oa), np.einsum("ij,ij->i", oa, oa)
            A = baba - bard * bard
            B = baba * rdoa - baoa * bard
            C = baba * oaoa - baoa * baoa - p["r"] ** 2 * baba
            h = B * B - A * C
            ts = (-B - np.sqrt(h)) / A
            y = baoa + ts * bard
            side = (h >= 0) & (y > 0) & (y < baba)
            ok_side = side & (ts > 0)
            t[ok_side] = ts[ok_side]
            cen[ok_side] = p["a"] + (y[ok_side] / baba)[:, None] * ba
            cap = (h >= 0) & ~side
            e = np.where((y <= 0)[:, None], p["a"], p["b"])
            oc = o - e
            b2 = np.einsum("ij,ij->i", d, oc)
            h2 = b2 * b2 - (np.einsum("ij,ij->i", oc, oc) - p["r"] ** 2)
            t2 = -b2 - np.sqrt(h2)
            ok_cap = cap & (h2 > 0) & (t2 > 0)
            t[ok_cap] = t2[ok_cap]
            cen[ok_cap] = e[ok_cap]
        else:
            den = d @ p["w"].T                                  # [K, 3]
            num = (o - p["a"]) @ p["w"].T
            t1, t2 = (p["lo"] - num) / den, (p["hi"] - num) / den
            te, tx = np.fmin(t1, t2), np.fmax(t1, t2)          # IEEE minNum / maxNum: a NaN (0 / 0) gives way
            te, tx = np.where(np.isnan(te), -np.inf, te), np.where(np.isnan(tx), np.inf, tx)
            kn = np.argmax(te, axis=1)
            tn = te[np.arange(K), kn]
            tf = tx.min(axis=1)
            ok = (tn <= tf) & (tn > 0)
            t[ok] = tn[ok]
            sgn = np.where(den[np.arange(K), kn] > 0, -1.0, 1.0)
            wn = p["w"][kn] / np.linalg.norm(p["w"][kn], axis=1, keepdims=True)
            n = sgn[:, None] * wn
            return t, n
    n = (o + np.nan_to_num(t)[:, None] * d - cen) / p["r"]
    return t, n


def render(kind, state, W, H, cam=None, counters=None):
    """One env's frame: rgb uint8 [H,W,3], depth float64 [H,W], seg uint8 [H,W], and aux = {prim: closest primitive index or -1,
    shadow: bool (lit side, shadow ray blocked)}.  state: the packed [186] state, or None for an empty scene (an invalid env id).
    counters (dict, optional): accumulates "primary" and "shadow" ray-primitive tests as the kernel's loops execute them (every
    primitive for a primary ray -- before the kernel's tile culling -- and primitives up to the first blocker for a shadow ray)."""
    cam = dict(DEFAULT_CAMERA, **(cam or {}))
    prims = scene(kind, state) if state is not None else []
    return render_prims(prims, camera(cam, state), cam, W, H, counters)


def render_prims(prims, basis, cam, W, H, counters=None):
    """render() of an explicit primitive list (scene() format) seen by the camera basis (eye, f, r, u)."""
    eye, f, r, u = basis
    d = rays(cam, W, H, eye, f, r, u).reshape(-1, 3)
    K = d.shape[0]
    df = d @ f
    best, hit, nrm = np.full(K, np.inf), np.full(K, -1), np.zeros((K, 3))
    for k, p in enumerate(prims):
        t, n = intersect(p, eye, d)
        better = (t > 0) & (t < best) & (t * df < cam["far_m"])
        best[better], hit[better], nrm[better] = t[better], k, n[better]
    if counters is not None:
        counters["primary"] = counters.get("primary", 0) + K * len(prims)
        counters["pixels"] = counters.get("pixels", 0) + K
    s = np.clip(0.5 + 0.5 * d[:, 2], 0, 1)
    rgb = (1 - s)[:, None] * HORIZON + s[:, None] * ZENITH
    depth = np.full(K, float(cam["far_m"]))
    seg = np.zeros(K, np.uint8)
    shadow = np.zeros(K, bool)
    m = hit >= 0
    if m.any():
        x = eye + best[m, None] * d[m]
        n = nrm[m]
        lit = np.maximum(n @ LIGHT, 0.0)
        if cam.get("shadows", True):
            idx = np.nonzero(lit > 0)[0]
            so = x[idx] + SHADOW_BIAS * n[idx]
            L = np.broadcast_to(LIGHT, so.shape)
            blocked = np.zeros(len(idx), bool)
            for p in prims:
                if counters is not None:
                    counters["shadow"] = counters.get("shadow", 0) + int((~blocked).sum())
                t, _ = intersect(p, so, L)
                blocked |= t > 0
            lit[idx[blocked]] = 0.0
            sh = np.zeros(m.sum(), bool)
            sh[idx[blocked]] = True
            shadow[m] = sh
        alb = np.array([prims[k]["albedo"] for k in hit[m]])
        rgb[m] = alb * (AMBIENT + DIFFUSE * lit)[:, None]
        depth[m] = best[m] * df[m]
        seg[m] = [prims[k]["seg"] for k in hit[m]]
    rgb8 = np.floor(np.clip(rgb, 0, 1) * 255 + 0.5).astype(np.uint8)
    aux = dict(prim=hit.reshape(H, W), shadow=shadow.reshape(H, W))
    return rgb8.reshape(H, W, 3), depth.reshape(H, W), seg.reshape(H, W), aux


def edges(a):
    """True where the 3x3 neighbourhood of a pixel holds more than one value of `a` [H, W]."""
    p = np.pad(a, 1, mode="edge")
    H, W = a.shape
    out = np.zeros((H, W), bool)
    for di in (0, 1, 2):
        for dj in (0, 1, 2):
            out |= p[di:di + H, dj:dj + W] != a
    return out


def compare(frame, ref, label=""):
    """The tolerances of tests/test_render_host.py and tests/test_gpu_render.py: segmentation mismatches <= 0.3 % of the pixels, each
    on a silhouette edge of the numpy frame; where the ids agree depth within 1e-4 depth + 1e-5 and, away from primitive and shadow
    edges, RGB within 2.  frame = (rgb, depth, seg) of the kernel, ref = np_render.render(...)."""
    rgb, depth, seg = frame
    rrgb, rdepth, rseg, aux = ref
    H, W = rseg.shape
    bad = seg != rseg
    assert bad.mean() <= 0.003, "%s: %d of %d segmentation ids differ" % (label, bad.sum(), H * W)
    assert not (bad & ~edges(rseg)).any(), "%s: segmentation differs away from a silhouette edge at %s" % (
        label, np.argwhere(bad & ~edges(rseg))[:5].tolist())
    ok = ~bad
    derr = np.abs(depth.astype(np.float64) - rdepth)
    assert (derr[ok] <= 1e-4 * rdepth[ok] + 1e-5).all(), "%s: depth off by up to %.3g" % (label, derr[ok].max())
    smooth = ok & ~edges(aux["prim"]) & ~edges(aux["shadow"])
    cerr = np.abs(rgb.astype(int) - rrgb.astype(int)).max(axis=-1)
    assert (cerr[smooth] <= 2).all(), "%s: rgb off by up to %d at %s" % (label, cerr[smooth].max(),
                                                                           np.argwhere(smooth & (cerr > 2))[:5].tolist())
    return dict(seg_mismatch=int(bad.sum()), depth_err=float(derr[ok].max()) if ok.any() else 0.0,
                rgb_err=int(cerr[smooth].max()) if smooth.any() else 0)         # a 4 x 4 frame can be all edges
