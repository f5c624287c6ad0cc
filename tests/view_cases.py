"""Shared inputs of the free-viewpoint render tests (kfx_render_view, DESIGN.md
§18): the scene, the view cameras, and the numpy restatement of the hit vertex
in volume coordinates, of the fused-colour blend and of its Phong fallback.

The restated vertex is P = org + dir * Ts with dir in the oracle's written
float32 order (kfx_oracle.cpp raycast_impl) and org = cam2vol.t; pushed through
Rinv * (P - org) it must reproduce the oracle's vmap bit for bit
(test_view_restatement.py), which is what makes the colour restatement below a
reference for the GPU."""
import functools

import numpy as np

import oracle as O
from kfx import synth
from kfx.abi import Intrinsics, default_params

F = np.float32
RANGE_M = 2.048
N_FRAMES = 4
DIMS = (64, 128)


@functools.lru_cache(maxsize=None)
def scene():
    intr = synth.Intrinsics.qvga()
    bgr, dep, _ = synth.sequence(5, intr, noise=True, dropout=0.01)
    return intr, bgr[:N_FRAMES], dep[:N_FRAMES].astype(np.float32)


def params(dims):
    return default_params(dims=dims, range_m=RANGE_M)


@functools.lru_cache(maxsize=None)
def fused(dims):
    """Oracle pipeline over the scene: (tsdf, weight, rgb (nvox, 4) u8, poses)."""
    intr, bgr, dep = scene()
    pipe = O.Pipeline(Intrinsics.from_any(intr), params(dims))
    for k in range(N_FRAMES):
        assert pipe.process(bgr[k], dep[k]) == 0
    t, w, c = pipe.volume()
    for a in (t, w, c):
        a.setflags(write=False)
    return t, w, c.reshape(-1, 4), pipe.poses()


def _rot(axis, ang):
    c, s = np.cos(ang), np.sin(ang)
    m = np.eye(4)
    i, j = {"x": (1, 2), "y": (2, 0)}[axis]
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def _pose(last, tx, ay, ax):
    T = np.eye(4)
    T[:3, 3] = (tx, 0.05, -0.1)
    return (last.astype(np.float64) @ T @ _rot("y", ay) @ _rot("x", ax)).astype(F)


def _intr(W, H, s):
    q = synth.Intrinsics.qvga()
    return Intrinsics(W, H, float(F(q.fx * s)), float(F(q.fy * s * 1.02)), float(F(W / 2 - 0.5 + 3.25)),
                      float(F(H / 2 - 0.5 - 1.5)))


# (W, H, s, ay, ax, tx)
VIEW_OFF = (200, 152, 0.55, 0.35, -0.1, -0.45)   # off-trajectory
VIEW_ODD = (97, 61, 0.3, -0.3, 0.15, 0.4)        # odd sizes: partly filled tiles in both directions
VIEW_QVGA = (320, 240, 1.0, 0.0, 0.0, 0.0)       # tracker-sized
VIEW_BIG = (400, 300, 1.25, 0.2, -0.05, -0.2)    # larger than the tracker's image


def make_view(spec, last):
    W, H, s, ay, ax, tx = spec
    return _intr(W, H, s), _pose(last, tx, ay, ax)


def views(last):
    """[(name, Intrinsics, 4x4 float32 camera-to-world pose)] for a last tracked pose."""
    out = [(n, *make_view(sp, last)) for n, sp in (("off", VIEW_OFF), ("odd", VIEW_ODD), ("qvga", VIEW_QVGA))]
    out.append(("own", Intrinsics.from_any(synth.Intrinsics.qvga()), last.astype(F)))
    out.append(("big", *make_view(VIEW_BIG, last)))
    out.append(("miss", Intrinsics.from_any(synth.Intrinsics.qvga()),
                (last.astype(np.float64) @ _rot("y", np.pi)).astype(F)))
    return out


def cam2vol(p, pose):
    """(cam2vol Pose, Rinv (9,) float32) in the library's float arithmetic."""
    c2v = O.pose_mul(O.pose_inv(p.volu_pose), O.Pose.from_matrix(pose))
    R = np.array(c2v.R[:], F).reshape(3, 3)
    return c2v, np.ascontiguousarray(R.T).reshape(9)


def oracle_view(dims, intr, pose):
    """The reference raycast of the fused volume at the view: (vmap, nmap, ts)."""
    t, _, _, _ = fused(dims)
    p = params(dims)
    vol = O.Volume((dims,) * 3, (RANGE_M,) * 3)
    c2v, Rinv = cam2vol(p, pose)
    _, v, n, ts = O.raycast_slab(t, vol, intr, c2v, Rinv, 0, dims, 0, dims)
    return v, n, ts


def restate_vertex(p, intr, pose, ts):
    """P = org + dir * Ts per component, (H, W, 3) float32, and org."""
    c2v, _ = cam2vol(p, pose)
    R = np.array(c2v.R[:], F)
    org = np.array(c2v.t[:], F)
    x = np.arange(intr.width, dtype=F)[None, :]
    y = np.arange(intr.height, dtype=F)[:, None]
    p0 = np.broadcast_to((F(1) * (x - F(intr.cx))) / F(intr.fx), (intr.height, intr.width))
    p1 = np.broadcast_to((F(1) * (y - F(intr.cy))) / F(intr.fy), (intr.height, intr.width))
    p2 = F(1)
    v = [R[3 * i] * p0 + R[3 * i + 1] * p1 + R[3 * i + 2] * p2 for i in range(3)]
    t = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    P = np.stack([org[i] + (v[i] / t) * ts for i in range(3)], axis=-1)
    assert P.dtype == F
    return P, org


def restate_vmap(p, pose, P, org):
    """Rinv * (P - org): the oracle's vmap from the restated vertex."""
    _, Rinv = cam2vol(p, pose)
    w = [P[..., i] - org[i] for i in range(3)]
    return np.stack([Rinv[3 * i] * w[0] + Rinv[3 * i + 1] * w[1] + Rinv[3 * i + 2] * w[2] for i in range(3)], axis=-1)


def corners(p, P):
    """Cell g (H, W, 3) int64 and the 8-bit fractions q of the restated vertex."""
    dims = np.array(p.volu_dims[:], np.int64)
    vs = (np.array(p.volu_range[:], F) / dims.astype(F)).astype(F)
    vs_inv = F(1) / vs
    cf = P * vs_inv
    gf = np.floor(cf)
    q = ((cf - gf) * F(256)).astype(np.int64)
    return gf.astype(np.int64), q, dims


def restate_colour(p, P, hit, rgb, phong):
    """The colour image of DESIGN.md §18 in integers: (image, coloured-hit mask)."""
    g, q, dims = corners(p, P)
    X, Y, Z = (int(d) for d in dims)
    sw = np.zeros(hit.shape, np.int64)
    sc = np.zeros(hit.shape + (3,), np.int64)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                x, y, z = g[..., 0] + dx, g[..., 1] + dy, g[..., 2] + dz
                inside = hit & (x >= 0) & (x < X) & (y >= 0) & (y < Y) & (z >= 0) & (z < Z)
                idx = np.where(inside, x + y * X + z * X * Y, 0)
                c = rgb[idx, :3].astype(np.int64)
                counts = inside & (c.any(axis=-1))
                W = np.where(counts, (q[..., 0] if dx else 256 - q[..., 0]) * (q[..., 1] if dy else 256 - q[..., 1]) *
                             (q[..., 2] if dz else 256 - q[..., 2]), 0)
                sw += W
                sc += W[..., None] * c
    assert sw.max() <= 1 << 24
    col = hit & (sw > 0)
    den = np.where(col, sw, 1)
    img = ((sc + (den >> 1)[..., None]) // den[..., None]).astype(np.uint8)
    out = np.where(col[..., None], img, np.where(hit[..., None], phong, 0)).astype(np.uint8)
    return out, col


def reference(dims, intr, pose):
    """Everything a view must equal: dict of vmap, nmap, ts, phong, normal, color."""
    p = params(dims)
    _, _, rgb, _ = fused(dims)
    v, n, ts = oracle_view(dims, intr, pose)
    eye = pose[:3, 3]
    phong = O.render(v, n, eye, "phong")
    hit = ts != 0
    P, _ = restate_vertex(p, intr, pose, ts)
    color, col = restate_colour(p, P, hit, rgb, phong)
    return dict(vmap=v, nmap=n, ts=ts, phong=phong, normal=O.render(v, n, eye, "normal"), color=color, hit=hit,
                coloured=col)
