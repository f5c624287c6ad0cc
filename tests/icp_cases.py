"""Crafted inputs for the ICP correspondence gates and its 27-term reduction,
and a plain numpy restatement of one ICP accumulation to judge them by.

accumulate_np restates rigid_icp.cu:46-113 as the oracle states it
(kfo_icp_accumulate): every operation a float32 numpy operation in the
oracle's association order, nothing fused, each product turned into fixed
point as rint(float32(a * b) * 2^32) and the 27 sums taken in Python integers.
It shares no code with the C++ oracle or the HIP kernels.

The generators build vertex / normal maps (current frame and model) aimed at
one class of edge each, for the identity pose, and return with them a label
per pixel of the floor-covered region: which gate must reject it, or that it
must be accepted.  All of them use power-of-two focal lengths and dyadic
principal points (crafted_intrinsics), so a vertex depth * ((u - cx) / fx,
(v - cy) / fy, 1) with a short depth projects back to (u, v) without rounding.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np

from kfx.abi import Intrinsics, Pose

f32 = np.float32
ACCEPT, NAN, PROJ, DIST, ANGLE = 0, 1, 2, 3, 4
GATES = {"nan": NAN, "proj": PROJ, "dist": DIST, "angle": ANGLE}
FIX = f32(4294967296.0)
INT_MIN = -(2 ** 31)
THREADS = 256  # kIcpThreads
BLOCK_PIX = 1024  # kIcpThreads * kIcpPix


# --------------------------------------------------------------------------
# restatement

def _c(a, k):
    return a[..., k]


def _dot(a, b):
    return _c(a, 0) * _c(b, 0) + _c(a, 1) * _c(b, 1) + _c(a, 2) * _c(b, 2)


def _cross(a, b):
    return np.stack([_c(a, 1) * _c(b, 2) - _c(a, 2) * _c(b, 1),
                     _c(a, 2) * _c(b, 0) - _c(a, 0) * _c(b, 2),
                     _c(a, 0) * _c(b, 1) - _c(a, 1) * _c(b, 0)], axis=-1)


def _rmul(R, v):
    return np.stack([R[3 * i] * _c(v, 0) + R[3 * i + 1] * _c(v, 1) + R[3 * i + 2] * _c(v, 2) for i in range(3)],
                    axis=-1)


def _f2i_rn(v):
    r = np.rint(v)
    ok = (r > f32(-2.0e9)) & (r < f32(2.0e9))
    return np.where(ok, np.where(ok, r, f32(0)).astype(np.int64), INT_MIN)


def region(w, h):
    return (w // 32) * 32, (h // 32) * 32


def accumulate_np(cur_v, cur_n, pre_v, pre_n, I, pose, dist_thr, angle_thr, keep_scaled=False):
    """One ICP accumulation.  Returns sums (27 Python ints), label (ye, xe:
    ACCEPT or the rejecting gate), accepted and rejected[gate] masks, terms
    (ye * xe, 27 int64: each pixel's fixed-point products, zero where
    rejected), the unrounded projection (pu, pv), |d|^2 and |sine|^2, and with
    keep_scaled the float32 products * 2^32 before rint."""
    cur_v, cur_n, pre_v, pre_n = (np.ascontiguousarray(a, f32) for a in (cur_v, cur_n, pre_v, pre_n))
    h, w = cur_v.shape[:2]
    assert (w, h) == (I.width, I.height)
    xe, ye = region(w, h)
    R = [f32(x) for x in pose.R]
    t = np.array([f32(x) for x in pose.t], f32)
    fx, fy, cx, cy = f32(I.fx), f32(I.fy), f32(I.cx), f32(I.cy)
    dist_thr, angle_thr = f32(dist_thr), f32(angle_thr)
    with np.errstate(all="ignore"):
        v0, n0 = cur_v[:ye, :xe], cur_n[:ye, :xe]
        nan = np.isnan(_c(n0, 0))
        vcur = _rmul(R, v0) + t
        pu = (_c(vcur, 0) / _c(vcur, 2)) * fx + cx
        pv = (_c(vcur, 1) / _c(vcur, 2)) * fy + cy
        px, py = _f2i_rn(pu), _f2i_rn(pv)
        inside = (_c(vcur, 2) > 0) & (px >= 0) & (py >= 0) & (px < w) & (py < h)
        j = np.where(inside, py * w + px, 0)
        vpre = pre_v.reshape(-1, 3)[j]
        npre = pre_n.reshape(-1, 3)[j]
        dd = vcur - vpre
        dist2 = _dot(dd, dd)
        near = np.sqrt(dist2) <= dist_thr
        ncur = _rmul(R, n0)
        sa = _cross(ncur, npre)
        sine2 = _dot(sa, sa)
        aligned = np.sqrt(sine2) <= angle_thr
        c = _cross(vcur, npre)
        row = np.concatenate([c, npre, _dot(npre, vpre - vcur)[..., None]], axis=-1)
        label = np.full((ye, xe), ACCEPT, np.int8)
        label[~aligned] = ANGLE
        label[~near] = DIST
        label[~inside] = PROJ
        label[nan] = NAN
        acc = label == ACCEPT
        terms = np.zeros((ye * xe, 27), np.int64)
        scaled = np.zeros((ye * xe, 27), f32) if keep_scaled else None
        flat = acc.ravel()
        rows = row.reshape(-1, 7)[flat]
        s = 0
        for a in range(6):
            for b in range(a, 7):
                sc = (rows[:, a] * rows[:, b]) * FIX
                assert np.all(np.abs(sc) < f32(2.0 ** 62))
                terms[flat, s] = np.rint(sc).astype(np.int64)
                if keep_scaled:
                    scaled[flat, s] = sc
                s += 1
    hi, lo = terms >> 32, terms & 0xFFFFFFFF  # exact in int64 for any pixel count below 2^31
    sums = [(int(hi[:, k].sum()) << 32) + int(lo[:, k].sum()) for k in range(27)]
    return SimpleNamespace(sums=sums, label=label, accepted=acc,
                           rejected={g: label == k for g, k in GATES.items()}, terms=terms, scaled=scaled,
                           pu=pu, pv=pv, px=px, py=py, dist2=dist2, sine2=sine2, row=row)


def sums_i64(sums):
    """The 27 Python-integer sums as int64 (they must fit: the oracle's and the kernel's are int64)."""
    assert all(-(2 ** 63) <= s < 2 ** 63 for s in sums)
    return np.array(sums, np.int64)


def block_sum_report(terms, plan):
    """For pixels grouped as `plan` groups them into blocks (an int: that many
    consecutive pixels of the region per block; a dict from
    KinectFusion.debug_cap_icp_blocks plus "level": that level's span or pixel
    group), per slot the largest |block sum| and the largest sum of |terms| of
    a block (a bound on every partial sum of any summation order), as Python
    integers.  Either below 2^53 means the fp64 additions of that block are
    exact in the first case for the totals, in the second for every order."""
    if isinstance(plan, dict):
        l = plan.get("level", 0)
        plan = plan["span"][l] if plan["span"][l] > 0 else THREADS * plan["ppl"][l]
    n = terms.shape[0]
    nb = (n + plan - 1) // plan
    pad = np.zeros((nb * plan, 27), np.int64)
    pad[:n] = terms
    pad = pad.reshape(nb, plan, 27)

    def exact(a):  # (nb, plan, 27) -> (nb, 27) Python ints
        hi, lo = (a >> 32).sum(axis=1), (a & 0xFFFFFFFF).sum(axis=1)
        return [[(int(hi[b, k]) << 32) + int(lo[b, k]) for k in range(27)] for b in range(nb)]

    tot, mag = exact(pad), exact(np.abs(pad))
    return SimpleNamespace(block_pixels=plan, blocks=nb,
                           max_abs_sum=[max(abs(tot[b][k]) for b in range(nb)) for k in range(27)],
                           max_sum_abs=[max(mag[b][k] for b in range(nb)) for k in range(27)])


# --------------------------------------------------------------------------
# thresholds

def sinf_deg(deg):
    """The sine threshold as the library and the oracle derive it from degrees
    (icp_registration.cpp:5): libm's sinf of the float32 product."""
    m = C.CDLL("libm.so.6")
    m.sinf.argtypes, m.sinf.restype = [C.c_float], C.c_float
    return f32(m.sinf(C.c_float(float(f32(deg) * f32(0.017453293)))))


def sqrt_le_bound(t):
    """The largest float32 x with float32 sqrt(x) <= t (t > 0, finite)."""
    t = f32(t)
    x, inf = f32(t * t), f32(np.inf)
    while np.sqrt(x) > t:
        x = np.nextafter(x, f32(0))
    while np.sqrt(np.nextafter(x, inf)) <= t:
        x = np.nextafter(x, inf)
    return x


def step(x, k):
    """x moved by k float32 ulps."""
    x = f32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, f32(np.inf) if k > 0 else f32(-np.inf))
    return x


def dist_thr_bound_above_square():
    """A distance threshold t near the default with sqrt_le_bound(t) above
    float32(t * t), so `|d|^2 <= t * t` would reject what `sqrt(|d|^2) <= t`
    admits.  (The opposite, a float32 t * t whose square root exceeds t, cannot
    happen in binary floating point: sqrt(RN(t * t)) = t.)"""
    t = f32(0.0125)
    while not sqrt_le_bound(t) > f32(t * t):
        t = np.nextafter(t, f32(1))
    return t


RUNGS = (-3, -2, -1, 0, 1, 2, 3)  # ulps of the squared quantity from sqrt_le_bound(t); <= 0 is accepted


# --------------------------------------------------------------------------
# scenes

def crafted_intrinsics(w, h):
    """Power-of-two focal length near 0.8 w and a dyadic principal point."""
    fx = 2.0 ** round(np.log2(0.8 * w))
    return Intrinsics(w, h, fx, fx, (w - 1) / 2.0, (h - 1) / 2.0)


def moved_pose():
    """A rotation (0.01 degrees about a skew axis) and a translation (under half
    a millimetre) small enough that most pixels keep their correspondence."""
    ax = np.array([0.3, 1.0, -0.2])
    ax /= np.linalg.norm(ax)
    a = np.deg2rad(0.01)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    m[:3, 3] = [0.0003, -0.0002, 0.0004]
    return Pose.from_matrix(m)


def special_pixels(npix):
    """Region pixels (linear index) at the first and last pixel, lanes 0 and 63,
    and both sides of a wave (64), a pixel-per-lane (256) and a block (1024) boundary."""
    s = [0, 1, 62, 63, 64, 65, 127, 128, 255, 256, 257, 1022, 1023, 1024, 1025, 2047, 2048]
    s += [npix - k for k in (1, 2, 63, 64, 65, 66, 256, 257, 1024, 1025)]
    return sorted({i for i in s if 0 <= i < npix})


def probe_pixels(npix, limit):
    """The special pixels first, then every 7th pixel, `limit` at the most."""
    sp = special_pixels(npix)
    rest = sorted(set(range(3, npix, 7)) - set(sp))
    if len(sp) + len(rest) > limit:
        keep = max(limit - len(sp), 0)
        rest = [rest[(k * len(rest)) // max(keep, 1)] for k in range(keep)]
    return sp + rest


def base_scene(I):
    """Benign maps: every region pixel is accepted under the identity pose and
    projects onto itself exactly.  Depths 1 + k / 8, three normals, and on half
    the pixels a model offset of 2^-9 m along z so the residual term is non-zero."""
    w, h = I.width, I.height
    u, v = np.meshgrid(np.arange(w, dtype=f32), np.arange(h, dtype=f32))
    z = f32(1) + ((3 * u + 5 * v) % 8).astype(f32) / f32(8)
    a = np.stack([(u - f32(I.cx)) / f32(I.fx), (v - f32(I.cy)) / f32(I.fy), np.ones_like(u)], axis=-1)
    cur_v = (a * z[..., None]).astype(f32)
    normals = np.array([[0, 0, -1], [0.6, 0, -0.8], [0, -0.6, -0.8]], f32)
    cur_n = normals[((u + 2 * v) % 3).astype(int)]
    pre_v, pre_n = cur_v.copy(), cur_n.copy()
    pre_v[..., 2] -= np.where((u + v) % 2 == 0, f32(2.0 ** -9), f32(0))
    xe, ye = region(w, h)
    return SimpleNamespace(I=I, w=w, h=h, xe=xe, ye=ye, npix=xe * ye, cur_v=cur_v, cur_n=cur_n.copy(), pre_v=pre_v,
                           pre_n=pre_n, label=np.zeros((ye, xe), np.int8), tag=np.full((ye, xe), -1, np.int16),
                           tags=[])


def _case(S, **meta):
    return SimpleNamespace(I=S.I, cur_v=S.cur_v, cur_n=S.cur_n, pre_v=S.pre_v, pre_n=S.pre_n, label=S.label,
                           tag=S.tag, tags=S.tags, **meta)


def _yx(S, i):
    return divmod(i, S.xe)


def _tag(S, y, x, name, label):
    if name not in S.tags:
        S.tags.append(name)
    S.tag[y, x] = S.tags.index(name)
    S.label[y, x] = label


def gen_invalid(I):
    """Class a: NaNs, zero / negative / denormal depth, NaN or zero model entries."""
    S = base_scene(I)
    nan, den = f32(np.nan), f32(1.4e-45)
    assert den > 0 and den == np.nextafter(f32(0), f32(1))

    def cur_nx(y, x): S.cur_n[y, x, 0] = nan
    def cur_ny(y, x): S.cur_n[y, x] = (0, nan, -1)
    def z_zero(y, x): S.cur_v[y, x, 2] = 0
    def z_negzero(y, x): S.cur_v[y, x, 2] = f32(-0.0)
    def z_neg(y, x): S.cur_v[y, x, 2] = -S.cur_v[y, x, 2]
    def z_denormal(y, x): S.cur_v[y, x, 2] = den
    def v_zero(y, x): S.cur_v[y, x] = 0
    def v_nan_x(y, x): S.cur_v[y, x, 0] = nan
    def v_nan_y(y, x): S.cur_v[y, x, 1] = nan
    def v_nan_z(y, x): S.cur_v[y, x, 2] = nan
    def m_nan_x(y, x): S.pre_v[y, x, 0] = nan
    def m_nan_z(y, x): S.pre_v[y, x, 2] = nan
    def mn_nan_x(y, x): S.pre_n[y, x, 0] = nan
    def mn_nan_z(y, x): S.pre_n[y, x, 2] = nan
    def mn_zero(y, x): S.pre_n[y, x] = 0

    variants = [(cur_nx, NAN), (cur_ny, ANGLE), (z_zero, PROJ), (z_negzero, PROJ), (z_neg, PROJ),
                (z_denormal, PROJ), (v_zero, PROJ), (v_nan_x, PROJ), (v_nan_y, PROJ), (v_nan_z, PROJ),
                (m_nan_x, DIST), (m_nan_z, DIST), (mn_nan_x, ANGLE), (mn_nan_z, ANGLE), (mn_zero, ACCEPT)]
    for k, i in enumerate(probe_pixels(S.npix, 600)):
        y, x = _yx(S, i)
        fn, lab = variants[k % len(variants)]
        fn(y, x)
        _tag(S, y, x, fn.__name__, lab)
    return _case(S)


def gen_projection(I, seed=7):
    """Class b: projections on rounding ties, at and around the four borders, and
    into the columns and rows beyond the 32-floor (never a source, legal targets)."""
    S = base_scene(I)
    w, h, xe, ye = S.w, S.h, S.xe, S.ye
    rng = np.random.default_rng(seed)
    probes = probe_pixels(S.npix, 170)
    taken = np.zeros((h, w), bool)
    for i in probes:
        taken[_yx(S, i)] = True
    order = rng.permutation(w * h)
    uu, vv = order % w, order // w

    def alloc(cond, du=0, dv=0):
        """A pixel (u, v) satisfying cond(u, v) such that (u + du, v + dv) is inside and free."""
        lu, lv = uu + du, vv + dv
        ok = cond(uu, vv) & (lu < w) & (lv < h)
        ok &= ~taken[np.minimum(lv, h - 1), np.minimum(lu, w - 1)]
        k = np.flatnonzero(ok)
        assert k.size, "no free target left"
        return int(uu[k[0]]), int(vv[k[0]])

    # interior variants: (name, condition on the base pixel, axis, offset of the target coordinate from the
    # base, where it lands relative to the base); border variants: (name, target coordinate, axis, None, the
    # landing coordinate or None if outside)
    variants = [
        ("tie_x_even_down", lambda u, v: u % 2 == 0, 0, 0.5, 0),
        ("tie_x_odd_up", lambda u, v: u % 2 == 1, 0, 0.5, 1),
        ("tie_y_even_down", lambda u, v: v % 2 == 0, 1, 0.5, 0),
        ("tie_y_odd_up", lambda u, v: v % 2 == 1, 1, 0.5, 1),
        ("left_tie_in", -0.5, 0, None, 0), ("left_in", -0.25, 0, None, 0), ("left_out", -0.75, 0, None, None),
        ("right_tie_out", w - 0.5, 0, None, None), ("right_in", w - 0.75, 0, None, w - 1),
        ("right_out", w - 0.25, 0, None, None), ("right_exact", w - 1.0, 0, None, w - 1),
        ("top_tie_in", -0.5, 1, None, 0), ("top_in", -0.25, 1, None, 0), ("top_out", -0.75, 1, None, None),
        ("bottom_tie_out", h - 0.5, 1, None, None), ("bottom_in", h - 0.75, 1, None, h - 1),
        ("bottom_out", h - 0.25, 1, None, None), ("bottom_exact", h - 1.0, 1, None, h - 1),
    ]
    if w > xe:
        variants.append(("beyond_floor_x", lambda u, v: u >= xe, 0, 0.0, 0))
    if h > ye:
        variants.append(("beyond_floor_y", lambda u, v: v >= ye, 1, 0.0, 0))
    for k, i in enumerate(probes):
        y, x = _yx(S, i)
        name, where, axis, off, res = variants[k % len(variants)]
        if callable(where):
            u0, v0 = alloc(where, res if axis == 0 else 0, res if axis == 1 else 0)
            tgt, land = [float(u0), float(v0)], [u0, v0]
            tgt[axis] += off
            land[axis] += res
        elif res is None:  # outside: the other coordinate is the source's own
            tgt, land = [float(x), float(y)], None
            tgt[axis] = where
        else:  # the other coordinate from a free pixel of the landing column / row
            u0, v0 = alloc((lambda u, v: u == res) if axis == 0 else (lambda u, v: v == res))
            tgt, land = [float(u0), float(v0)], [u0, v0]
            tgt[axis] = where
        vert = np.array([(f32(tgt[0]) - f32(I.cx)) / f32(I.fx), (f32(tgt[1]) - f32(I.cy)) / f32(I.fy), 1], f32)
        S.cur_v[y, x], S.cur_n[y, x] = vert, (0, 0, -1)
        if land is None:
            _tag(S, y, x, name, PROJ)
            continue
        lu, lv = land
        assert not taken[lv, lu]
        taken[lv, lu] = True
        S.pre_v[lv, lu], S.pre_n[lv, lu] = vert, (0, 0, -1)
        _tag(S, y, x, name, ACCEPT)
        if lu < xe and lv < ye:  # the source under the rewritten model pixel leaves at the first gate
            S.cur_n[lv, lu, 0] = np.nan
            _tag(S, lv, lu, "under_target", NAN)
    return _case(S)


def _find(s_of, want, cands):
    s = s_of(*cands)
    k = np.flatnonzero(s == want)
    assert k.size, "ladder rung not reachable"
    return k[0]


def gen_distance(I, dist_thr):
    """Class c: model offsets whose float32 |d|^2 is sqrt_le_bound(t) stepped by RUNGS ulps."""
    S = base_scene(I)
    bound = sqrt_le_bound(dist_thr)
    for k, i in enumerate(probe_pixels(S.npix, 42)):
        y, x = _yx(S, i)
        rung = RUNGS[k % len(RUNGS)]
        want = step(bound, rung)
        vc = S.cur_v[y, x]
        # z carries the bulk, x and y (finer ulps) the remainder
        uz, ux, uy = (np.spacing(np.nextafter(c, f32(0))) for c in (vc[2], abs(vc[0]), abs(vc[1])))
        nz = int(np.floor(np.sqrt(float(want)) / float(uz)))
        mz, mx = np.meshgrid(np.arange(nz - 7, nz + 1), np.arange(0, 512), indexing="ij")
        rem = float(want) - (mz * float(uz)) ** 2 - (mx * float(ux)) ** 2
        my = np.rint(np.sqrt(np.maximum(rem, 0)) / float(uy))
        cz, cxx, cy = (np.repeat(a[..., None], 5, -1) for a in (mz, mx, my))
        cy = cy + np.arange(-2, 3)
        sx, sy = (1 if vc[0] > 0 else -1), (1 if vc[1] > 0 else -1)  # towards zero: the differences stay exact
        pre = np.stack([vc[0] - f32(sx) * (cxx * float(ux)).astype(f32), vc[1] - f32(sy) * (cy * float(uy)).astype(f32),
                        vc[2] - (cz * float(uz)).astype(f32)], axis=-1).astype(f32).reshape(-1, 3)
        dd = vc[None, :] - pre
        hit = np.flatnonzero((_dot(dd, dd) == want) & (rem.repeat(5).reshape(-1) >= 0))
        assert hit.size, ("distance rung not reachable", dist_thr, rung)
        S.pre_v[y, x] = pre[hit[0]]
        _tag(S, y, x, f"rung{rung:+d}", ACCEPT if rung <= 0 else DIST)
    return _case(S, bound=bound, thr=f32(dist_thr))


def gen_angle(I, angle_thr):
    """Class d: model normals whose float32 |n_cur x n_model|^2 is sqrt_le_bound(sin) stepped by RUNGS ulps."""
    S = base_scene(I)
    bound = sqrt_le_bound(angle_thr)
    for k, i in enumerate(probe_pixels(S.npix, 42)):
        y, x = _yx(S, i)
        rung = RUNGS[k % len(RUNGS)]
        want = step(bound, rung)
        # n_cur = (0, 0, -1): the cross product is (n.y, -n.x, 0), its square n.y^2 + n.x^2
        nx = np.array([step(np.sqrt(want), -2 - d) for d in range(64)], f32)[:, None]
        ny0 = np.sqrt(np.maximum(float(want) - nx.astype(np.float64) ** 2, 0)).astype(f32)
        ny = np.concatenate([np.nextafter(ny0, f32(0)), ny0, np.nextafter(ny0, f32(1))], axis=1)
        nx = np.broadcast_to(nx, ny.shape)
        hit = np.argwhere(ny * ny + nx * nx == want)
        assert hit.size, ("angle rung not reachable", angle_thr, rung)
        nx, ny = nx[tuple(hit[k % len(hit)])], ny[tuple(hit[k % len(hit)])]
        sign = f32(-1 if k % 2 else 1)
        S.cur_n[y, x] = (0, 0, -1)
        S.pre_n[y, x] = (sign * nx, ny, -np.sqrt(f32(1) - want))
        _tag(S, y, x, f"rung{rung:+d}", ACCEPT if rung <= 0 else ANGLE)
    return _case(S, bound=bound, thr=f32(angle_thr))


def gen_fixed_point(I):
    """Class e: model normals (three of the seven row entries, identical current
    normals so the sine is exactly 0) whose products * 2^32 end in .5, .25 or
    .75, of both signs; entries near 2^-70 and 2^-63 (subnormal products, and the
    smallest normal ones); unit rows as control."""
    S = base_scene(I)
    variants = []
    for sa in (1, -1):
        for sb in (1, -1):
            for a, b, c in ((3, 5, 7), (5, 5, 3), (4095, 4093, 4091), (1, 1, 1), (7, 9, 11), (2049, 3, 1025)):
                variants.append((f"halves{sa:+d}{sb:+d}", (sa * a * 2.0 ** -16, sb * b * 2.0 ** -17, c * 2.0 ** -17)))
    for s in (1, -1):
        variants.append((f"subnormal{s:+d}", (s * 2.0 ** -70, 1.5 * 2.0 ** -70, -1.25 * 2.0 ** -72)))
        variants.append((f"edge_normal{s:+d}", (s * 1.5 * 2.0 ** -63, 1.5 * 2.0 ** -63, 2.0 ** -64)))
        variants.append((f"unit{s:+d}", (0.0, 0.0, float(s))))
        variants.append((f"unit_x{s:+d}", (float(s), 0.0, 0.0)))
    for k, i in enumerate(probe_pixels(S.npix, 900)):
        y, x = _yx(S, i)
        name, n = variants[k % len(variants)]
        S.cur_n[y, x] = S.pre_n[y, x] = np.array(n, f32)
        assert np.all(S.pre_n[y, x].astype(np.float64) == np.array(n))
        _tag(S, y, x, name, ACCEPT)
    return _case(S)


def gen_magnitude(zfar, slant=False, w=256, h=128):
    """Class f: a wall at depth zfar with a near strip, every vertex depth *
    ((u - cx) / fx, (v - cy) / fy, 1); model = current frame; the far normals lie
    in the x-z plane, perpendicular to the viewing ray (or 60 degrees off the
    optical axis with slant), which makes the (c_y, c_y) products as large as the
    geometry allows."""
    I = Intrinsics(w, h, 184.0, 184.0, 121.3, 63.5)
    u, v = np.meshgrid(np.arange(w, dtype=f32), np.arange(h, dtype=f32))
    near = (u >= 118) & (u <= 137)
    depth = np.where(near, f32(0.53) + f32(0.0013) * v, f32(zfar)).astype(f32)
    a = np.stack([(u - f32(I.cx)) / f32(I.fx), (v - f32(I.cy)) / f32(I.fy), np.ones_like(u)], axis=-1)
    vert = (a * depth[..., None]).astype(f32)
    if slant:
        far_n = np.broadcast_to(np.array([0.5, 0, -0.866], f32), vert.shape)
    else:
        nrm = np.sqrt(vert[..., 0] * vert[..., 0] + vert[..., 2] * vert[..., 2])
        far_n = np.stack([vert[..., 2] / nrm, np.zeros_like(nrm), -vert[..., 0] / nrm], axis=-1)
    n = np.where(near[..., None], np.array([0, 0, -1], f32), far_n).astype(f32)
    xe, ye = region(w, h)
    return SimpleNamespace(I=I, cur_v=vert, cur_n=n, pre_v=vert.copy(), pre_n=n.copy(),
                           label=np.zeros((ye, xe), np.int8), tag=None, tags=[], zfar=zfar)


def gen_degenerate(kind, I):
    """Systems the solve must refuse or barely accept: no, one, three or six
    correspondences; one, two or three planes."""
    S = base_scene(I)
    if kind in ("none", "one", "three", "six"):
        keep = {"none": 0, "one": 1, "three": 3, "six": 6}[kind]
        S.cur_n[..., 0] = np.nan
        S.label[:] = NAN
        for i in [5, 700, 1500, 2300, 3100, 4000][:keep]:
            y, x = _yx(S, i)
            S.cur_n[y, x] = S.pre_n[y, x]
            S.label[y, x] = ACCEPT
        return _case(S)
    w, h = S.w, S.h
    u, v = np.meshgrid(np.arange(w, dtype=f32), np.arange(h, dtype=f32))
    a = np.stack([(u - f32(I.cx)) / f32(I.fx), (v - f32(I.cy)) / f32(I.fy), np.ones_like(u)], axis=-1)
    inf = f32(np.inf)
    with np.errstate(all="ignore"):
        zs = [np.full((h, w), f32(2))]  # the wall z = 2 (normal (0, 0, -1))
        ns = [np.array([0, 0, -1], f32)]
        if kind in ("two_planes", "three_planes"):  # the wall x = 0.5
            zs.append(np.where(a[..., 0] > 0, f32(0.5) / a[..., 0], inf))
            ns.append(np.array([-1, 0, 0], f32))
        if kind == "three_planes":  # the floor y = 0.4
            zs.append(np.where(a[..., 1] > 0, f32(0.4) / a[..., 1], inf))
            ns.append(np.array([0, -1, 0], f32))
    which = np.argmin(np.stack(zs), axis=0)
    z = np.min(np.stack(zs), axis=0).astype(f32)
    S.cur_v = (a * z[..., None]).astype(f32)
    S.cur_n = np.stack(ns)[which]
    S.pre_n = S.cur_n.copy()
    S.pre_v = (S.cur_v + f32(2.0 ** -9) * S.cur_n).astype(f32)  # the model 2 mm behind, along the normal
    return _case(S)


# --------------------------------------------------------------------------
# the cases by name: (generator, distance threshold, angle in degrees)

def case_table():
    t3 = float(dist_thr_bound_above_square())
    return {
        "a_invalid": (gen_invalid, 0.015, 30.0),
        "b_projection": (gen_projection, 0.015, 30.0),
        "c_distance_15mm": (lambda I: gen_distance(I, 0.015), 0.015, 30.0),
        "c_distance_4mm": (lambda I: gen_distance(I, 0.004), 0.004, 30.0),
        "c_distance_bound_above_square": (lambda I: gen_distance(I, t3), t3, 30.0),
        "d_angle_30deg": (lambda I: gen_angle(I, sinf_deg(30.0)), 0.015, 30.0),
        "d_angle_8deg": (lambda I: gen_angle(I, sinf_deg(8.0)), 0.015, 8.0),
        "e_fixed_point": (gen_fixed_point, 0.015, 30.0),
    }


DEFAULT_THRESHOLD_CASES = ("a_invalid", "b_projection", "c_distance_15mm", "d_angle_30deg", "e_fixed_point")
_cache = {}


def crafted(name, w, h):
    """(case, distance threshold, angle threshold in degrees), built once per name and size."""
    key = (name, w, h)
    if key not in _cache:
        gen, dist, deg = case_table()[name]
        _cache[key] = (gen(crafted_intrinsics(w, h)), dist, deg)
    return _cache[key]
