"""One table of crafted raycast cases over ray space: exact-zero direction
components, origins on face planes and lattice points, the validity limit and
the occupancy words past bit 63 / 31, usable without a GPU.

test_ray_cases.py checks on the oracle alone that every case reaches what it is
named for (its MEASURED table); test_gpu_ray_space.py compares the five raycast
kernels (k_raycast plain / 64-bit index / slab, k_view, k_world_view) with the
same oracle results; ref_cases.py pins the oracle on them to the reference.
Pure numpy plus the oracle; nothing here touches the device library.

A case is a volume built analytically (no scene, no fusing), intrinsics, and
the ray frame given directly in volume coordinates: cam2vol = (R, org) and
Rinv = R^T.  The contexts' volume pose is the identity, so the camera pose of
kfx_render_view that gives the same cam2vol is cam2vol itself.

Volumes (V = 2^-6 m unless said; tsdf = rint(clip(sd / trunc, -1, 1) 32767),
weight 1 and a colour where |sd| <= 3 trunc, 0 / 0 elsewhere):

  sphere32  32^3, a sphere of radius 5.5 voxels about (15.3, 16.2, 15.6)
  blob64    64^3, 2 x 2 x 2 negative voxels inside a positive shell at voxels
            7 / 8 (a brick corner) and at 31 / 32 (a super-brick corner)
  shell32   32^3, a skin 1.5 voxels inside every face, positive towards the
            face, and a sphere of radius 4 voxels in the middle
  tall1040  16 x 16 x 1040 (3 brick words, 2 super-brick words along z), one
            sheet per case
  aniso52   24 x 40 x 52 at 13 / 11 / 17 mm, a tilted plane

Names: <volume>_<facing>[_<how the turn is written>]_<origin>.  Facing pz is
the identity; px, nx, py, ny, nz are the signed permutations written with
literal 0 and +-1, `cos` the same turn through cos / sin(pi / 2), `sub` the
turn with 2^-130 in place of the zeros, `obl` a generic rotation.

The normal of a hit is NaN only where the vertex lies within half a voxel of
the volume's faces.  The vertex lies one step before the last positive sample
(the reference's ray_len lags its sample), so with cubic voxels that happens
only where the sample before the positive one was not valid: at a surface
right behind the face a ray enters through.  From inside the volume every
hit lies between valid samples and its normal is finite: shell32's NaN-normal
resumes are therefore seen from outside, and shell32_pz_inside is named for the
-/+ stop at the last valid layer instead.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np

import oracle as O
from kfx.abi import Intrinsics, Pose, default_params

F = np.float32
V = 2.0 ** -6
SUB = 2.0 ** -130  # subnormal in float32

A = Intrinsics(64, 48, 64.0, 64.0, 32.0, 24.0)      # column 32 and row 24: exact zeros
N = Intrinsics(32, 32, 2048.0, 2048.0, 16.0, 16.0)  # tall1040's: column 16 and row 16
C = Intrinsics(64, 48, 64.0, 64.0, 31.5, 23.5)      # the control: no exact zero


# --------------------------------------------------------------------------
# volumes

def _finish(sd, trunc, dims):
    """(tsdf, weight, rgb flat u8x4) of a signed distance given on the (Z, Y, X) lattice."""
    X, Y, Z = dims
    band = np.abs(sd) <= 3 * trunc
    t = np.where(band, np.rint(np.clip(sd / trunc, -1, 1) * 32767), 0).astype(np.int16).ravel()
    w = band.astype(np.int16).ravel()
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    c = np.stack([(7 * x + 3 * y + 40) % 256, (11 * y + 5 * z + 90) % 256, (13 * z + 2 * x + 17) % 256,
                  np.zeros_like(x)], -1).astype(np.uint8)
    c[~band] = 0
    out = t, w, c.ravel()
    for a in out:
        a.setflags(write=False)
    return out


def _lattice(dims):
    X, Y, Z = dims
    return np.meshgrid(np.arange(Z, dtype=np.float64), np.arange(Y, dtype=np.float64),
                       np.arange(X, dtype=np.float64), indexing="ij")


def _box_sd(x, y, z, lo, hi):
    """Signed distance (voxels) to the box [lo, hi]^3, negative inside."""
    q = np.stack([np.maximum(lo - a, a - hi) for a in (x, y, z)], -1)
    return np.linalg.norm(np.maximum(q, 0), axis=-1) + np.minimum(q.max(-1), 0)


SPHERE_C, SPHERE_R = (15.3, 16.2, 15.6), 5.5
BLOBS = (7, 31)  # the blobs' lower voxel on every axis
# facing -z / +z.  519.5 and 503.5 put the first negative voxel in the second brick past a brick
# word's boundary in the direction of travel (bricks 65 and 62): the boundary brick's dilated bit is
# set while the word before it is clear to its end, so the clear run ends by the word's length
SHEETS_NEG = (508.5, 511.5, 512.5, 519.5, 1020.5, 1027.5, 1036.5)
SHEETS_POS = (3.5, 7.5, 8.5, 503.5, 511.5, 512.5, 519.5)
GEOM = {
    "sphere32": ((32, 32, 32), (0.5, 0.5, 0.5)),
    "blob64": ((64, 64, 64), (1.0, 1.0, 1.0)),
    "shell32": ((32, 32, 32), (0.5, 0.5, 0.5)),
    "tall1040": ((16, 16, 1040), (0.25, 0.25, 16.25)),
    "aniso52": ((24, 40, 52), (24 * 0.013, 40 * 0.011, 52 * 0.017)),
}
ANISO_N = np.array([0.5, 0.3, 0.81]) / np.linalg.norm([0.5, 0.3, 0.81])
ANISO_P0 = np.array([12 * 0.013, 20 * 0.011, 26 * 0.017])


@functools.lru_cache(maxsize=None)
def volume(key):
    """(tsdf, weight, rgb) of a volume key: a GEOM name, or ("tall1040", sheet, facing)."""
    name = key if isinstance(key, str) else key[0]
    dims = GEOM[name][0]
    z, y, x = _lattice(dims)
    if name == "sphere32":
        cx, cy, cz = SPHERE_C
        return _finish(np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) - SPHERE_R, 2.0, dims)
    if name == "blob64":
        sd = np.minimum(*[_box_sd(x, y, z, b, b + 1) - 0.5 for b in BLOBS])
        return _finish(sd, 2.0, dims)
    if name == "shell32":
        skin = _box_sd(x, y, z, 1.5, 29.5)  # positive outside the box, towards the faces
        ball = np.sqrt((x - 16.0) ** 2 + (y - 16.0) ** 2 + (z - 16.0) ** 2) - 4.0
        return _finish(np.where(np.abs(skin) <= 3.0, skin, ball), 1.0, dims)
    if name == "tall1040":
        _, sheet, facing = key
        return _finish((sheet - z) if facing < 0 else (z - sheet), 2.0, dims)
    if name == "aniso52":
        vs = np.array(GEOM[name][1]) / np.array(dims)
        sd = -((x * vs[0] - ANISO_P0[0]) * ANISO_N[0] + (y * vs[1] - ANISO_P0[1]) * ANISO_N[1] +
               (z * vs[2] - ANISO_P0[2]) * ANISO_N[2])
        return _finish(sd, 0.03, dims)
    raise KeyError(key)


# --------------------------------------------------------------------------
# rotations: rows give the volume axes in camera coordinates

ROT = {
    "pz": [[1, 0, 0], [0, 1, 0], [0, 0, 1]],
    "nz": [[-1, 0, 0], [0, 1, 0], [0, 0, -1]],
    "px": [[0, 0, 1], [1, 0, 0], [0, 1, 0]],     # column 0 -> dir.y == 0, row 0 -> dir.z == 0
    "nx": [[0, 0, -1], [-1, 0, 0], [0, 1, 0]],
    "py": [[0, 1, 0], [0, 0, 1], [1, 0, 0]],     # column 0 -> dir.z == 0, row 0 -> dir.x == 0
    "ny": [[0, 1, 0], [0, 0, -1], [-1, 0, 0]],
}


def _rot_y(a):
    c, s = math.cos(a), math.sin(a)
    return [[c, 0, s], [0, 1, 0], [-s, 0, c]]


def _rot_x(a):
    c, s = math.cos(a), math.sin(a)
    return [[1, 0, 0], [0, c, -s], [0, s, c]]


ROT["px_cos"] = _rot_y(math.pi / 2)    # faces +x; cos(pi / 2) = 6e-17 where px has zeros
ROT["py_cos"] = _rot_x(-math.pi / 2)   # faces +y
ROT["nx_cos"] = _rot_y(-math.pi / 2)   # faces -x
ROT["nz_cos"] = _rot_y(math.pi)        # faces -z; sin(pi) = 1.2e-16
ROT["px_sub"] = [[SUB, -SUB, 1], [1, SUB, -SUB], [-SUB, 1, SUB]]
ROT["pz_sub"] = [[1, SUB, -SUB], [-SUB, 1, SUB], [SUB, -SUB, 1]]
ROT["obl"] = (np.array(_rot_y(0.5)) @ np.array(_rot_x(-0.3))).tolist()
for _k, _r in ROT.items():
    assert abs(np.linalg.det(np.array(_r, np.float64)) - 1.0) < 1e-6, _k


def facing(rot):
    """The camera's viewing direction in the volume: R's third column."""
    return np.array(ROT[rot], np.float64)[:, 2]


# --------------------------------------------------------------------------
# the table

CASES = {}


def _case(name, vol, rot, org, intr=A, unit=V):
    """org in voxels of `unit` metres (exact in float32 for the dyadic lattice)."""
    vname = vol if isinstance(vol, str) else vol[0]
    dims, rng = GEOM[vname]
    m = np.eye(4)
    m[:3, :3] = np.array(ROT[rot], np.float64)
    m[:3, 3] = [float(o) * unit for o in org]
    cam2vol = Pose.from_matrix(m)
    R = np.array(cam2vol.R[:], F).reshape(3, 3)
    p = default_params(dims=64, range_m=1.0)
    for i in range(3):
        p.volu_dims[i] = int(dims[i])
        p.volu_range[i] = float(rng[i])
    p.volu_pose = Pose.identity()
    CASES[name] = SimpleNamespace(name=name, vol=vol, vname=vname, dims=tuple(dims), range=tuple(rng), intr=intr,
                                  rot=rot, cam2vol=cam2vol, Rinv=np.ascontiguousarray(R.T).reshape(9), params=p,
                                  pose=cam2vol.matrix())


# sphere32, facing +z from 8 voxels in front: the zero column's x and the zero row's y at k + 0.5
_case("sphere32_pz_tie_even", "sphere32", "pz", (14.5, 16.5, -8))   # rintf ties to 14 and 16
_case("sphere32_pz_tie_odd", "sphere32", "pz", (15.5, 17.5, -8))    # ties to 16 and 18
_case("sphere32_pz_lattice", "sphere32", "pz", (15, 16, -8))        # on the trilinear cell boundary
_case("sphere32_pz_control", "sphere32", "pz", (15, 16, -8), intr=C)
_case("sphere32_pz_x0", "sphere32", "pz", (0, 16.5, -16))           # org.x == 0: tbot.x = inf 0 in the zero column
_case("sphere32_pz_xrange", "sphere32", "pz", (32, 16.5, -16))      # org.x == range: ttop.x = inf 0
_case("sphere32_nz_farface", "sphere32", "nz", (15.5, 16, 32))      # on the far face, looking back in
_case("sphere32_pz_inside", "sphere32", "pz", (15.5, 16, 4))        # tnear < 0
_case("sphere32_px_tie", "sphere32", "px", (-8, 16.5, 15.5))        # dir.y == 0 column, dir.z == 0 row
_case("sphere32_nx_lattice", "sphere32", "nx", (40, 16, 15))
_case("sphere32_py_tie", "sphere32", "py", (15.5, -8, 16.5))        # dir.z == 0 column, dir.x == 0 row
_case("sphere32_ny_lattice", "sphere32", "ny", (15, 40, 16))
_case("sphere32_px_cos", "sphere32", "px_cos", (-8, 16.5, 15.5))
_case("sphere32_py_cos", "sphere32", "py_cos", (15.5, -8, 16.5))
_case("sphere32_nz_cos", "sphere32", "nz_cos", (15.5, 16.5, 40))
_case("sphere32_px_sub", "sphere32", "px_sub", (-8, 16.5, 15.5))
_case("sphere32_pz_sub", "sphere32", "pz_sub", (15.5, 16.5, -8))
_case("sphere32_obl", "sphere32", "obl", tuple(np.array(SPHERE_C) - 22 * facing("obl")))
_case("sphere32_px_plane_z0", "sphere32", "px", (-40, 16.5, 0))     # the dir.z == 0 row runs in the z = 0 face
_case("sphere32_px_plane_zrange", "sphere32", "px", (-40, 16.5, 32))
_case("sphere32_pz_corner", "sphere32", "pz", (28, 16.5, -16))      # column 48 meets the edge x = range, z = 0
_case("sphere32_pz_behind", "sphere32", "pz", (15, 16, 40))         # the volume wholly behind the camera

# blob64: the camera close, so that a 2-voxel blob covers some 16 pixels
_case("blob64_pz_corner8", "blob64", "pz", (7.5, 8.5, -6))
_case("blob64_px_corner8", "blob64", "px", (-6, 7.5, 8))
_case("blob64_obl_corner8", "blob64", "obl", tuple(np.array([8.0, 8.0, 8.0]) - 14 * facing("obl")))
_case("blob64_pz_corner32_inside", "blob64", "pz", (31.5, 32, 20))
_case("blob64_ny_corner32_inside", "blob64", "ny", (31.5, 44, 32.5))
_case("blob64_nx_cos_corner32_inside", "blob64", "nx_cos", (45, 31.5, 32))
_case("blob64_obl_corner32_inside", "blob64", "obl", tuple(np.array([32.0, 32.0, 32.0]) - 12 * facing("obl")))

# shell32
_case("shell32_pz_outside", "shell32", "pz", (15.5, 16, -8))
_case("shell32_nx_cos_outside", "shell32", "nx_cos", (40, 16.5, 15.5))
_case("shell32_pz_inside", "shell32", "pz", (16, 16.5, 5.5))

# aniso52 (origins in metres)
_case("aniso52_pz", "aniso52", "pz", (0.156, 0.22, -0.25), unit=1.0)
_case("aniso52_px", "aniso52", "px", (-0.25, 0.22, 0.442), unit=1.0)
_case("aniso52_obl", "aniso52", "obl", tuple(ANISO_P0 - 0.45 * facing("obl")), unit=1.0)

# tall1040: from 0.5 m outside either z end, on the axis of the 16 x 16 section
for _s in SHEETS_NEG:
    _case(f"tall1040_pz_{_s}", ("tall1040", _s, -1), "pz", (8, 8, -32), intr=N)
for _s in SHEETS_POS:
    _case(f"tall1040_nz_{_s}", ("tall1040", _s, +1), "nz", (8, 8, 1040 + 32), intr=N)
# and from inside
_case("tall1040_pz_inside_1020.5", ("tall1040", 1020.5, -1), "pz", (8, 8.5, 516), intr=N)
_case("tall1040_nz_inside_519.5", ("tall1040", 519.5, +1), "nz", (8.5, 8, 700), intr=N)
_case("tall1040_nz_inside_512.5", ("tall1040", 512.5, +1), "nz", (7.5, 8.5, 1030), intr=N)

AXIS_ALIGNED_BOX = tuple(n for n, c in CASES.items() if c.vname in ("sphere32", "blob64") and
                         c.rot in ("pz", "nz", "px", "nx", "py", "ny"))


def records(case):
    """The reference's 8-byte voxel records of the case's volume (what upload_tsdf takes)."""
    t, w, c = volume(case.vol)
    rec = np.zeros(t.size, dtype=np.dtype([("tsdf", "<i2"), ("weight", "<i2"), ("rgb", "u1", 3), ("pad", "u1")]))
    rec["tsdf"], rec["weight"] = t, w
    rec["rgb"] = c.reshape(-1, 4)[:, :3]
    return rec


# --------------------------------------------------------------------------
# oracle side

@functools.lru_cache(maxsize=None)
def expected(name):
    """The oracle's results of a case, computed once and shared read-only: dict of
    maps = [(vmap, nmap)] of levels 0..2, ts (H, W), normal (the renderNormals image)."""
    case = CASES[name]
    t, _, _ = volume(case.vol)
    vol = O.Volume(case.dims, case.range)
    vol.tsdf[:] = t
    v, n = O.raycast(vol, case.intr, case.cam2vol, case.Rinv)
    Z = case.dims[2]
    _, sv, sn, ts = O.raycast_slab(t, vol, case.intr, case.cam2vol, case.Rinv, 0, Z, 0, Z)
    maps = [(v, n)]
    for _ in (1, 2):
        maps.append(O.resize_points_normals(*maps[-1]))
    out = dict(maps=maps, ts=ts, slab_maps=(sv, sn), normal=O.render(v, n, case.pose[:3, 3], "normal"))
    for a in [ts, sv, sn, out["normal"]] + [x for m in maps for x in m]:
        a.setflags(write=False)
    return out


def hit_mask(nmap):
    return (nmap != 0).any(-1) & ~np.isnan(nmap).any(-1)


# --------------------------------------------------------------------------
# the rays, restated in float32 numpy in the oracle's written order

def rays(case):
    """dir (3 x (H, W)), org, and the prologue's tbot, ttop, ray0, tfar, all float32;
    fmin / fmax drop a NaN operand as C's do."""
    I = case.intr
    R = np.array(case.cam2vol.R[:], F)
    org = np.array(case.cam2vol.t[:], F)
    rng = np.array(case.range, F)
    x = np.arange(I.width, dtype=F)[None, :]
    y = np.arange(I.height, dtype=F)[:, None]
    p0 = np.broadcast_to((F(1) * (x - F(I.cx))) / F(I.fx), (I.height, I.width))
    p1 = np.broadcast_to((F(1) * (y - F(I.cy))) / F(I.fy), (I.height, I.width))
    v = [R[3 * i] * p0 + R[3 * i + 1] * p1 + R[3 * i + 2] * F(1) for i in range(3)]
    nrm = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    d = [(v[i] / nrm).astype(F) for i in range(3)]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = [F(1) / d[i] for i in range(3)]
        tb = [inv[i] * (F(0) - org[i]) for i in range(3)]
        tt = [inv[i] * (rng[i] - org[i]) for i in range(3)]
        tmin = [np.fmin(tt[i], tb[i]) for i in range(3)]
        tmax = [np.fmax(tt[i], tb[i]) for i in range(3)]
        tnear = np.fmax(np.fmax(tmin[0], tmin[1]), np.fmax(tmin[0], tmin[2]))
        tfar = np.fmin(np.fmin(tmax[0], tmax[1]), np.fmin(tmax[0], tmax[2]))
        ray0 = np.fmax(tnear, F(0))
    assert all(a.dtype == F for a in d + tb + tt + [ray0, tfar])
    return SimpleNamespace(d=d, org=org, tb=tb, tt=tt, ray0=ray0, tfar=tfar)


def march(case, r=None):
    """The reference's sample loop up to each ray's first +/- candidate.  Returns
    cand_len (the loop's ray_len at the candidate, 0: none: a hit made of that
    candidate has Ts in [cand_len - step, cand_len], a later or missing hit means
    that its normal was NaN and the march went on), prev (the voxel of the
    sample before the candidate, (H, W, 3) int) and stop (the ray ended at a
    -/+ event, with the voxel of that event's sample in stop_vox).  Used only
    to show what a case reaches, never as a reference."""
    r = r or rays(case)
    I = case.intr
    H, W = I.height, I.width
    dims = np.array(case.dims, np.int64)
    vs = (np.array(case.range, F) / dims.astype(F)).astype(F)
    vinv = [F(1) / vs[i] for i in range(3)]
    t = volume(case.vol)[0].reshape(case.dims[2], case.dims[1], case.dims[0])
    step = vs[0]
    with np.errstate(invalid="ignore", over="ignore"):
        live = r.ray0 < r.tfar
        ray_len = (r.ray0 + step).astype(F)
        ray_len = np.where(live, ray_len, F(0))
        nextp = [(r.org[i] + r.d[i] * ray_len).astype(F) for i in range(3)]
        vstep = [(r.d[i] * vs[i]).astype(F) for i in range(3)]

        def read(pp):
            g = [np.rint(pp[i] * vinv[i]) for i in range(3)]
            ok = np.ones((H, W), bool)
            for i in range(3):
                ok &= (g[i] >= 1) & (g[i] <= dims[i] - 2)
            gi = [np.where(ok, g[i], 1).astype(np.int64) for i in range(3)]
            return np.sign(np.where(ok, t[gi[2], gi[1], gi[0]], 0).astype(np.int64)), np.stack(gi, -1), ok

        sprev, gprev, _ = read(nextp)
        cand_len = np.zeros((H, W), F)
        prev = np.zeros((H, W, 3), np.int64)
        stop = np.zeros((H, W), bool)
        stop_vox = np.zeros((H, W, 3), np.int64)
        for _ in range(4 * int(dims.max()) + 64):
            live = live & (ray_len < r.tfar)
            if not live.any():
                break
            nextp = [(nextp[i] + vstep[i]).astype(F) for i in range(3)]
            s, g, ok = read(nextp)
            hit = live & (sprev > 0) & (s < 0)
            end = live & (sprev < 0) & (s > 0)
            cand_len = np.where(hit, ray_len, cand_len)
            prev = np.where(hit[..., None], gprev, prev)
            stop |= end
            stop_vox = np.where(end[..., None], g, stop_vox)
            live = live & ~hit & ~end
            sprev = np.where(ok, s, 0)  # an invalid sample is NaN: no event on either side of it
            gprev = g
            ray_len = (ray_len + step).astype(F)
    return SimpleNamespace(cand_len=cand_len, prev=prev, stop=stop, stop_vox=stop_vox)


def populations(name):
    """The measured classes of a case: dict of pixel counts."""
    case = CASES[name]
    e = expected(name)
    r = rays(case)
    m = march(case, r)
    hit = hit_mask(e["maps"][0][1])
    zero = [r.d[i] == 0 for i in range(3)]
    anyzero = zero[0] | zero[1] | zero[2]
    with np.errstate(invalid="ignore"):
        crossing = r.ray0 < r.tfar
        graze = (r.ray0 == r.tfar) & np.isfinite(r.tfar) & (r.ray0 > 0)
    nanpro = np.zeros(hit.shape, bool)
    for a in r.tb + r.tt:
        nanpro |= np.isnan(a)
    tiny = F(2.0 ** -126)
    sub = np.zeros(hit.shape, bool)
    small = np.zeros(hit.shape, bool)  # normal, but below 2^-40: cos(pi / 2) and its like
    for d in r.d:
        sub |= (d != 0) & (np.abs(d) < tiny)
        small |= (np.abs(d) >= tiny) & (np.abs(d) < F(2.0 ** -40))
    cand = m.cand_len > 0
    ts = e["ts"]
    resumed = cand & ((ts == 0) | (ts > m.cand_len))
    first = hit & cand & ~resumed
    out = dict(hits=int(hit.sum()), zx_hit=int((hit & zero[0]).sum()), zy_hit=int((hit & zero[1]).sum()),
               zz_hit=int((hit & zero[2]).sum()), zero_miss=int((anyzero & crossing & ~hit).sum()),
               zero_pixels=int(anyzero.sum()), crossing=int(crossing.sum()), nan_prologue=int(nanpro.sum()),
               graze=int(graze.sum()), subnormal=int(sub.sum()), tiny=int(small.sum()),
               tiny_hit=int((small & hit).sum()), resumed=int(resumed.sum()),
               resumed_hit=int((resumed & hit).sum()), stop=int(m.stop.sum()))
    out["_first"], out["_prev"], out["_stop"], out["_stop_vox"] = first, m.prev, m.stop, m.stop_vox
    return out


def prev_in(pop, axis, lo, hi):
    """Hits made of the first candidate whose sample before the event has voxel[axis] in [lo, hi]."""
    g = pop["_prev"][..., axis]
    return int((pop["_first"] & (g >= lo) & (g <= hi)).sum())


# --------------------------------------------------------------------------
# the world view's inputs (world_view_cases.py's machinery, imported on use)

def window_bricks(case):
    """The case's volume as the world_bricks() of a context that holds it at origin 0."""
    import stream_cases as ST
    import world_cases as WC
    t, w, c = volume(case.vol)
    return WC.bricks_of(t, w, c.reshape(-1, 4)[:, :3], case.dims, ST.nonempty_bricks(t, w, c, case.dims))


def tight_box(case):
    """(origin, dims): the window cut on lattice planes one brick inside every face."""
    return (8, 8, 8), tuple(d - 16 for d in case.dims)


@functools.lru_cache(maxsize=None)
def box_reference(name):
    """world_view_cases.reference of an AXIS_ALIGNED_BOX case on its tight box: the oracle's
    raycast on the dense assembly of the window's bricks cut to the box."""
    import world_view_cases as W
    case = CASES[name]
    return W.reference(case.params, window_bricks(case), case.intr, case.pose, box=tight_box(case))
