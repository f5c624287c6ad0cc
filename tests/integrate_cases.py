"""One table of integrate cases over volume geometry, poses and arithmetic
paths, with the oracle's result for each, usable without a GPU.

test_integrate_cases.py checks on the oracle alone that every case reaches
what it is meant to reach (the populations below); test_gpu_integrate_space.py
compares k_integrate with the same oracle results.  Pure numpy plus the
oracle; nothing here touches the device library.

Frame: frame 0 of the noisy 160x120 synthetic sequence, camera at identity,
preprocessed with the default filter parameters, unless a case brings its own
(the wide-angle cases).  The volume is placed by an explicit vol2cam per launch
(the stage seam's pose), so a case is a volume geometry, a truncation distance
and a list of poses integrated one after another into one volume.

Notation: L = 2.048, vs = L / 64, T() a translation; C = T(0, 0, 0.5 + L/2) and
O0 = T(-L/2, -L/2, -L/2), so C @ Rot @ O0 turns the default volume about its
centre.  Exact matrices are written with literal 0 / +-1 entries; the *_cos
case goes through cos(pi/2) on purpose (6e-17 as a float).

What each case reaches in k_integrate (csrc/kfx_kernels.hip):

  base            control: the default placement
  axis_x, axis_y  sz == 0 exactly: the beta == 0 arm of clip_lin for the
                  vc.z > 0 and far clips; columns wholly beyond the far clip
  axis_x_behind   the same about a centre 0.3 m from the camera: columns wholly
                  behind the camera beside columns in front of it
  axis_x_cos      zs.z ~ 2e-18: every wave takes the IEEE loop (column_fast's
                  exponent test), rcp(beta) overflows in the clips
  reversed(_gen)  sz < 0: the clips' branches the other way round
  oblique         all three zs components comparable
  inside          the camera inside the volume; vc.z crosses 0 inside columns
  plane           vs = 2^-5, all sums exact: vc.z == 0 exactly on slice 8 and
                  vc.x == 0 exactly on column 32, in the fast loop (rcp of 0)
  tilt_1e-6       zs.x = 3.2e-8: the IEEE loop on an otherwise ordinary frame
  mixed           column 5 has vc0.x ~ 1e-7: slow and fast waves in one launch
  behind, beside, far   empty intervals everywhere
  trunc_big/tiny  a colour band as wide as the scene / thinner than a voxel
  aniso(_oblique) vs[1] != vs[0] != vs[2] under the reference's voxel_size.x z
                  step, tiles_x != tiles_y, Z % 8 == 4
  odd             Z = 13: batch and brick tails past the last slice (the
                  z + j <= lb guard), a single tile row
  deep1500        1024 <= Z < 2048: length-capped chunks, surplus items
                  (3 of 4 chunks used), k_int_order rewriting the order between
                  launches (poses A, B, A in one context), Z % 8 == 4
  deep1030        the first Z of that range with a 6-slice tail; 4 capped
                  chunks, one of which starts past 768 slices: the ff_add
                  fast-forward of the chunk-start replay (deep1500's three
                  chunks all start below it)
  deep2056        Z >= 2048: geometric chunks again, 8 of them, the
                  fast-forward on most
  deep_coarse     deep, with tiles whose interval lengths differ widely
  slab300         Z-slab contexts (rank 1 of 2 stores from slice 140: its
                  chunk-start replays take the slab fast-forward)
  wide_angle*     fx ~ 10 px: the far clip and occlusion clip under pixels so
                  coarse that half a pixel changes lambda by several per cent;
                  _inf: fx = 1.4 px, where no far bound holds at all
"""
import functools
import math
from types import SimpleNamespace

import numpy as np

import oracle as O
from kfx import synth
from kfx.abi import Intrinsics, Pose, default_params

f32 = np.float32
L = 2.048
VS = L / 64


# --------------------------------------------------------------------------
# poses

def T(x, y, z):
    m = np.eye(4)
    m[:3, 3] = [x, y, z]
    return m


def _h(R):
    m = np.eye(4)
    m[:3, :3] = R
    return m


def rot_x(a):
    c, s = math.cos(a), math.sin(a)
    return _h([[1, 0, 0], [0, c, -s], [0, s, c]])


def rot_y(a):
    c, s = math.cos(a), math.sin(a)
    return _h([[c, 0, s], [0, 1, 0], [-s, 0, c]])


C0 = T(0, 0, 0.5 + L / 2)
O0 = T(-L / 2, -L / 2, -L / 2)
P_ZX = _h([[0, 0, 1], [0, 1, 0], [-1, 0, 0]])   # e_z -> e_x, exact (columns [0,0,-1], [0,1,0], [1,0,0])
P_ZY = _h([[1, 0, 0], [0, 0, 1], [0, -1, 0]])   # e_z -> e_y, exact
P_REV = _h(np.diag([-1.0, 1.0, -1.0]))          # half a turn about y, exact


# --------------------------------------------------------------------------
# frames

QQVGA = Intrinsics(160, 120, 131.25, 131.25, 79.5, 59.5)
WIDE24 = Intrinsics(24, 16, 9.6, 9.6, 11.5, 7.5)
WIDE32 = Intrinsics(32, 32, 12.8, 12.8, 15.5, 15.5)
WIDE16 = Intrinsics(16, 16, 1.4, 1.4, 7.5, 7.5)  # hypot(1/fx, 1/fy) / 2 = 0.505: no far bound holds


def _wall(I, depth_mm):
    """A flat wall at depth_mm +- 2 mm, and a colour ramp."""
    rng = np.random.default_rng(3)
    d = (depth_mm + rng.uniform(-2.0, 2.0, (I.height, I.width))).astype(f32)
    y, x = np.mgrid[0:I.height, 0:I.width]
    bgr = np.stack([40 + 5 * x, 30 + 9 * y, 200 - 3 * x - 2 * y], -1).astype(np.uint8)
    return bgr, d


@functools.lru_cache(maxsize=None)
def frame(key):
    """(bgr u8, depth f32 mm) of a frame key, rendered once."""
    if key == "qqvga":
        bgr, dep, _ = synth.sequence(2, synth.Intrinsics.qqvga(), noise=True, dropout=0.01)
        out = bgr[0].copy(), dep[0].astype(f32)
    elif key == "qqvga_full":  # the same without dropouts: every pixel has depth
        bgr, dep, _ = synth.sequence(2, synth.Intrinsics.qqvga(), noise=True, dropout=0.0)
        out = bgr[0].copy(), dep[0].astype(f32)
    elif key == "wide24":
        out = _wall(WIDE24, 4000.0)
    elif key == "wide32":
        out = _wall(WIDE32, 4900.0)
    elif key == "wide16":
        out = _wall(WIDE16, 1000.0)
    else:
        raise KeyError(key)
    for a in out:
        a.setflags(write=False)
    return out


# --------------------------------------------------------------------------
# the table

def _params(dims, rng, trunc, **kw):
    p = default_params(dims=64, range_m=L)
    for i in range(3):
        p.volu_dims[i] = int(dims[i])
        p.volu_range[i] = float(rng[i])
    p.volu_trun_dist = float(f32(2.1) * f32(rng[0]) / f32(dims[0])) if trunc is None else float(trunc)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


CASES = {}


def _case(name, poses, dims=(64, 64, 64), rng=(L, L, L), trunc=None, intr=QQVGA, frame_key="qqvga", **kw):
    CASES[name] = SimpleNamespace(name=name, intr=intr, frame=frame_key, dims=tuple(dims), range=tuple(rng),
                                  params=_params(dims, rng, trunc, **kw),
                                  poses=[Pose.from_matrix(m) for m in poses])


BASE = T(-L / 2, -L / 2, 0.5)
OBLIQUE = C0 @ rot_y(1.1) @ rot_x(-0.5) @ O0

_case("base", [BASE])
_case("axis_x", [C0 @ P_ZX @ O0])
_case("axis_x_behind", [T(0, 0, 0.3) @ P_ZX @ O0])
_case("axis_x_cos", [C0 @ rot_y(math.pi / 2) @ O0])
_case("axis_y", [C0 @ P_ZY @ O0])
_case("reversed", [C0 @ P_REV @ O0])
_case("reversed_gen", [C0 @ rot_y(math.pi - 0.2) @ rot_x(0.15) @ O0])
_case("oblique", [OBLIQUE])
_case("inside", [rot_x(0.3) @ rot_y(-0.4) @ T(-L / 2, -L / 2, -0.4)])
_case("plane", [T(-1, -1, -0.25)], rng=(2.0, 2.0, 2.0))
_case("tilt_1e-6", [BASE @ rot_y(1e-6)])
_case("mixed", [T(float(f32(f32(-5 * f32(VS)) + f32(1e-7))), -L / 2, 0.5)])
_case("behind", [T(-L / 2, -L / 2, -3)])
_case("beside", [T(4, -L / 2, 0.5)])
_case("far", [T(-L / 2, -L / 2, 6)])
_case("trunc_big", [BASE], trunc=0.5)
_case("trunc_tiny", [BASE], trunc=VS / 4)
_case("aniso", [BASE], dims=(64, 40, 100))
_case("aniso_oblique", [OBLIQUE], dims=(64, 40, 100))
_case("odd", [T(-0.384, -0.128, 0.9), T(0.2, -0.128, 1.1) @ rot_y(-0.6)], dims=(24, 8, 13),
      rng=(0.768, 0.256, 1.0), trunc=0.0672)
_DEEP_A, _DEEP_B = T(-0.016, -0.024, 0.4), T(0.3, -0.024, 0.6) @ rot_y(-0.35)
_case("deep1500", [_DEEP_A, _DEEP_B, _DEEP_A], dims=(16, 24, 1500), rng=(0.032, 0.048, 1.0), trunc=0.0042)
_case("deep1030", [_DEEP_A, _DEEP_B, _DEEP_A], dims=(16, 16, 1030), rng=(0.032, 0.032, 1.0), trunc=0.0042)
_case("deep2056", [_DEEP_A, _DEEP_B], dims=(16, 24, 2056), rng=(0.032, 0.048, 1.0), trunc=0.0042)
# 16 mm pitch in x and y, so a 16 mm z step: 24 m deep.  The volume lies right
# of the optical axis, from 0.5 m to 1.5 m: its left columns enter the frustum
# 0.8 m from the camera, the ones further right ever later, the last just
# before the back wall.
_COARSE_A, _COARSE_B = T(0.5, -0.192, 0.3), T(0.2, -0.192, 0.35) @ rot_y(-0.25)
_case("deep_coarse", [_COARSE_A, _COARSE_B, _COARSE_A], dims=(64, 24, 1500), rng=(1.024, 0.384, 1.0))
_case("slab300", [T(-0.064, -0.096, 0.9), T(0.5, -0.096, 1.2) @ rot_y(-0.5)], dims=(16, 24, 300),
      rng=(0.128, 0.192, 1.0), trunc=0.0168)
# the volume just inside the right image edge at the wall's depth
_case("wide_angle", [T(11.5 / 9.6 * 4 - 0.128, -0.064, 3.9)], dims=(64, 64, 256), rng=(0.128, 0.128, 0.512),
      trunc=2.1 * 0.002, intr=WIDE24, frame_key="wide24", pyramid_height=1, bfilter_kernel_size=1)
# (here at the image corner: the diagonal half pixel is what exceeds the 2 % at fx = 12.8)
_case("wide_angle_32", [T(15.5 / 12.8 * 4.9 - 0.064, 15.5 / 12.8 * 4.9 - 0.064, 4.8)], dims=(64, 64, 256), rng=(0.064, 0.064, 0.256),
      trunc=2.1 * 0.001, intr=WIDE32, frame_key="wide32", pyramid_height=1, bfilter_kernel_size=1)
# a camera so coarse that delta >= 0.5 (far_clip_factor = +inf: no far clip, no certificate): the
# pixels' rays are 12 % longer than the voxels', so voxels 0.13 m behind the wall are still updated
_case("wide_angle_inf", [T(-0.064, -0.064, 0.7)], dims=(16, 16, 64), rng=(0.128, 0.128, 0.512), trunc=2.1 * 0.008,
      intr=WIDE16, frame_key="wide16", pyramid_height=1, bfilter_kernel_size=1, dfilter_dist=2.0)

EMPTY = ("behind", "beside", "far")
SEQUENCES = tuple(n for n, c in CASES.items() if len(c.poses) > 1)

# Floors of the oracle's populations on a zeroed volume, per launch: (updated,
# coloured, negative tsdf), about half of what the oracle measured when the
# table was written (the figures in the comment); None: not asserted.
FLOORS = {
    "base": [(48000, 3800, 3700)],             # 97270 / 7602 / 7410
    "axis_x": [(48000, 3800, 3600)],           # 97340 / 7601 / 7354
    "axis_x_behind": [(13000, 190, None)],     # 26277 / 392
    "axis_x_cos": [(48000, 3800, None)],       # 97340 / 7601
    "axis_y": [(48000, 3700, None)],           # 97046 / 7482
    "reversed": [(49000, 3800, None)],         # 98465 / 7732
    "reversed_gen": [(47000, 3300, None)],     # 94960 / 6730
    "oblique": [(46000, 3100, None)],          # 93622 / 6290
    "inside": [(19000, 390, None)],            # 39896 / 784
    "plane": [(27000, 800, 750)],              # 55310 / 1694 / 1511
    "tilt_1e-6": [(48000, 3800, None)],        # 97255 / 7601
    "mixed": [(34000, 2700, None)],            # 69125 / 5426
    "trunc_big": [(63000, 25000, None)],       # 126394 / 51748
    "trunc_tiny": [(45000, 290, None)],        # 90820 / 585
    "aniso": [(30000, 2300, None)],            # 60898 / 4750
    "aniso_oblique": [(31000, 2300, None)],    # 62962 / 4697
    "odd": [(1100, None, None), (1100, None, None)],  # 2291 / 18, 2209 / 74 (the issue's floor: >= 500)
    "deep1500": [(180000, 390, None), (170000, 410, None), (180000, 390, None)],  # 373309 / 787, 351874 / 834
    "deep1030": [(120000, None, None), (110000, None, None), (120000, None, None)],  # 248815, 234122
    "deep2056": [(180000, None, None), (170000, None, None)],  # 373309, 351874
    "deep_coarse": [(31000, 1200, None), (62000, 1600, None), (31000, 1200, None)],  # 62451 / 2533, 125951 / 3248
    "slab300": [(34000, 400, None), (28000, 770, None)],  # 69440 / 814, 57499 / 1542
    "wide_angle": [(176000, None, None)],      # 352248
    "wide_angle_32": [(380000, None, None)],   # 763428
    "wide_angle_inf": [(6900, None, None)],    # 13864
}


# --------------------------------------------------------------------------
# oracle side

def new_volume(case, init=None):
    vol = O.Volume(case.dims, case.range)
    if init is not None:
        vol.tsdf[:], vol.weight[:], vol.rgb[:] = init
    return vol


@functools.lru_cache(maxsize=None)
def depth_maps(frame_key):
    """The oracle's level-0 depth map (m) of a frame; preprocess depends on the
    filter parameters only, which the cases of one frame share."""
    case = next(c for c in CASES.values() if c.frame == frame_key.replace("_full", ""))
    _, d = frame(frame_key)
    ds, _, _ = O.preprocess(d, case.intr, case.params)
    ds[0].setflags(write=False)
    return ds[0]


def integrate_steps(case, init=None):
    """The oracle's result after each pose of the case, integrated in turn into
    one volume that starts zeroed or from init = (tsdf, weight, rgb): a list of
    ((updated, coloured), tsdf, weight, rgb), and the final O.Volume."""
    bgr, _ = frame(case.frame)
    d0 = depth_maps(case.frame)
    vol = new_volume(case, init)
    out = []
    for pose in case.poses:
        counts = O.integrate(vol, case.params.volu_trun_dist, case.intr, pose, d0, bgr)
        out.append((counts, vol.tsdf.copy(), vol.weight.copy(), vol.rgb.copy()))
    return out, vol


@functools.lru_cache(maxsize=None)
def oracle_zeroed(name):
    """integrate_steps of a case from the zeroed volume, computed once and shared read-only."""
    steps, vol = integrate_steps(CASES[name])
    for _, t, w, c in steps:
        for a in (t, w, c):
            a.setflags(write=False)
    for a in (vol.tsdf, vol.weight, vol.rgb):
        a.setflags(write=False)
    return steps, vol


def raycast_levels(case, vol, pose):
    """(cam2vol, Rinv, [(vmap, nmap) per pyramid level]) of the oracle's raycast from the pose's camera."""
    cam2vol = O.pose_inv(pose)
    Rinv = cam2vol.matrix()[:3, :3].T.copy()
    maps = [O.raycast(vol, case.intr, cam2vol, Rinv)]
    for _ in range(1, case.params.pyramid_height):
        maps.append(O.resize_points_normals(*maps[-1]))
    return cam2vol, Rinv, maps


def records(t, w, c):
    """The reference's 8-byte voxel records of SoA arrays (what upload_tsdf takes)."""
    rec = np.zeros(t.size, dtype=np.dtype([("tsdf", "<i2"), ("weight", "<i2"), ("rgb", "u1", 3), ("pad", "u1")]))
    rec["tsdf"], rec["weight"] = t, w
    rec["rgb"] = c.reshape(-1, 4)[:, :3]
    return rec


def tsat():
    """T*: the tsdf fixed point of a weight-64, ts = 1 update (test_gpu_regimes.tsat)."""
    t = 32767
    for _ in range(64):
        pre = f32(t) * f32(0.0000305185)
        new = (pre * f32(64) + f32(1)) / f32(65)
        q = max(-32767, min(32767, int(f32(new) * f32(32767))))
        if q == t:
            return t
        t = q
    raise AssertionError("no fixed point")


@functools.lru_cache(maxsize=None)
def random_volume(dims, seed=5):
    """An uploaded volume in the style of test_gpu_regimes.saturated_volume with
    the weights drawn from all of 0..255 (upload accepts them: the divisor
    table's entries up to 256, and weights that fall from 255 to 64)."""
    rng = np.random.default_rng(seed)
    N = int(np.prod(dims))
    w = rng.integers(0, 256, N).astype(np.int16)
    ts = tsat()
    kind = rng.integers(0, 6, N)
    t = np.where(kind <= 2, ts + rng.integers(-3, 4, N),
                 np.where(kind == 3, 32767, rng.integers(-32767, 32768, N))).astype(np.int16)
    t = np.where(kind == 5, -np.abs(t), t).astype(np.int16)
    t[w == 0] = 0
    c = rng.integers(0, 256, 4 * N, dtype=np.uint8)
    c.reshape(-1, 4)[:, 3] = 0
    c.reshape(-1, 4)[w == 0] = 0
    for a in (t, w, c):
        a.setflags(write=False)
    return t, w, c


def settled_volume(dims):
    """Every voxel at weight 64 and T*: free space as 63 integrations leave it."""
    N = int(np.prod(dims))
    return np.full(N, tsat(), np.int16), np.full(N, 64, np.int16), np.zeros(4 * N, np.uint8)


# --------------------------------------------------------------------------
# the pose's columns, restated in float32 numpy

def columns(case, pose):
    """vc0 (Y, X, 3) and zs (3,) of every column as int_column and the oracle
    form them: R (x vs0, y vs1, 0 vs2) + t in float32, left to right."""
    X, Y, _ = case.dims
    vs = (np.array(case.range, f32) / np.array(case.dims, np.int32).astype(f32)).astype(f32)
    R = np.array(pose.R[:], f32)
    t = np.array(pose.t[:], f32)
    vx = (np.arange(X, dtype=np.int32).astype(f32) * vs[0])[None, :]
    vy = (np.arange(Y, dtype=np.int32).astype(f32) * vs[1])[:, None]
    vz = f32(0) * vs[2]
    vc0 = np.stack([(R[3 * i] * vx + R[3 * i + 1] * vy + R[3 * i + 2] * vz) + t[i] for i in range(3)], -1)
    zs = np.array([R[2] * vs[0], R[5] * vs[0], R[8] * vs[0]], f32)
    return vc0.astype(f32), zs


def accumulated(case, pose):
    """vc (Z, Y, X, 3): vc0 plus z float adds of zs, as every voxel's position is formed."""
    vc0, zs = columns(case, pose)
    out = np.empty((case.dims[2],) + vc0.shape, f32)
    vc = vc0
    for z in range(case.dims[2]):
        out[z] = vc
        vc = (vc + zs).astype(f32)
    return out


def _exp_of(a):
    return ((np.asarray(a, f32).view(np.uint32) >> 23) & 0xff).astype(np.int64) - 127


def column_fast(case, pose):
    """column_fast() of csrc/kfx_kernels.hip for every column, (Y, X) bool, from
    vc0 and zs.  (The kernel evaluates it on the position at a chunk's first
    batch; in the table's cases the component that decides is one of zs, or one
    that zs == 0 leaves where vc0 put it, so the answer is the chunk's too.)
    Used only to count slow and fast tiles on the oracle side."""
    vc0, zs = columns(case, pose)
    Z = case.dims[2]
    ok = np.ones(vc0.shape[:2], bool)
    for k in range(3):
        c0, s = vc0[..., k], zs[k]
        bound = f32(2) * (np.abs(c0) + f32(Z + 1) * np.abs(s))
        ok &= bound <= f32(float.fromhex("0x1.fcp39"))
        e = np.full(c0.shape, 1000, np.int64)
        e = np.where(c0 != 0, np.minimum(e, _exp_of(c0)), e)
        if s != 0:
            e = np.minimum(e, _exp_of(s))
        ok &= (e == 1000) | (e - 23 >= -40)
    return ok


def tiles_of(mask_yx):
    """(Y/8, X/8) bool: tiles with any column of the mask."""
    Y, X = mask_yx.shape
    return mask_yx.reshape(Y // 8, 8, X // 8, 8).any(axis=(1, 3))


def updated_columns(case, weight):
    """(Y, X) bool: columns with an updated voxel in a volume that started zeroed."""
    X, Y, Z = case.dims
    return (np.asarray(weight).reshape(Z, Y, X) > 0).any(axis=0)


def tile_spans(case, weight):
    """Per tile with an updated voxel: last - first updated slice + 1."""
    X, Y, Z = case.dims
    upd = (np.asarray(weight).reshape(Z, Y // 8, 8, X // 8, 8) > 0).any(axis=(2, 4))  # (Z, ty, tx)
    any_ = upd.any(axis=0)
    first = upd.argmax(axis=0)
    last = Z - 1 - upd[::-1].argmax(axis=0)
    return (last - first + 1)[any_]
