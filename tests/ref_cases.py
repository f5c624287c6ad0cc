"""The cases on which the oracle is pinned to the reference's own kernels, and
the two backends that run them.

A case is an id and a function of a backend that returns a list of named
arrays.  The backends expose one interface over
  * Oracle: oracle/kfx_oracle.cpp through oracle.py, and
  * Reference: the reference's per-thread kernels compiled for the host
    (oracle/Makefile target `ref`, oracle/ref_driver.cpp, oracle.ref_lib()).
test_ref_parity.py runs every case on both and compares element by element, and
compares both with the digests tools/ref_digests.py recorded from the
reference (tests/golden/ref_digests.json); test_gpu_ref_digests.py holds
libkfx to the same recorded digests.  Inputs come from the project's existing
case tables (integrate_cases, icp_cases, view_cases, ray_cases, and the tables of
test_gpu_ray_chain / test_gpu_param_space / test_icp_restatement), imported as
they stand.

The reference kernels write only the pixels they reach (a raycast miss, a
normal map's border, a shader's early return), over buffers Frame::reset
zeroes; the backends hand them zeroed buffers accordingly.
"""
import ctypes as C
import functools
import hashlib
import json
import os

import numpy as np

import icp_cases as K
import integrate_cases as IC
import oracle as O
import ray_cases as RS
import test_gpu_param_space as PS
import test_gpu_ray_chain as RC
import test_icp_restatement as IR
import view_cases as VC
from kfx import synth
from kfx.abi import Intrinsics, Pose, default_params

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_digests.json")
REC = np.dtype([("tsdf", "<i2"), ("weight", "<i2"), ("rgb", "u1", 3), ("pad", "u1")])


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _c(a, dt=f32):
    """A contiguous, writable array of dtype dt (the reference's signatures are not const)."""
    return np.array(a, dtype=dt, order="C", copy=True)


def _k4(I):
    return np.array([I.fx, I.fy, I.cx, I.cy], f32)


def _rt(pose):
    return np.array(pose.R[:], f32), np.array(pose.t[:], f32)


def sine_threshold(deg):
    return float(K.sinf_deg(deg))


# --------------------------------------------------------------------------
# backends

class Oracle:
    name = "oracle"

    def new_volume(self, dims, rng, init=None):
        vol = O.Volume(dims, rng)
        if init is not None:
            vol.tsdf[:], vol.weight[:], vol.rgb[:] = init
        return vol

    def integrate(self, vol, trunc, I, pose, dmap, bgr):
        return O.integrate(vol, trunc, I, pose, dmap, bgr)

    def soa(self, vol):
        return vol.tsdf.copy(), vol.weight.copy(), vol.rgb.reshape(-1, 4)[:, :3].copy()

    def raycast(self, vol, I, cam2vol, Rinv):
        return O.raycast(vol, I, cam2vol, Rinv)

    def depth_truncation(self, d_mm, max_dist):
        d = _c(d_mm)
        O.lib().kfo_depth_truncation(O.fptr(d), d.size, max_dist)
        return d

    def vertex_map(self, d, li):
        return O.vertex_map(d, li)

    def normal_map(self, v):
        return O.normal_map(v)

    def resize(self, v, n):
        return O.resize_points_normals(v, n)

    def render(self, v, n, eye, kind):
        return O.render(v, n, eye, kind)

    def level(self, I, l):
        L = O.lib()
        L.kfo_level_intrinsics.argtypes = [C.POINTER(Intrinsics), C.c_int, C.POINTER(Intrinsics)]
        L.kfo_level_intrinsics.restype = None
        out = Intrinsics()
        L.kfo_level_intrinsics(C.byref(I), l, C.byref(out))
        return (out.width, out.height), _k4(out)

    def icp_sums(self, c, I, pose, dist, ang):
        return O.icp_accumulate(c.cur_v, c.cur_n, c.pre_v, c.pre_n, I, pose, dist, ang), None


class Reference:
    name = "reference"

    def __init__(self, lib):
        self.L = lib

    def new_volume(self, dims, rng, init=None):
        n = int(np.prod(dims))
        rec = np.zeros(n, REC) if init is None else IC.records(*init)
        assert rec.dtype.itemsize == self.L.ref_voxel_bytes()
        return dict(rec=rec, dims=np.array(dims, np.int32), range=np.array(rng, f32))

    def integrate(self, vol, trunc, I, pose, dmap, bgr):
        R, t = _rt(pose)
        d, b = _c(dmap), _c(bgr, np.uint8)
        assert d.shape == (I.height, I.width) and b.shape == (I.height, I.width, 3)
        self.L.ref_integrate(_p(vol["rec"]), _p(vol["dims"]), _p(vol["range"]), trunc, _p(_k4(I)), _p(R), _p(t),
                             _p(d), I.width, I.height, _p(b))

    def soa(self, vol):
        r = vol["rec"]
        return r["tsdf"].copy(), r["weight"].copy(), r["rgb"].copy()

    def raycast(self, vol, I, cam2vol, Rinv):
        R, t = _rt(cam2vol)
        v = np.zeros((I.height, I.width, 3), f32)
        n = np.zeros_like(v)
        self.L.ref_raycast(_p(vol["rec"]), _p(vol["dims"]), _p(vol["range"]), _p(_k4(I)), _p(R), _p(t),
                           _p(_c(Rinv).reshape(9)), _p(v), _p(n), I.width, I.height)
        return v, n

    def depth_truncation(self, d_mm, max_dist):
        d = _c(d_mm)
        h, w = d.shape
        # the kernel's second `if` stands outside its bounds check: only where the
        # 32 x 8 blocks tile the image exactly does no thread touch another row
        # or memory past the image
        assert w % 32 == 0 and h % 8 == 0
        self.L.ref_depth_truncation(_p(d), w, h, max_dist)
        return d

    def vertex_map(self, d, li):
        d = _c(d)
        v = np.zeros(d.shape + (3,), f32)
        self.L.ref_vertex_map(_p(d), d.shape[1], d.shape[0], _p(_k4(li)), _p(v))
        return v

    def normal_map(self, v):
        v = _c(v)
        n = np.zeros_like(v)
        self.L.ref_normal_map(_p(v), v.shape[1], v.shape[0], _p(n))
        return n

    def resize(self, v, n):
        v, n = _c(v), _c(n)
        hs, ws = v.shape[0] // 2, v.shape[1] // 2
        assert v.shape[:2] == (2 * hs, 2 * ws) == n.shape[:2]
        vs = np.zeros((hs, ws, 3), f32)
        ns = np.zeros_like(vs)
        self.L.ref_resize(_p(v), _p(n), ws, hs, _p(vs), _p(ns))
        return vs, ns

    def render(self, v, n, eye, kind):
        v, n = _c(v), _c(n)
        out = np.zeros(v.shape, np.uint8)
        self.L.ref_render(_p(v), _p(n), v.shape[1], v.shape[0], _p(_c(eye)), 0 if kind == "phong" else 1, _p(out))
        return out

    def level(self, I, l):
        size, k = np.zeros(2, np.int32), np.zeros(4, f32)
        self.L.ref_level_intrinsics(_p(np.array([I.width, I.height], np.int32)), _p(_k4(I)), l, _p(size), _p(k))
        return (int(size[0]), int(size[1])), k

    def icp_rows(self, c, I, pose, dist, ang):
        R, t = _rt(pose)
        h, w = c.cur_v.shape[:2]
        rows = np.zeros((h, w, 7), f32)
        self.L.ref_icp_rows(_p(_c(c.cur_v)), _p(_c(c.cur_n)), _p(_c(c.pre_v)), _p(_c(c.pre_n)), w, h, _p(_k4(I)),
                            _p(R), _p(t), dist, ang, _p(rows))
        return rows

    def icp_sums(self, c, I, pose, dist, ang):
        """The 27 sums the reference's rows give over the block grid's region
        32 floor(w / 32) x 32 floor(h / 32), each product a float as the kernel
        forms it (row[i] * row[j]), then rint(double(product) * 2^32) summed in
        integers; and the number of pixels with a correspondence (a non-zero row)."""
        rows = self.icp_rows(c, I, pose, dist, ang)
        h, w = rows.shape[:2]
        xe, ye = K.region(w, h)
        r = rows[:ye, :xe].reshape(-1, 7)
        sums, s = np.zeros(27, np.int64), 0
        for a in range(6):
            for b in range(a, 7):
                term = np.rint((r[:, a] * r[:, b]).astype(np.float64) * 2.0 ** 32).astype(np.int64)
                total = (int((term >> 32).sum()) << 32) + int((term & 0xFFFFFFFF).sum())
                assert -(2 ** 63) <= total < 2 ** 63
                sums[s] = total
                s += 1
        return sums, int((r != 0).any(axis=1).sum())


@functools.lru_cache(maxsize=None)
def reference():
    """The Reference backend, or None where libkfx_ref.so can be neither built nor loaded."""
    lib = O.ref_lib()
    return None if lib is None else Reference(lib)


ORACLE = Oracle()


# --------------------------------------------------------------------------
# digests

def canonical(a):
    """Little-endian bytes; every NaN as 0x7fc00000, signed zeros kept."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        u = a.view(np.uint32).copy()
        u[np.isnan(a)] = 0x7FC00000
        return u.astype("<u4").tobytes()
    assert a.dtype.kind in "iu", a.dtype
    return a.astype(a.dtype.newbyteorder("<")).tobytes()


def digest(outputs):
    h = hashlib.sha256()
    for name, a in outputs:
        a = np.ascontiguousarray(a)
        h.update(f"{name}:{a.dtype.kind}{a.dtype.itemsize}:{a.shape};".encode())
        h.update(canonical(a))
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def differing(a, b):
    """(count, first few flat indices) of elements that differ, NaNs matched by position."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return -1, [("shape", a.shape, b.shape, str(a.dtype), str(b.dtype))]
    if a.dtype == np.float32:
        na, nb = np.isnan(a), np.isnan(b)
        bad = (na != nb) | (~na & ~nb & (a.view(np.uint32) != b.view(np.uint32)))
    else:
        bad = a != b
    idx = np.flatnonzero(bad)
    return int(idx.size), idx[:5].tolist()


# --------------------------------------------------------------------------
# shared inputs

def hits(n):
    return int(((n != 0).any(-1) & ~np.isnan(n).any(-1)).sum())


def chain(B, v, n, levels=3):
    """[(v, n)] of the resizePointsNormals chain; an odd-sized level is cropped
    to the 2 ws x 2 hs pixels the kernel reads."""
    out = [(v, n)]
    for _ in range(1, levels):
        v, n = out[-1]
        hs, ws = v.shape[0] // 2, v.shape[1] // 2
        out.append(B.resize(np.ascontiguousarray(v[:2 * hs, :2 * ws]), np.ascontiguousarray(n[:2 * hs, :2 * ws])))
    return out


def named(maps, prefix=""):
    out = []
    for l, (v, n) in enumerate(maps):
        out += [(f"{prefix}vmap{l}", v), (f"{prefix}nmap{l}", n)]
    return out


@functools.lru_cache(maxsize=None)
def qqvga_seq():
    intr = synth.Intrinsics.qqvga()
    return (intr,) + synth.sequence(3, intr, noise=True, dropout=0.01)


# --------------------------------------------------------------------------
# integrate

UPLOADED = ("oblique", "reversed", "mixed", "aniso_oblique", "odd") + IC.EMPTY
SETTLED_SEQUENCE = ("base", "base", "reversed_gen", "axis_x", "oblique", "base")


def run_integrate(B, name, init=None, poses=None, frame_key=None):
    """(outputs after every pose, the backend's final volume, the oracle-style counts or None)."""
    case = IC.CASES[name]
    key = frame_key or case.frame
    bgr, _ = IC.frame(key)
    d0 = IC.depth_maps(key)
    vol = B.new_volume(case.dims, case.range, init)
    out, counts = [], []
    for k, pose in enumerate(poses or case.poses):
        counts.append(B.integrate(vol, case.params.volu_trun_dist, case.intr, pose, d0, bgr))
        t, w, c = B.soa(vol)
        out += [(f"tsdf@{k}", t), (f"weight@{k}", w), (f"rgb@{k}", c)]
    return out, vol, counts


def _int_case(name, start):
    def run(B):
        case = IC.CASES[name]
        if start == "zero":
            out, vol, counts = run_integrate(B, name)
        elif start == "random":
            out, vol, counts = run_integrate(B, name, IC.random_volume(case.dims))
        else:
            out, vol, counts = run_integrate(B, name, IC.settled_volume(case.dims),
                                             [IC.CASES[n].poses[0] for n in SETTLED_SEQUENCE], "qqvga_full")
        # raycast_levels of the case from its last pose's camera
        pose = case.poses[-1] if start != "settled" else case.poses[0]
        cam2vol = O.pose_inv(pose)
        Rinv = cam2vol.matrix()[:3, :3].T.copy()
        v, n = B.raycast(vol, case.intr, cam2vol, Rinv)
        out += named(chain(B, v, n, case.params.pyramid_height), "ray_")
        run.counts = counts
        return out
    return run


def check_integrate(name, start, ref_out, oracle_counts):
    """The table's population floors, on the oracle's counts (the table's own
    measure) and, where the arrays show them, on the reference's arrays."""
    o = dict(ref_out)
    if start == "zero" and name not in IC.EMPTY:
        for k, ((nu, nc), (fu, fc, _)) in enumerate(zip(oracle_counts, IC.FLOORS[name])):
            assert nu >= fu, (name, k, nu)
            assert fc is None or nc >= fc, (name, k, nc)
            prev = o[f"weight@{k - 1}"] if k else np.zeros_like(o["weight@0"])
            assert int((o[f"weight@{k}"] != prev).sum()) == nu  # weights below 64 rise with every update
    elif name in IC.EMPTY:
        assert oracle_counts[0] == (0, 0)
    elif start == "random":
        assert oracle_counts[0][0] >= 500
    else:
        assert all(nu >= 10000 for nu, _ in oracle_counts)


# --------------------------------------------------------------------------
# raycast

@functools.lru_cache(maxsize=None)
def fused_records(fz):
    """(t, w, c) of test_gpu_ray_chain.fuse's volume, fused once by the oracle (an input here)."""
    vol = RC.fuse(fz, *qqvga_seq())
    out = vol.tsdf.copy(), vol.weight.copy(), vol.rgb.copy()
    for a in out:
        a.setflags(write=False)
    return out


def fused_geometry(fz):
    _, dimz, rangez = RC.FUSED[fz]
    return (64, 64, dimz), (RC.L_VOL, RC.L_VOL, rangez)


def chain_view(name):
    """(fused placement, cam2vol, Rinv) of a ray-chain case, or of a placement seen from the fusing camera."""
    if name in RC.CASES:
        fz = RC.CASES[name][0]
        vpose = RC.case_params(name).volu_pose
    else:
        fz = name
        vpose = Pose.from_matrix(RC.FUSED[fz][0])
    cam2vol = O.pose_inv(vpose)
    return fz, cam2vol, cam2vol.matrix()[:3, :3].T.copy()


def _ray_maps(B, name):
    fz, cam2vol, Rinv = chain_view(name)
    dims, rng = fused_geometry(fz)
    vol = B.new_volume(dims, rng, fused_records(fz))
    I = Intrinsics.from_any(qqvga_seq()[0])
    return B.raycast(vol, I, cam2vol, Rinv)


def _ray_case(name):
    def run(B):
        return named(chain(B, *_ray_maps(B, name)))
    return run


def _view_inputs(dims, vname):
    t, w, c, poses = VC.fused(dims)
    I, pose = next((I, pose) for n, I, pose in VC.views(poses[-1]) if n == vname)
    c2v, Rinv = VC.cam2vol(VC.params(dims), pose)
    return (t, w, c.reshape(-1)), I, pose, c2v, Rinv


def _view_maps(B, dims, vname):
    init, I, _, c2v, Rinv = _view_inputs(dims, vname)
    vol = B.new_volume((dims,) * 3, (VC.RANGE_M,) * 3, init)
    return B.raycast(vol, I, c2v, Rinv)


def _view_case(dims, vname):
    def run(B):
        return named(chain(B, *_view_maps(B, dims, vname)))
    return run


VIEW_NAMES = ("off", "odd", "qvga", "own", "big", "miss")


def _rayspace_case(name):
    """A crafted case of ray_cases.py: its analytic volume raycast from its own ray frame."""
    def run(B):
        case = RS.CASES[name]
        vol = B.new_volume(case.dims, case.range, RS.volume(case.vol))
        return named(chain(B, *B.raycast(vol, case.intr, case.cam2vol, case.Rinv)))
    return run


# --------------------------------------------------------------------------
# image kernels

def _image_outputs(B, depth_mm, I, p):
    """Vertex and normal maps of every level from the oracle's filtered depth (pyrDown and the
    bilateral filter are OpenCV's, not the reference's: inputs here), and O.preprocess's own."""
    ds, vs, ns = O.preprocess(depth_mm, I, p)
    out = []
    for l in range(p.pyramid_height):
        if B is ORACLE:
            v, n = vs[l], ns[l]
        else:
            v = B.vertex_map(ds[l], I.level(l))
            n = B.normal_map(v)
        out += [(f"vmap{l}", v), (f"nmap{l}", n)]
    return out


def _seq_frame(geom, k):
    return PS.sequence(*geom)[2][k]


VGA = (640, 480, 525.0, 525.0, 319.5, 239.5)
IMAGE = {}
for _tag, _geom in (("qqvga", PS.QQVGA), ("qvga", PS.QVGA), ("vga", VGA)):
    IMAGE[f"seq_{_tag}"] = (lambda g=_geom: (_seq_frame(g, 0), Intrinsics(*g), PS.params()))
for _n, _kw in PS.PREPROCESS.items():
    for _k in (0, 3):
        IMAGE[f"pp_{_n}_{_k}"] = (lambda kw=_kw, k=_k: (_seq_frame(PS.QVGA, k), Intrinsics(*PS.QVGA), PS.params(**kw)))
for _w, _h, _height, _ksz in ((24, 16, 1, 15), (16, 16, 2, 15), (32, 32, 3, 7), (64, 48, 4, 11), (40, 24, 3, 5)):
    IMAGE[f"tiny_{_w}x{_h}"] = (lambda w=_w, h=_h, height=_height, ksz=_ksz: (
        PS.tiny_depth(w, h), Intrinsics(w, h, 0.8 * w, 0.8 * w, (w - 1) / 2.0, (h - 1) / 2.0),
        PS.params(pyramid_height=height, bfilter_kernel_size=ksz, bfilter_spatial_sigma=3.0,
                  bfilter_color_sigma=40.0)))
for _k in range(PS.N_FRAMES):
    IMAGE[f"hostile_{_k}"] = (lambda k=_k: (PS.hostile(_seq_frame(PS.QVGA, k), k), Intrinsics(*PS.QVGA), PS.params()))


def _image_case(tag):
    def run(B):
        return _image_outputs(B, *IMAGE[tag]())
    return run


# depthTruncation: raw millimetre frames at sizes the 32 x 8 blocks tile exactly
TRUNC = {
    "qqvga_5.0": (lambda: _seq_frame(PS.QQVGA, 0), 5.0),
    "qvga_2.3": (lambda: _seq_frame(PS.QVGA, 3), 2.3),
    "hostile_qvga_5.0": (lambda: PS.hostile(_seq_frame(PS.QVGA, 1), 1), 5.0),
}


def _trunc_case(tag):
    def run(B):
        make, dist = TRUNC[tag]
        return [("dmap", B.depth_truncation(make(), dist))]
    return run


LEVEL_INTRINSICS = [Intrinsics(*PS.QVGA), Intrinsics(*PS.ODD), Intrinsics(*PS.ODD_OFF), Intrinsics(97, 61, 78.75, 80.3, 51.25, 28.5),
                    Intrinsics(1280, 720, 1050.0, 1050.0, 639.5, 359.5), IC.WIDE24, IC.WIDE16, Intrinsics(*VGA)]


def _level_case(B):
    sizes, ks = [], []
    for I in LEVEL_INTRINSICS:
        for l in range(4):
            s, k = B.level(I, l)
            sizes.append(s)
            ks.append(k)
    return [("size", np.array(sizes, np.int32)), ("k", np.array(ks, f32))]


# --------------------------------------------------------------------------
# render

def kat_maps():
    """test_oracle_kat.test_render_kat's pixels: early returns (zero normal, zero vertex) and a NaN normal."""
    rng = np.random.default_rng(3)
    h, w = 4, 5
    v = rng.uniform(-1, 1, (h, w, 3)).astype(f32)
    v[..., 2] += 2
    n = rng.normal(size=(h, w, 3)).astype(f32)
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    n[0, 0] = 0
    v[0, 1] = 0
    n[1, 1] = np.nan
    return v, n, np.array([0.1, -0.2, 0.3], f32)


def _render_case(src):
    def run(B):
        kind, _, rest = src.partition("/")
        if kind == "kat":
            v, n, eye = kat_maps()
        elif kind == "view":
            dims, vname = rest.split("/")
            v, n = _view_maps(B, int(dims), vname)
            eye = _view_inputs(int(dims), vname)[2][:3, 3].astype(f32)
        else:
            v, n = _ray_maps(B, rest)
            eye = np.zeros(3, f32)  # the pose a context logs for its first frame
        run.render_inputs = (v, n, eye)
        return [("phong", B.render(v, n, eye, "phong")), ("normal", B.render(v, n, eye, "normal"))]
    return run


POW_ULPS = 4  # CUDA's documented bound for powf, in float32 ulps


def phong_pow_sensitive(v, n, eye):
    """(H, W) bool: pixels of renderPhong whose bytes depend on how pow(h_cos, 10)
    rounds.  The kernel calls pow(float, int), which no IEEE operation defines:
    CUDA's is within POW_ULPS ulps, a host compiler promotes to double, the
    oracle and the device library multiply (h2 = h h, h4 = h2 h2, h8 = h4 h4,
    h8 h2; DESIGN.md section 5, deviation `pow`).  The shader is restated here
    in float32 numpy in the kernel's order up to h_cos, then finished once with
    the exact power lowered and once raised by POW_ULPS ulps: the colour is
    monotone in the power, so where both ends give the same three bytes every
    admissible pow does, and the pixel is compared; elsewhere the reference's
    value is undefined and the pixel is masked."""
    v, n, eye = (np.asarray(a, f32) for a in (v, n, eye))
    with np.errstate(all="ignore"):
        def unit(a):
            t = np.sqrt(a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1] + a[..., 2] * a[..., 2])
            return a / t[..., None]

        def dot(a, b):
            return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]
        e = unit(eye - v)
        li = unit(np.array([500, 500, -500], f32) - v)
        diffuse = np.array([0.3843, 0.4745, 0.580], f32) * (f32(0.9) * np.abs(dot(n, li)))[..., None]
        hc = np.abs(dot(n, unit(li + e))).astype(np.float64)
        base = (f32(0.1) + diffuse).astype(np.float64)
        ends = []
        for s in (-1, 1):
            pw = hc ** 10 * (1.0 + s * POW_ULPS * 2.0 ** -23)
            coef = (np.float64(f32(0.9)) * pw).astype(f32)
            k = np.minimum(1.0, base + (0.5 * coef.astype(np.float64))[..., None]).astype(f32)
            ends.append((k * f32(255)).astype(np.int64))
        skipped = ~n.any(-1) | ~v.any(-1)  # the kernel's early returns
        return (ends[0] != ends[1]).any(-1) & ~skipped & ~np.isnan(hc)


def masks(cid, fn):
    """{output name: bool mask} of the elements a case leaves out, from the
    case's own inputs: only renderPhong's pow-sensitive pixels."""
    if cid.startswith("render/"):
        m = phong_pow_sensitive(*fn.render_inputs)
        return {"phong": np.broadcast_to(m[..., None], m.shape + (3,))} if m.any() else {}
    return {}


def masked_outputs(cid, fn, outputs):
    """(outputs with the masked elements zeroed, number of masked elements)."""
    ms = masks(cid, fn)
    return [(n, np.where(ms[n], 0, a).astype(a.dtype) if n in ms else a) for n, a in outputs], \
        int(sum(m.sum() for m in ms.values()))


# --------------------------------------------------------------------------
# ICP

ICP_POSES = (("identity", Pose.identity), ("moved", K.moved_pose))
MAGNITUDE = {"f_wall_12m": (12.0, False), "f_wall_30m": (30.0, False), "f_slant_30m": (30.0, True)}


@functools.lru_cache(maxsize=None)
def tracked_qvga():
    """Frame 2 of the noisy QVGA sequence against the model maps the oracle
    pipeline raycast after frame 1 (what its ICP ran on): [(maps, level
    intrinsics)] per level, and the poses its first iteration started from
    (frame 1's) and its last one reached (frame 2's)."""
    from types import SimpleNamespace
    intr = synth.Intrinsics.qvga()
    I = Intrinsics.from_any(intr)
    bgr, dep, _ = synth.sequence(3, intr, noise=True, dropout=0.01)
    p = default_params(dims=64, range_m=2.048)
    pipe = O.Pipeline(I, p)
    for k in range(2):
        assert pipe.process(bgr[k], dep[k].astype(f32)) == 0
    model = [(pipe.map(1, 1, l).copy(), pipe.map(1, 2, l).copy()) for l in range(3)]
    start = Pose.from_matrix(pipe.poses()[-1])
    assert pipe.process(bgr[2], dep[2].astype(f32)) == 0
    reached = Pose.from_matrix(pipe.poses()[-1])
    _, vs, ns = O.preprocess(dep[2].astype(f32), I, p)
    levels = [(SimpleNamespace(cur_v=vs[l], cur_n=ns[l], pre_v=model[l][0], pre_n=model[l][1]), I.level(l))
              for l in range(3)]
    return levels, (("start", start), ("reached", reached))


def icp_runs(cid):
    """[(label, maps, intrinsics, pose, distance threshold, sine threshold, floor on accepted pixels)]."""
    _, kind, *rest = cid.split("/")
    if kind == "tracked":
        levels, poses = tracked_qvga()
        # noisy measured maps against a raycast model that the reference's raycast bias (A3)
        # puts about two voxels off, under a 15 mm gate: only a share of the pixels passes.
        # The floor asks for ten correspondences per unknown of the 6 x 6 system (64), at
        # every level and at both ends of the iteration, so that no sum is formed from nothing
        return [(f"{pn}_level{l}", c, li, pose, 0.015, sine_threshold(30.0), 64)
                for pn, pose in poses for l, (c, li) in enumerate(levels)]
    if kind == "mag":
        c = K.gen_magnitude(*MAGNITUDE[rest[0]])
        npix = c.label.size  # test_icp_restatement: every pixel of these is accepted
        return [("identity", c, c.I, Pose.identity(), 0.015, sine_threshold(30.0), npix)]
    w, h = (int(x) for x in rest[1].split("x"))
    c, dist, deg = K.crafted(rest[0], w, h)
    # test_icp_restatement's floors: at most half rejected by the NaN gate at
    # the identity, more than half accepted under the moved pose.  A zero model
    # normal gives an accepted all-zero row (a_invalid's mn_zero, 1 probe in
    # 15 of at most 600), which the rows alone cannot tell from a rejection.
    floor = c.label.size // 2 - (40 if rest[0] == "a_invalid" else 0)
    return [(n, c, c.I, mk(), dist, sine_threshold(deg), floor) for n, mk in ICP_POSES]


def _icp_case(cid):
    def run(B):
        out, acc = [], []
        for label, c, I, pose, dist, ang, _ in icp_runs(cid):
            sums, n = B.icp_sums(c, I, pose, dist, ang)
            out.append((label, np.asarray(sums, np.int64)))
            acc.append(n)
        run.accepted = acc
        return out
    return run


# --------------------------------------------------------------------------
# the registry: id -> run(backend) -> [(name, array)]

CASES = {}
for _n in IC.CASES:
    CASES[f"int/{_n}"] = _int_case(_n, "zero")
for _n in UPLOADED:
    CASES[f"int_up/{_n}"] = _int_case(_n, "random")
CASES["int_settled/base"] = _int_case("base", "settled")
for _n in list(RC.CASES) + [f for f in RC.FUSED]:
    _id = _n if _n in RC.CASES else f"fused_{_n}"
    CASES[f"ray/{_id}"] = _ray_case(_n)
    CASES[f"render/ray/{_id}"] = _render_case(f"ray/{_n}")
for _d in VC.DIMS:
    for _n in VIEW_NAMES:
        CASES[f"view/{_d}/{_n}"] = _view_case(_d, _n)
        CASES[f"render/view/{_d}/{_n}"] = _render_case(f"view/{_d}/{_n}")
for _n in RS.CASES:
    CASES[f"rayspace/{_n}"] = _rayspace_case(_n)
CASES["render/kat"] = _render_case("kat/")
for _n in IMAGE:
    CASES[f"img/{_n}"] = _image_case(_n)
for _n in TRUNC:
    CASES[f"trunc/{_n}"] = _trunc_case(_n)
CASES["level_intrinsics"] = _level_case
for _n in K.case_table():
    for _w, _h in IR.SIZES:
        CASES[f"icp/crafted/{_n}/{_w}x{_h}"] = _icp_case(f"icp/crafted/{_n}/{_w}x{_h}")
for _n in MAGNITUDE:
    CASES[f"icp/mag/{_n}"] = _icp_case(f"icp/mag/{_n}")
CASES["icp/tracked/qvga"] = _icp_case("icp/tracked/qvga")


def is_icp(cid):
    return cid.startswith("icp/")


def recorded(cid, outputs):
    """What the golden file holds for a case: the 27 sums per pose for ICP cases, else one SHA-256."""
    if is_icp(cid):
        return {name: [int(x) for x in a] for name, a in outputs}
    return digest(outputs)
