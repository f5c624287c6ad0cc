"""References of the moving volume, shared by
test_shift_restatement.py (CPU) and test_gpu_shift.py.

oracle.Pipeline cannot change its volume pose mid-run, so the pipeline is
restated here from the oracle's stage functions with a mutable volume pose
(StagePipeline); test_shift_restatement.py pins it to oracle.Pipeline bit for
bit before anything is judged by it.
"""
import ctypes as C
import functools

import numpy as np

import oracle as O
from kfx import synth
from kfx.abi import Intrinsics, Params, Pose, default_params

f32 = np.float32
L_VOL = 2.048


def feq(a, b):
    """Bitwise equality of float arrays, NaNs equal."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    z = np.float32(0)
    return np.array_equal(na, nb) and np.array_equal(np.where(na, z, a).view(np.uint32),
                                                     np.where(nb, z, b).view(np.uint32))


def copy_params(p: Params) -> Params:
    q = Params()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(Params))
    return q


def params(dims, rng=None):
    """default_params with per-axis dims; the range keeps the voxel size of 64 voxels per L_VOL
    unless given (the default volume pose centres x and y on the camera)."""
    dims = (dims,) * 3 if np.isscalar(dims) else tuple(dims)
    rng = tuple(L_VOL * d / 64 for d in dims) if rng is None else rng
    p = default_params(dims=dims[0], range_m=rng[0])
    for k in range(3):
        p.volu_dims[k] = int(dims[k])
        p.volu_range[k] = float(rng[k])
    pose = np.eye(4)
    pose[:3, 3] = [float(-f32(rng[0]) / f32(2)), float(-f32(rng[1]) / f32(2)), 0.5]
    p.volu_pose = Pose.from_matrix(pose)
    return p


def shift_soa(t, w, c, dims, s):
    """Roll-and-clear of x-fastest arrays: voxel v <- voxel v + s where that lies inside, else 0."""
    X, Y, Z = (int(d) for d in dims)
    out = []
    for a, per in ((t, 1), (w, 1), (c, 4)):
        a = np.asarray(a).reshape(Z, Y, X, per)
        o = np.zeros_like(a)
        src, dst = [], []
        for n, sk in ((Z, s[2]), (Y, s[1]), (X, s[0])):
            lo, hi = max(0, -sk), min(n, n - sk)  # destination indices with a source inside
            dst.append(slice(lo, max(lo, hi)))
            src.append(slice(lo + sk, max(lo, hi) + sk))
        o[dst[0], dst[1], dst[2]] = a[src[0], src[1], src[2]]
        out.append(o.reshape(-1))
    return tuple(out)


def volume_pose(p: Params, origin, pose0: Pose | None = None) -> Pose:
    """The volume pose of voxel origin `origin` (kfx.h): R0, t0 + R0 (o * vs) in float32:
    d_k = (float)o_k * vs_k; (R[3i] d0 + R[3i+1] d1) + R[3i+2] d2; t0_i + sum."""
    p0 = p.volu_pose if pose0 is None else pose0
    R = [f32(x) for x in p0.R]
    d = [f32(int(origin[k])) * (f32(p.volu_range[k]) / f32(int(p.volu_dims[k]))) for k in range(3)]
    out = Pose()
    for i in range(9):
        out.R[i] = p0.R[i]
    for i in range(3):
        s = f32(f32(f32(R[3 * i] * d[0]) + f32(R[3 * i + 1] * d[1])) + f32(R[3 * i + 2] * d[2]))
        out.t[i] = float(f32(f32(p0.t[i]) + s))
    return out


def shift_for_pose(p: Params, vpose: np.ndarray, cam: np.ndarray, ahead: float):
    """kfx_shift_for_pose restated in double."""
    vpose, cam = np.asarray(vpose, np.float64), np.asarray(cam, np.float64)
    c = cam[:3, :3] @ np.array([0.0, 0.0, float(f32(ahead))]) + cam[:3, 3]
    q = vpose[:3, :3].T @ (c - vpose[:3, 3])
    out = []
    for k in range(3):
        rng = float(p.volu_range[k])
        vs = rng / int(p.volu_dims[k])
        v = ((q[k] - rng / 2) / vs) / 8
        out.append(8 * int(np.floor(abs(v) + 0.5) * np.sign(v)))  # lround: ties away from zero
    return tuple(out)


class StagePipeline:
    """kinectfusion::pipeline (kinectfusion.cpp:78-127) as oracle.Pipeline restates it, composed
    from the oracle's stage functions, with a volume pose that shift() moves."""

    def __init__(self, intr, p: Params):
        self.intr = Intrinsics.from_any(intr)
        self.p = copy_params(p)
        self.L = p.pyramid_height
        self.dims = tuple(int(d) for d in p.volu_dims)
        self.vol = O.Volume(self.dims, [float(r) for r in p.volu_range])
        self.origin = (0, 0, 0)
        self.vpose = volume_pose(self.p, self.origin)
        self.angle = float(f32(np.sin(f32(p.icp_angle_threshold) * f32(0.017453293))))
        self.reset()

    def _zero_maps(self):
        sh = [(self.intr.level(l).height, self.intr.level(l).width, 3) for l in range(self.L)]
        self.pv = [np.zeros(s, np.float32) for s in sh]
        self.pn = [np.zeros(s, np.float32) for s in sh]

    def reset(self, keep_origin=False):
        """kinectfusion::reset.  keep_origin: a tracking-loss reset, which happens on the device
        and leaves the volume pose where the shifts put it."""
        self.frame_count = 1
        self._zero_maps()
        self.vol.tsdf[:] = 0
        self.vol.weight[:] = 0
        self.vol.rgb[:] = 0
        self.poses = [Pose.identity()]
        if not keep_origin:
            self.origin = (0, 0, 0)
            self.vpose = volume_pose(self.p, self.origin)

    def set_volume(self, t, w, c):
        self.vol.tsdf[:], self.vol.weight[:], self.vol.rgb[:] = t, w, c

    def volume(self):
        return self.vol.tsdf, self.vol.weight, self.vol.rgb

    def pose_matrices(self):
        return np.stack([q.matrix() for q in self.poses])

    def shift(self, s):
        t, w, c = shift_soa(self.vol.tsdf, self.vol.weight, self.vol.rgb, self.dims, s)
        self.set_volume(t, w, c)
        self.origin = tuple(int(self.origin[k] + s[k]) for k in range(3))
        self.vpose = volume_pose(self.p, self.origin)

    def vol2cam(self):
        return O.pose_mul(O.pose_inv(self.poses[-1]), self.vpose)  # tsdf_volume.cpp:50

    def cam2vol(self):
        c2v = O.pose_mul(O.pose_inv(self.vpose), self.poses[-1])  # tsdf_volume.cpp:59
        return c2v, c2v.matrix()[:3, :3].T.copy()

    def _integrate(self, ds, bgr):
        O.integrate(self.vol, float(self.p.volu_trun_dist), self.intr, self.vol2cam(), ds[0], bgr)

    def process(self, bgr, depth_mm) -> int:
        ds, vs, ns = O.preprocess(depth_mm, self.intr, self.p)
        self.cur = (ds, vs, ns)
        if self.frame_count == 1:
            self._integrate(ds, bgr)
            self.pv = [v.copy() for v in vs]
            self.pn = [n.copy() for n in ns]
            self.frame_count += 1
            return 0
        cam = Pose.identity()
        for level in range(self.L - 1, -1, -1):  # icp_registration.cpp:16-46
            li = self.intr.level(level)
            for _ in range(int(self.p.icp_iter_count[level])):
                sums = O.icp_accumulate(vs[level], ns[level], self.pv[level], self.pn[level], li, cam,
                                        float(self.p.icp_dist_threshold), self.angle)
                st, cam, _ = O.icp_update(sums, cam)
                if st:  # kinectfusion.cpp:97-101
                    self.reset(keep_origin=True)
                    return 1
        self.poses.append(O.pose_mul(self.poses[-1], cam))
        self._integrate(ds, bgr)
        c2v, Rinv = self.cam2vol()
        self.pv[0], self.pn[0] = O.raycast(self.vol, self.intr, c2v, Rinv)
        for l in range(1, self.L):
            self.pv[l], self.pn[l] = O.resize_points_normals(self.pv[l - 1], self.pn[l - 1])
        self.frame_count += 1
        return 0


def leaving(dims, s):
    """(Z*Y*X,) bool: the voxels shift s drops (not 0 <= v_k - s_k < dims_k)."""
    X, Y, Z = dims
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    keep = ((x - s[0] >= 0) & (x - s[0] < X) & (y - s[1] >= 0) & (y - s[1] < Y) & (z - s[2] >= 0) & (z - s[2] < Z))
    return ~keep.ravel()


def evicted_mask(vol: O.Volume, vpose: Pose, s):
    """Bool mask over oracle.extract_points(vol): the items whose edge has an end that shift s
    drops.  The kept items are the extraction with every leaving voxel's weight 0 (same pose, same
    order); the ordered difference of the two lists marks the evicted positions."""
    dims = tuple(int(d) for d in vol.dims)
    full, n = O.extract_points(vol, vpose)
    w2 = np.array(vol.weight, np.int16)
    w2[leaving(dims, s)] = 0
    kept, nk = O.extract_points(vol, vpose, weight=w2)
    assert n == len(full) and nk == len(kept)
    fb = np.ascontiguousarray(full).view(np.uint32).reshape(-1, 3)
    kb = np.ascontiguousarray(kept).view(np.uint32).reshape(-1, 3)
    mask = np.ones(len(fb), bool)
    j = 0
    for i in range(len(fb)):
        if j < len(kb) and fb[i, 0] == kb[j, 0] and fb[i, 1] == kb[j, 1] and fb[i, 2] == kb[j, 2]:
            mask[i] = False
            j += 1
    assert j == len(kb), "the kept items are no subsequence of the full extraction"
    return mask


def settled_free_volume(dims, intr, depth_mm, p: Params):
    """integrate_cases.settled_volume's values (weight 64 at the ts = 1 fixed point) where the
    voxel lies at least 0.25 m in front of the depth its pixel shows (camera at the origin, the
    start pose of `p`), zero elsewhere: free space as 63 integrations leave it, while the frames
    still build their surfaces from weight 0 (the construction of test_gpu_settled.py, per axis)."""
    import integrate_cases as IC
    X, Y, Z = dims
    t0 = [float(p.volu_pose.t[k]) for k in range(3)]
    vs = [float(p.volu_range[k]) / int(p.volu_dims[k]) for k in range(3)]
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    px, py, pz = x * vs[0] + t0[0], y * vs[1] + t0[1], z * vs[2] + t0[2]
    u = np.rint(px / pz * intr.fx + intr.cx).astype(np.int64)
    v = np.rint(py / pz * intr.fy + intr.cy).astype(np.int64)
    inside = (u >= 0) & (u < intr.width) & (v >= 0) & (v < intr.height)
    d = np.where(inside, depth_mm[np.clip(v, 0, intr.height - 1), np.clip(u, 0, intr.width - 1)] * 0.001, 0.0)
    free = (inside & (d > 0) & (d - np.sqrt(px * px + py * py + pz * pz) >= 0.25)).ravel()
    st, sw, sc = IC.settled_volume(tuple(dims))
    return np.where(free, st, 0).astype(np.int16), np.where(free, sw, 0).astype(np.int16), sc


# --------------------------------------------------------------------------
# shared inputs

def qvga():
    return synth.Intrinsics.qvga()


@functools.lru_cache(maxsize=None)
def frames(n=12, amp_t=0.16):
    """n QVGA frames of the moving trajectory test_gpu_settled.py tracks."""
    bgr, dep, gt = synth.sequence(n, qvga(), noise=True, dropout=0.005, traj_seed=7, amp_t=amp_t, period=60.0)
    return bgr, dep.astype(np.float32), gt


# the pipeline test's two shifts: another axis, another sign
PIPE_SHIFTS = ((8, 0, 0), (0, -8, 0))  # the first drops the left wall, the second keeps the floor


@functools.lru_cache(maxsize=None)
def pipeline_reference(dims=(64, 64, 64)):
    """StagePipeline over 4 frames, shift, 4 frames, shift, 4 frames; every frame KFX_OK (a
    condition on the inputs).  Returns (pipe, fused): fused = the (t, w, c, pose record) before
    the first shift."""
    bgr, dep, _ = frames(12)
    sp = StagePipeline(qvga(), params(dims))
    fused = None
    for k in range(12):
        if k in (4, 8):
            if k == 4:
                fused = tuple(a.copy() for a in sp.volume())
            sp.shift(PIPE_SHIFTS[k // 4 - 1])
        assert sp.process(bgr[k], dep[k]) == 0, f"frame {k} lost in the reference"
    return sp, fused


# eviction / counting identity: a partial shift on each axis and a mixed one.  FullScan6 never
# visits the top slice z = Z - 1, not even for its x and y edges, so the count of the shifted
# volume equals the kept items only while the slice a shift moves to (sz < 0) or away from
# (sz > 0) the top holds no x or y crossing: here sz > 0 and the scene's top slice lies behind the
# back wall, unobserved.
EVICT_SHIFTS = ((16, 0, 0), (0, -16, 0), (0, 0, 24), (-8, 16, 24))


@functools.lru_cache(maxsize=None)
def fused_volume(dims=(64, 64, 64)):
    """The oracle volume of pipeline_reference before its first shift, at the start pose."""
    _, fused = pipeline_reference(dims)
    p = params(dims)
    vol = O.Volume(dims, [float(r) for r in p.volu_range])
    vol.tsdf[:], vol.weight[:], vol.rgb[:] = fused
    return vol, volume_pose(p, (0, 0, 0)), p
