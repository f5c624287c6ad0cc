"""k_integrate against the oracle over volume geometry, poses and arithmetic
paths (the case table of integrate_cases.py; what each case reaches is listed
there, and test_integrate_cases.py holds the populations on the oracle alone).

The bar is test_gpu_parity.py's: counts equal, tsdf / weight / rgb arrays
equal, float maps bit for bit with NaNs matched by position.  No tolerance is
chosen anywhere, and every "this is not vacuous" assertion is evaluated on the
oracle's side.  After the last pose of a case the volume is raycast from that
pose's camera: a brick whose negative voxel integrate failed to mark in the
occupancy maps shows there, under these poses, tails and chunkings.

Every volume is at most 2.3 M voxels and every oracle call takes well under a
second: the smallest shapes that reach each path, not the workload's.
"""
import functools

import numpy as np
import pytest

import integrate_cases as IC
import oracle as O
from kfx import KFX_FRAME_PREV, KinectFusion

pytestmark = pytest.mark.gpu


def feq(a, b):
    """Bit equality of float32 arrays with NaNs compared by position (test_gpu_parity.feq)."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    z = np.float32(0)
    return np.array_equal(np.where(na, z, a).view(np.uint32), np.where(nb, z, b).view(np.uint32))


def mismatch(a, b):
    a = np.asarray(a, np.float32).ravel()
    b = np.asarray(b, np.float32).ravel()
    return int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())


def assert_volume_equal(kf, t, w, c, what, lo=0, hi=None):
    """The context's volume against (t, w, c); lo:hi the voxel range compared (a slab's owned slices)."""
    gt, gw, gc = kf.volume_soa()
    s, s4 = slice(lo, hi), slice(4 * lo, None if hi is None else 4 * hi)
    assert np.array_equal(gt[s], t[s]), f"{what}: tsdf, {(gt[s] != t[s]).sum()} voxels differ"
    assert np.array_equal(gw[s], w[s]), f"{what}: weight, {(gw[s] != w[s]).sum()} voxels differ"
    assert np.array_equal(gc[s4], c[s4]), f"{what}: rgb, {(gc[s4] != c[s4]).sum()} bytes differ"


def assert_raycast_equal(kf, case, vol, pose, what):
    cam2vol, Rinv, maps = IC.raycast_levels(case, vol, pose)
    kf.stage_raycast(cam2vol, Rinv)
    for l, (ov, on) in enumerate(maps):
        _, gv, gn = kf.frame_maps(KFX_FRAME_PREV, l)
        assert feq(gv, ov), f"{what}: raycast vmap level {l}, {mismatch(gv, ov)} of {ov.size} values differ"
        assert feq(gn, on), f"{what}: raycast nmap level {l}, {mismatch(gn, on)} of {on.size} values differ"


@functools.lru_cache(maxsize=None)
def uploaded_steps(name):
    """The oracle's steps of a case from the 0..255-weight random volume, once per case."""
    case = IC.CASES[name]
    steps, vol = IC.integrate_steps(case, IC.random_volume(case.dims))
    for _, t, w, c in steps:
        for a in (t, w, c):
            a.setflags(write=False)
    return steps, vol


def run_case(name, uploaded=False, index64=False):
    """Every pose of the case through stage_integrate in one context, the
    counts and the whole volume against the oracle's after each, then the
    raycast from the last pose."""
    case = IC.CASES[name]
    bgr, depth = IC.frame(case.frame)
    steps, vol = uploaded_steps(name) if uploaded else IC.oracle_zeroed(name)
    with KinectFusion(case.intr, case.params) as kf:
        if index64:
            kf.debug_force_index64(True)
        if uploaded:
            kf.upload_tsdf(IC.records(*IC.random_volume(case.dims)))
        kf.stage_preprocess(bgr, depth)
        for k, (pose, (counts, t, w, c)) in enumerate(zip(case.poses, steps)):
            got = kf.stage_integrate(pose)
            assert got == counts, f"{name} launch {k}: counts {got}, oracle {counts}"
            assert_volume_equal(kf, t, w, c, f"{name} launch {k}")
        assert_raycast_equal(kf, case, vol, case.poses[-1], name)
    return steps


@pytest.mark.parametrize("name", [n for n in IC.CASES if not n.startswith("wide_angle")])
def test_integrate_case(name):
    if name in IC.EMPTY:  # nothing may be touched: the uploaded volume comes back as it went in
        steps = run_case(name, uploaded=True)
        init = IC.random_volume(IC.CASES[name].dims)
        assert steps[0][0] == (0, 0) and all(np.array_equal(a, b) for a, b in zip(steps[0][1:], init))
    else:
        steps = run_case(name)
        assert all(nu >= 500 for (nu, _), *_ in steps)  # oracle only (floors: test_integrate_cases.py)


@pytest.mark.parametrize("name", ["oblique", "reversed", "mixed", "aniso_oblique", "odd"])
def test_integrate_case_on_uploaded_volume(name):
    """From the random volume with weights 0..255: the divisor table up to 256,
    weights falling from 255 to 64, stores over existing colours."""
    steps = run_case(name, uploaded=True)
    w0 = IC.random_volume(IC.CASES[name].dims)[1]
    (nu, nc), _, w1, _ = steps[0]
    assert nu >= 500 and ((w0 > 64) & (w1 == 64)).sum() >= 100  # oracle only


@pytest.mark.parametrize("name", ["oblique", "axis_x_cos", "deep1500", "odd"])
def test_integrate_case_index64(name):
    run_case(name, index64=True)


@pytest.mark.parametrize("name,world", [("slab300", 2), ("slab300", 3), ("aniso_oblique", 2)])
def test_integrate_case_slabs(name, world):
    """One Z-slab context per rank through the stage seam: each rank's owned
    slices equal the oracle's after every pose, and the owned ranges tile Z."""
    case = IC.CASES[name]
    X, Y, Z = case.dims
    bgr, depth = IC.frame(case.frame)
    steps, _ = IC.oracle_zeroed(name)
    own, updated = [], []
    for r in range(world):
        with KinectFusion(case.intr, case.params, slab=(r, world)) as kf:
            zb, zn, o0, o1 = kf.slab_info()
            assert 0 <= zb <= o0 < o1 <= zb + zn <= Z
            own.append((o0, o1))
            kf.stage_preprocess(bgr, depth)
            for k, (pose, (_, t, w, c)) in enumerate(zip(case.poses, steps)):
                kf.stage_integrate(pose, counts=False)
                assert_volume_equal(kf, t, w, c, f"{name} rank {r} of {world} launch {k}", o0 * X * Y, o1 * X * Y)
        updated.append(int((steps[-1][2][o0 * X * Y:o1 * X * Y] > 0).sum()))
    assert own[0][0] == 0 and own[-1][1] == Z and all(a[1] == b[0] for a, b in zip(own, own[1:])), own
    print(f"{name} world {world}: owned {own}, updated voxels per rank {updated}")
    # oracle only: the first two ranks hold updates; in slab300 / 2 rank 1
    # stores from slice 140, above the slab fast-forward's 128 adds
    assert updated[0] >= 1000 and updated[1] >= 1000
    if (name, world) == ("slab300", 2):
        assert own[1][0] - 4 >= 128


def test_settled_skip_under_rotated_poses():
    """Settled free space (weight 64 at T*), the frame twice at the base pose
    (the first launch sets the bytes, the second skips bricks), then from
    behind, along x, obliquely and at the base pose again: the volume equals the
    oracle's after every launch, so no brick is skipped that a pose changes.
    The frame is the table's without its dropouts: a brick is settled only when
    every one of its voxels was updated, and at 32 mm voxels under 160x120
    pixels a brick's 40x40-pixel footprint holds a pixel without depth at 1 %
    dropouts (the device then sets one byte and skips nothing)."""
    case = IC.CASES["base"]
    bgr, depth = IC.frame("qqvga_full")
    d0 = IC.depth_maps("qqvga_full")
    assert (depth > 0).all()
    names = ["base", "base", "reversed_gen", "axis_x", "oblique", "base"]
    init = IC.settled_volume(case.dims)
    vol = IC.new_volume(case, init)
    with KinectFusion(case.intr, case.params) as kf:
        kf.debug_count_settled(True)
        kf.upload_tsdf(IC.records(*init))
        kf.stage_preprocess(bgr, depth)
        for k, n in enumerate(names):
            pose = IC.CASES[n].poses[0]
            before = vol.tsdf.copy()
            counts = O.integrate(vol, case.params.volu_trun_dist, case.intr, pose, d0, bgr)
            assert counts[0] >= 10000 and (vol.tsdf != before).sum() >= 1000  # oracle only
            got = kf.stage_integrate(pose)
            nset, nskip = kf.debug_get_settled()
            print(f"launch {k} ({n}): {nset} bricks set, {nskip} skipped")
            assert got == counts, (k, n, got, counts)
            assert_volume_equal(kf, vol.tsdf, vol.weight, vol.rgb, f"launch {k} ({n})")
            if k == 1:
                assert nskip > 0
        assert_raycast_equal(kf, case, vol, case.poses[0], "after the settled sequence")


@pytest.mark.parametrize("name", ["wide_angle", "wide_angle_32", "wide_angle_inf"])
def test_wide_angle_far_clip(name):
    """fx ~ 10 px: half a pixel changes lambda by several per cent, so updated
    voxels lie up to (1 + delta) / (1 - delta) beyond the depth their pixel
    shows (delta = hypot(1/fx, 1/fy) / 2); the far clips must keep them."""
    steps = run_case(name)
    assert steps[0][0][0] >= IC.FLOORS[name][0][0]  # oracle only
