"""The paths of the extraction that only a product-size volume takes by itself, on volumes of a
few MB: several units per wave (kfx_debug_extract_units forces the K of 512^3 .. 2048^3), the
offset scan over more than one block (kfx_debug_scan, and one volume of three blocks), the skip
of clear bricks next to isolated negatives, depths that are no multiple of 8, and items extracted
under the pose of a shifted volume.  Everything is compared bit for bit with the numpy restatement
of extract_cases.py, which restate() first holds to the oracle's positions; poses are
crafted_params()'s rotated pose and three different voxel sizes unless a test says otherwise.
test_extract_cases.py (CPU) checks that the volumes hold what they are used for here."""
import numpy as np
import pytest

import extract_cases as EC
import integrate_cases as IC
import shift_cases as SC
from kfx import KinectFusion, synth
from kfx.abi import Intrinsics

pytestmark = pytest.mark.gpu

INTR = Intrinsics.from_any(synth.Intrinsics.qvga())
KINDS = ("points", "mesh", "points_attr", "mesh_attr")


def want_of(kind, pts, tri):
    w = tri if kind.startswith("mesh") else pts
    return w if kind.endswith("attr") else w["xyz"]


def extract(kf, kind, cap):
    return getattr(kf, "extract_" + kind)(cap)


def count(kf, kind):
    return kf.extract_count(kind.startswith("mesh"), kind.endswith("attr"))


def differs(got, want):
    """None if got holds want's bytes, else where they part."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"shape / dtype {got.shape} {got.dtype} vs {want.shape} {want.dtype}"
    if got.tobytes() == want.tobytes():
        return None
    if got.dtype == EC.VDT:
        return EC.first_difference(got, want)
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).reshape(len(got), -1).any(1))[0]
    return f"{len(bad)} of {len(got)} items differ, first at {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"


def check_all(kf, pts, tri, kinds=KINDS, what=""):
    for kind in kinds:
        want = want_of(kind, pts, tri)
        d = differs(extract(kf, kind, len(want) + 5), want)
        assert d is None, f"{what} {kind}: {d}"


# ---- forced units per wave -----------------------------------------------------------

SWEEP_VOLUMES = (("scene", EC.SWEEP_DIMS), ("dense", EC.SWEEP_DIMS), ("dense", EC.CRAFT_DIMS))
_contexts = {}


@pytest.fixture(scope="module")
def uploaded():
    """name, dims -> (context with the volume uploaded, params, records, points, triangles)."""
    def get(name, dims):
        if (name, dims) not in _contexts:
            p, rec, _, pts, tri = EC.reference(name, dims)
            kf = KinectFusion(INTR, p)
            kf.upload_tsdf(rec)
            _contexts[name, dims] = (kf, p, rec, pts, tri)
        return _contexts[name, dims]
    yield get
    for kf, *_ in _contexts.values():
        kf.close()
    _contexts.clear()


@pytest.mark.parametrize("K", EC.UNITS)
@pytest.mark.parametrize("name,dims", SWEEP_VOLUMES)
def test_forced_units(uploaded, name, dims, K):
    """Every kind through the pool pass, the overflowing pool + emit pass, the count pass and the
    two-pass path, with K units per wave."""
    kf, _, _, pts, tri = uploaded(name, dims)
    assert kf.debug_extract_units(0) == 1  # the automatic rule: below 131072 units
    assert kf.debug_extract_units(K) == K
    try:
        for kind in KINDS:
            want = want_of(kind, pts, tri)
            n, cap = len(want), len(want) // 3 + 1
            full = extract(kf, kind, n + 5)
            assert kf.extract_ms()["passes"] == 1
            assert differs(full, want) is None, f"{kind}: {differs(full, want)}"
            capped = extract(kf, kind, cap)  # the pool overflows: its counts, then the emit pass
            assert kf.extract_ms()["passes"] == 2
            assert differs(capped, want[:cap]) is None, f"{kind} capped: {differs(capped, want[:cap])}"
            assert count(kf, kind) == n
            kf.set_extract_passes(2)
            try:
                two = extract(kf, kind, n + 5)
                assert kf.extract_ms()["passes"] == 2
                two_capped = extract(kf, kind, cap)
            finally:
                kf.set_extract_passes(1)
            assert differs(two, want) is None, f"{kind} two-pass: {differs(two, want)}"
            assert differs(two_capped, want[:cap]) is None, f"{kind} two-pass capped"
    finally:
        assert kf.debug_extract_units(0) == 1


def test_units_argument(uploaded):
    kf, _, _, pts, _ = uploaded("dense", EC.CRAFT_DIMS)
    assert kf.debug_extract_units(8) == 8
    for bad in (-1, 3, 6, 65, 128):
        with pytest.raises(Exception) as e:
            kf.debug_extract_units(bad)
        assert "(-1)" in str(e.value), bad
        assert kf.debug_extract_units(8) == 8  # unchanged
    assert kf.debug_extract_units(0) == 1
    assert differs(kf.extract_points_attr(len(pts) + 5), pts) is None


@pytest.mark.parametrize("name,dims", SWEEP_VOLUMES)
def test_forced_units_index64(uploaded, name, dims):
    kf, _, _, pts, tri = uploaded(name, dims)
    assert kf.debug_extract_units(64) == 64
    kf.debug_force_index64(True)
    try:
        check_all(kf, pts, tri, what="index64")
    finally:
        kf.debug_force_index64(False)
        kf.debug_extract_units(0)


@pytest.mark.parametrize("K", [8, 64])
@pytest.mark.parametrize("cuts", [(0, 16, 42), (0, 8, 24, 42)])
@pytest.mark.parametrize("name", ["scene", "dense"])
def test_forced_units_slabs(name, cuts, K):
    """Two and three slabs, the volume uploaded to each: their items concatenate to the single
    volume's.  (Explicit cuts: 42 slices are too few for the equal partition's 16 per slab.)"""
    p, rec, _, pts, tri = EC.reference(name, EC.SWEEP_DIMS)
    world = len(cuts) - 1
    members = [KinectFusion(INTR, p, slab=(r, world), cuts=list(cuts)) for r in range(world)]
    try:
        parts = {kind: [] for kind in KINDS}
        for m in members:
            m.upload_tsdf(rec)
            assert m.debug_extract_units(K) == K
            for kind in KINDS:
                parts[kind].append(extract(m, kind, len(want_of(kind, pts, tri)) + 5))
    finally:
        for m in members:
            m.close()
    for kind in KINDS:
        assert all(len(x) > 0 for x in parts[kind])
        d = differs(np.concatenate(parts[kind]), want_of(kind, pts, tri))
        assert d is None, f"{kind}: {d}"


# ---- depths ----------------------------------------------------------------------------

@pytest.mark.parametrize("Z", [9, 13, 41])
def test_depths(Z):
    """Z no multiple of 8: a short last chunk (Z - 1 swept slices) and a short last brick."""
    dims = (24, 16, Z)
    p, rec, _, pts, tri = EC.reference("dense", dims)
    assert len(pts) > 500 and len(tri) > 300
    with KinectFusion(INTR, p) as kf:
        kf.upload_tsdf(rec)
        t, w, _ = kf.volume_soa()
        assert np.array_equal(t, rec["tsdf"]) and np.array_equal(w, rec["weight"])
        assert kf.debug_extract_units(0) == 1
        check_all(kf, pts, tri, what=f"Z = {Z}")
        for kind in KINDS:
            assert count(kf, kind) == len(want_of(kind, pts, tri))


# ---- the offset scan -------------------------------------------------------------------

SCAN_N = (1, 3, 4095, 4096, 4097, 8192, 4096 * 1023 + 1, 4096 * 1024, 4096 * 1024 + 1, 4096 * 2500 + 17)


@pytest.fixture(scope="module")
def small_ctx():
    with KinectFusion(INTR, EC.crafted_params()) as kf:
        yield kf


def check_scan(kf, counts, what):
    counts = np.asarray(counts, np.uint32)
    inc = np.cumsum(counts, dtype=np.uint64)
    want = np.concatenate([np.zeros(1, np.uint64), inc[:-1]])
    off, total = kf.debug_scan(counts)
    assert off.dtype == np.uint64 and off.shape == want.shape
    bad = np.nonzero(off != want)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} offsets differ, first at {bad[0]}: {off[bad[0]]} vs {want[bad[0]]}"
    assert total == int(inc[-1]), f"{what}: total {total} vs {int(inc[-1])}"


@pytest.mark.parametrize("n", SCAN_N)
def test_scan(small_ctx, n):
    """One block, the block boundary, more blocks than the block scan has threads (each then scans
    a run of block sums), against numpy.cumsum in uint64."""
    rng = np.random.default_rng(n)
    check_scan(small_ctx, rng.integers(0, 301, n), f"n = {n} random")
    check_scan(small_ctx, np.zeros(n, np.uint32), f"n = {n} zeros")
    last = np.zeros(n, np.uint32)
    last[-1] = 7
    check_scan(small_ctx, last, f"n = {n} last")


def test_scan_beyond_32_bits(small_ctx):
    check_scan(small_ctx, np.full(8193, 0xFFFFFFFF, np.uint32), "all ones")


def test_scan_arguments(small_ctx):
    import ctypes as C

    from kfx import lib
    cnt, off, tot = (C.c_uint32 * 4)(), (C.c_uint64 * 4)(), C.c_uint64()
    f = lib().kfx_debug_scan
    h = small_ctx._h
    assert f(h, cnt, 4, off, C.byref(tot)) == 0
    assert f(h, None, 4, off, C.byref(tot)) == -1 and f(h, cnt, 4, None, C.byref(tot)) == -1
    assert f(h, cnt, 4, off, None) == -1
    assert f(h, cnt, 0, off, C.byref(tot)) == -1 and f(h, cnt, -5, off, C.byref(tot)) == -1
    assert f(h, cnt, (1 << 28) + 1, off, C.byref(tot)) == -1


def test_three_scan_blocks():
    """8704 units, items in each of the three scan blocks: the block sums are no longer all zero."""
    p, rec, _, pts, tri = EC.reference("scene", EC.SCAN_DIMS)
    with KinectFusion(INTR, p) as kf:
        kf.upload_tsdf(rec)
        assert kf.debug_extract_units(0) == 1
        check_all(kf, pts, tri, kinds=("points_attr", "mesh_attr"), what="three blocks")
        kf.set_extract_passes(2)
        check_all(kf, pts, tri, kinds=("points", "mesh"), what="three blocks, two passes")


# ---- clear bricks --------------------------------------------------------------------------

CLEAR_KINDS = ("points", "mesh", "points_attr")


def isolated_case(which):
    dims = EC.ISOLATED_DIMS
    pos = EC.isolated_interior() if which == "interior" else EC.isolated_border()
    p = EC.params_for(dims)
    t, w, rgb = EC.isolated(dims, pos)
    return p, t, w, rgb


@pytest.mark.parametrize("which", ["interior", "border"])
def test_clear_bricks_after_upload(which):
    """A negative that is alone in its brick neighbourhood: each of the 27 bricks around it must
    be marked, or the items of a face, edge or corner neighbour are dropped."""
    p, t, w, rgb = isolated_case(which)
    pts, tri = EC.restate(EC.volume(p, t, w, rgb))
    assert len(pts) > 0 and len(tri) > 0
    with KinectFusion(INTR, p) as kf:
        kf.upload_tsdf(EC.records(t, w, rgb))
        for K in (0, 64):
            kf.debug_extract_units(K)
            check_all(kf, pts, tri, kinds=CLEAR_KINDS, what=f"{which} K = {K}")


@pytest.mark.parametrize("which", ["interior", "border"])
def test_clear_bricks_after_shifts(which):
    """There and back: the contents inside the kept box return, and the marks are the shift's own.
    (The interior negatives all stay inside the box; the border ones are dropped on the way, and
    with them the rim, which comes back unobserved.)"""
    p, t, w, rgb = isolated_case(which)
    dims, s = EC.ISOLATED_DIMS, EC.ISOLATED_SHIFT
    back = tuple(-x for x in s)
    c4 = np.zeros((len(t), 4), np.uint8)
    c4[:, :3] = rgb
    there = SC.shift_soa(t, w, c4.ravel(), dims, s)
    t2, w2, c2 = SC.shift_soa(*there, dims, back)
    v = EC.Vol(dims, tuple(float(r) for r in p.volu_range), p.volu_pose, t2, w2, c2)
    pts, tri = EC.restate(v)
    if which == "interior":
        assert (t2 < 0).sum() == 9 and (w2 == 0).any() and len(pts) == 54 and len(tri) == 72
    with KinectFusion(INTR, p) as kf:
        kf.upload_tsdf(EC.records(t, w, rgb))
        kf.shift_volume(s)
        kf.shift_volume(back)
        assert kf.volume_origin == (0, 0, 0)
        for a, b, name in zip(kf.volume_soa(), (t2, w2, c2), ("tsdf", "weight", "rgb")):
            assert np.array_equal(a, b), name
        for K in (0, 64):
            kf.debug_extract_units(K)
            check_all(kf, pts, tri, kinds=CLEAR_KINDS, what=f"{which} shifted K = {K}")


@pytest.mark.parametrize("which", ["interior", "border"])
def test_clear_bricks_in_two_slabs(which):
    """The two slabs meet at z = 32: the negatives at z = 31 have their +z edge and four cubes
    across the cut, in slices the lower slab only stores as its halo."""
    p, t, w, rgb = isolated_case(which)
    pts, tri = EC.restate(EC.volume(p, t, w, rgb))
    members = [KinectFusion(INTR, p, slab=(r, 2)) for r in range(2)]
    try:
        assert [m.slab_info()[2:] for m in members] == [(0, 32), (32, 68)]
        for K in (0, 64):
            parts = {kind: [] for kind in CLEAR_KINDS}
            for m in members:
                if K == 0:
                    m.upload_tsdf(EC.records(t, w, rgb))
                m.debug_extract_units(K)
                for kind in CLEAR_KINDS:
                    parts[kind].append(extract(m, kind, 1000))
            for kind in CLEAR_KINDS:
                d = differs(np.concatenate(parts[kind]), want_of(kind, pts, tri))
                assert d is None, f"{which} slabs K = {K} {kind}: {d}"
    finally:
        for m in members:
            m.close()


# ---- after a shift ---------------------------------------------------------------------------

def shifted_reference(p, vol, s, pose0=None):
    dims = tuple(int(d) for d in p.volu_dims)
    t, w, c = SC.shift_soa(vol.tsdf, vol.weight, vol.rgb, dims, s)
    v = EC.Vol(dims, tuple(float(r) for r in p.volu_range), SC.volume_pose(p, s, pose0), t, w, c)
    return EC.restate(v)


@pytest.mark.parametrize("s", SC.EVICT_SHIFTS)
def test_items_after_a_shift(s):
    """The shifted context's attributed items = the restatement of the rolled volume under the
    moved volume pose (which restate() holds to the oracle's positions)."""
    vol, _, p = SC.fused_volume()
    pts, tri = shifted_reference(p, vol, s)
    assert len(pts) > 1000 and len(tri) > 1000
    with KinectFusion(INTR, p) as kf:
        kf.upload_tsdf(IC.records(vol.tsdf, vol.weight, vol.rgb))
        kf.shift_volume(s)
        assert kf.volume_origin == tuple(s)
        check_all(kf, pts, tri, kinds=("points_attr", "mesh_attr"), what=f"shift {s}")


def test_items_after_a_shift_rotated():
    """The same with a start pose whose R is not the identity: t moves by R0 (s * voxel size)."""
    vol, _, p0 = SC.fused_volume()
    p = SC.copy_params(p0)
    p.volu_pose = EC.crafted_params().volu_pose
    s = SC.EVICT_SHIFTS[3]
    pts, tri = shifted_reference(p, vol, s)
    assert len(pts) > 1000 and len(tri) > 1000
    with KinectFusion(INTR, p) as kf:
        kf.upload_tsdf(IC.records(vol.tsdf, vol.weight, vol.rgb))
        kf.shift_volume(s)
        assert np.array_equal(kf.volume_pose.view(np.uint32), SC.volume_pose(p, s).matrix().view(np.uint32))
        check_all(kf, pts, tri, kinds=("points_attr", "mesh_attr"), what=f"rotated, shift {s}")
