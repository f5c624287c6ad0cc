"""The indexed mesh on the GPU: kfx_extract_mesh_indexed and kfx_world_mesh_indexed
against indexed_cases' reference (the distinct grid edges of extract_cases' oracle-checked soup in
the owner's canonical order, and each corner's rank among them), bit for bit, on the smallest
volumes at which each path can go wrong; test_indexed_cases.py (CPU) checks that the fixtures hold
what they are used for here.  verts[tris] must also be the soup call's own output."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import extract_cases as EC
import indexed_cases as IC
import integrate_cases as NC
import shift_cases as SC
import stream_cases as ST
import world_cases as WC
import kfx
from kfx import KFX_OK, BrickStore, KinectFusion, KfxError, synth
from kfx.abi import Intrinsics

pytestmark = pytest.mark.gpu
VDT = EC.VDT
INTR = Intrinsics.from_any(synth.Intrinsics.qvga())


def code_of(err) -> int:
    return int(re.search(r"failed \((-?\d+)\)", str(err.value)).group(1))


def assert_indexed(got, ref: IC.Indexed, what):
    verts, tris = got
    assert tris.dtype == np.uint32 and tris.shape == ref.tris.shape, f"{what}: {tris.shape} triangles, want {ref.tris.shape}"
    assert EC.same(verts, ref.verts), f"{what}: vertices: {EC.first_difference(verts, ref.verts)}"
    bad = np.nonzero((tris != ref.tris).any(1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(tris)} triangles differ, first {bad[0]}: {tris[bad[0]]} vs {ref.tris[bad[0]]}"


def assert_window(kf, ref, what):
    got = kf.extract_mesh_indexed()
    assert_indexed(got, ref, what)
    soup = kf.extract_mesh_attr(len(ref.tris) + 5)
    assert EC.same(got[0][got[1]], soup), f"{what}: verts[tris] vs extract_mesh_attr: {EC.first_difference(got[0][got[1]], soup)}"
    assert kf.indexed_count() == (len(ref.verts), len(ref.tris)), what
    return got


def assert_world(kf, bricks, ref, what):
    got = kf.world_mesh_indexed(bricks)
    assert_indexed(got, ref, what)
    soup = kf.world_mesh(bricks, len(ref.tris) + 5)
    assert EC.same(got[0][got[1]], soup), f"{what}: verts[tris] vs world_mesh_attr: {EC.first_difference(got[0][got[1]], soup)}"
    return got


_contexts = {}


@pytest.fixture(scope="module")
def uploaded():
    """name, dims -> (context with the volume uploaded, reference)."""
    def get(name, dims):
        if (name, dims) not in _contexts:
            p, rec, _, ref = IC.window_case(name, tuple(dims))
            kf = KinectFusion(INTR, p)
            kf.upload_tsdf(rec)
            _contexts[name, dims] = (kf, ref)
        return _contexts[name, dims]
    yield get
    for kf, _ in _contexts.values():
        kf.close()
    _contexts.clear()


# ---- small volumes ---------------------------------------------------------------------

@pytest.mark.parametrize("name,dims", [("dense", EC.CRAFT_DIMS), ("scene", (40, 32, 24))])
def test_small_volumes(uploaded, name, dims):
    kf, ref = uploaded(name, dims)
    assert_window(kf, ref, name)
    ms = kf.indexed_ms()
    assert ms["table"] == 0.0 and all(v >= 0.0 for v in ms.values())
    # a short cap on either side: the totals, and nothing written
    L = kfx.lib()
    V, T = len(ref.verts), len(ref.tris)
    for cv, ct in ((V - 1, T), (V, T - 1), (1, 1), (V + 3, 0), (0, T + 3)):
        verts = np.full(V + 3, 0x5a, np.uint8).repeat(28).view(VDT)
        tris = np.full((T + 3, 3), 0xa5a5a5a5, np.uint32)
        before = verts.tobytes(), tris.tobytes()
        nv, nt = C.c_int64(-7), C.c_int64(-7)
        rc = L.kfx_extract_mesh_indexed(kf._h, verts.ctypes.data_as(C.c_void_p) if cv else None, cv,
                                        tris.ctypes.data_as(C.c_void_p) if ct else None, ct, C.byref(nv), C.byref(nt))
        assert rc == 0 and (nv.value, nt.value) == (V, T), (cv, ct)
        assert (verts.tobytes(), tris.tobytes()) == before, (cv, ct)
    # larger buffers than needed: filled, the rest untouched
    verts = np.full(V + 3, 0x5a, np.uint8).repeat(28).view(VDT)
    tris = np.full((T + 3, 3), 0xa5a5a5a5, np.uint32)
    nv, nt = C.c_int64(), C.c_int64()
    assert L.kfx_extract_mesh_indexed(kf._h, verts.ctypes.data_as(C.c_void_p), V + 3, tris.ctypes.data_as(C.c_void_p), T + 3,
                                      C.byref(nv), C.byref(nt)) == 0
    assert_indexed((verts[:V], tris[:T]), ref, name + " with room")
    assert (verts[V:].view(np.uint8) == 0x5a).all() and (tris[T:] == 0xa5a5a5a5).all()


# ---- depths: the short last chunk, the top slice's +x / +y edges ---------------------------

@pytest.mark.parametrize("Z", IC.DEPTHS)
def test_depths(uploaded, Z):
    kf, ref = uploaded("dense", (24, 16, Z))
    assert (ref.edges[:, 2] == Z - 1).any()
    assert_window(kf, ref, f"Z = {Z}")


# ---- K units per wave ------------------------------------------------------------------------

@pytest.mark.parametrize("K", (1, 8, 64))
@pytest.mark.parametrize("name", ("dense", "scene"))
def test_forced_units(uploaded, name, K):
    kf, ref = uploaded(name, EC.SWEEP_DIMS)
    assert kf.debug_extract_units(K) == K
    try:
        assert_window(kf, ref, f"{name} K = {K}")
    finally:
        assert kf.debug_extract_units(0) == 1


def test_forced_units_index64(uploaded):
    kf, ref = uploaded("dense", EC.SWEEP_DIMS)
    assert kf.debug_extract_units(64) == 64
    kf.debug_force_index64(True)
    try:
        assert_window(kf, ref, "index64")
    finally:
        kf.debug_force_index64(False)
        kf.debug_extract_units(0)


def test_three_scan_blocks(uploaded):
    """8704 units: three blocks of each of the two scans, vertices and triangles in every one."""
    kf, ref = uploaded("scene", EC.SCAN_DIMS)
    X, Y, Z = EC.SCAN_DIMS
    assert (X // 8) * (Y // 8) * ((Z + 7) // 8) == 8704 and kf.debug_extract_units(0) == 1
    unit = (ref.edges[:, 2] // 8) * ((X // 8) * (Y // 8)) + (ref.edges[:, 1] // 8) * (X // 8) + ref.edges[:, 0] // 8
    assert set(np.unique(unit // 4096)) == {0, 1, 2}
    assert_window(kf, ref, "three scan blocks")


# ---- the brick skip --------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["interior", "border"])
def test_isolated_after_upload(uploaded, which):
    """An isolated negative's -x / -y / -z vertices are owned by voxels, and for a local coordinate
    0 by bricks, that hold nothing negative: a vertex pass that skips those units loses them."""
    kf, ref = uploaded(which, EC.ISOLATED_DIMS)
    if which == "interior":
        assert (len(ref.verts), len(ref.tris)) == (54, 72)
    for K in (0, 64):
        kf.debug_extract_units(K)
        assert_window(kf, ref, f"{which} K = {K}")
    kf.debug_extract_units(0)


@pytest.mark.parametrize("which", ["interior", "border"])
def test_isolated_after_shifts(which):
    """ISOLATED_SHIFT there and back: the occupancy marks are the shift's own."""
    dims, s = EC.ISOLATED_DIMS, EC.ISOLATED_SHIFT
    p = EC.params_for(dims)
    t, w, rgb = EC.isolated(dims, (EC.isolated_interior if which == "interior" else EC.isolated_border)(dims))
    back = tuple(-x for x in s)
    c4 = np.zeros((len(t), 4), np.uint8)
    c4[:, :3] = rgb
    t2, w2, c2 = SC.shift_soa(*SC.shift_soa(t, w, c4.ravel(), dims, s), dims, back)
    ref = IC.reference(EC.Vol(dims, tuple(float(r) for r in p.volu_range), p.volu_pose, t2, w2, c2))
    if which == "interior":
        assert (len(ref.verts), len(ref.tris)) == (54, 72)
    with KinectFusion(INTR, p) as kf:
        kf.upload_tsdf(EC.records(t, w, rgb))
        kf.shift_volume(s)
        kf.shift_volume(back)
        assert kf.volume_origin == (0, 0, 0)
        for K in (0, 64):
            kf.debug_extract_units(K)
            assert_window(kf, ref, f"{which} shifted K = {K}")


# ---- a shifted window --------------------------------------------------------------------

def test_shifted_fused_window():
    """A fused 64^3 window after a shift: the reference of the rolled volume under the moved pose."""
    vol, _, p = SC.fused_volume()
    s = SC.EVICT_SHIFTS[3]
    dims = tuple(int(d) for d in p.volu_dims)
    t, w, c = SC.shift_soa(vol.tsdf, vol.weight, vol.rgb, dims, s)
    v = EC.Vol(dims, tuple(float(r) for r in p.volu_range), SC.volume_pose(p, s), t, w, c)
    ref = IC.reference(v)
    assert EC.same(ref.verts[ref.tris], EC.restate(v)[1]) and len(ref.tris) > 1000
    with KinectFusion(INTR, p) as kf:
        kf.upload_tsdf(NC.records(vol.tsdf, vol.weight, vol.rgb))
        kf.shift_volume(s)
        assert kf.volume_origin == tuple(s)
        assert_window(kf, ref, f"shift {s}")


# ---- the world ---------------------------------------------------------------------------

def test_sparse_world():
    keep, t, w, rgb = WC.sparse_world()
    p = WC.window_params()
    got = []
    with KinectFusion(INTR, p) as kf:
        for base in WC.SPARSE_BASES:
            ref = IC.world_reference(p, WC.SPARSE_BOX, t, w, rgb, base)
            bricks = WC.bricks_of(t, w, rgb, WC.SPARSE_BOX, keep, base)
            got.append(assert_world(kf, bricks, ref, f"base {base}"))
        ms = kf.indexed_ms()
        print(f"{len(bricks)} bricks, {len(ref.verts)} vertices, {len(ref.tris)} triangles, last call {ms}")
        assert all(v >= 0.0 for v in ms.values()) and ms["table"] > 0.0
        kf.debug_force_index64(True)
        assert_world(kf, bricks, ref, "force_index64")
        kf.debug_force_index64(False)
        assert_world(kf, bricks[:1], IC.world_reference_of_bricks(p, bricks[:1]), "one brick")
        # n = 0: nothing, and no device work
        L = kfx.lib()
        nv, nt = C.c_int64(-7), C.c_int64(-7)
        assert L.kfx_world_mesh_indexed(kf._h, None, 0, None, 0, None, 0, C.byref(nv), C.byref(nt)) == 0
        assert (nv.value, nt.value) == (0, 0) and kf.indexed_ms() == {"table": 0.0, "count": 0.0, "verts": 0.0, "tris": 0.0}
        v0, t0 = kf.world_mesh_indexed(bricks[:0])
        assert len(v0) == 0 and t0.shape == (0, 3)
    (va, ta), (vb, tb) = got  # between the bases only the position differs
    assert np.array_equal(ta, tb) and va["normal"].tobytes() == vb["normal"].tobytes() and va["bgra"].tobytes() == vb["bgra"].tobytes()
    assert not np.array_equal(va["xyz"], vb["xyz"])


def test_every_neighbour_is_looked_up():
    """3 x 3 x 3 bricks, negatives at the centre brick's corners, each of the 26 neighbours absent in
    turn: owners in each of the 7 + neighbours, found through the table or absent with their cubes."""
    p = WC.window_params()
    base = (3, -1, 2)
    with KinectFusion(INTR, p) as kf:
        for removed in [None] + [r for r in range(27) if r != 13]:
            keep, t, w, rgb = WC.neigh_world(removed)
            ref = IC.world_reference(p, WC.NEIGH_BOX, t, w, rgb, base)
            assert len(ref.tris) > 0
            assert_world(kf, WC.bricks_of(t, w, rgb, WC.NEIGH_BOX, keep, base), ref, f"without brick {removed}")


def test_window_identity():
    """At origin (0, 0, 0) the world of the window's bricks is the window, on a volume whose top
    slice holds no crossing."""
    dims = (64, 64, 64)
    p, rec, v, ref = IC.window_case("scene", dims)
    with KinectFusion(INTR, p) as kf:
        kf.upload_tsdf(rec)
        win = assert_window(kf, ref, "window")
        world = assert_world(kf, kf.world_bricks(), ref, "world of the window")
        assert EC.same(win[0], world[0]) and np.array_equal(win[1], world[1])


def test_world_list_errors():
    keep, t, w, rgb = WC.sparse_world()
    p = WC.window_params()
    bricks = WC.bricks_of(t, w, rgb, WC.SPARSE_BOX, keep, (-2, 1, -3))
    bad = {"unsorted": bricks.copy(), "duplicate": np.concatenate([bricks[:5], bricks[4:]]), "reserved": bricks.copy(),
           "range": bricks.copy(), "range low": bricks.copy()}
    bad["unsorted"][[3, 4]] = bad["unsorted"][[4, 3]]
    bad["reserved"]["reserved"][7] = 1
    bad["range"]["b"][-1, 2] = 1 << 20
    bad["range low"]["b"][0, 2] = -(1 << 20)
    texts = {"unsorted": "ascend strictly", "duplicate": "ascend strictly", "reserved": "reserved field", "range": "outside (-2^20, 2^20)",
             "range low": "outside (-2^20, 2^20)"}
    L = kfx.lib()
    with KinectFusion(INTR, p) as kf:
        verts = np.full(40, 0x5a, np.uint8).repeat(28).view(VDT)
        tris = np.full((40, 3), 0xa5a5a5a5, np.uint32)
        before = verts.tobytes(), tris.tobytes()
        vp, tp = verts.ctypes.data_as(C.c_void_p), tris.ctypes.data_as(C.c_void_p)
        nv, nt = C.c_int64(-7), C.c_int64(-7)
        for what, b in bad.items():
            assert L.kfx_world_mesh_indexed(kf._h, b.ctypes.data_as(C.c_void_p), len(b), vp, 40, tp, 40, C.byref(nv), C.byref(nt)) == -1, what
            assert texts[what] in L.kfx_last_error().decode(), what
            soup_n = C.c_int64()
            assert L.kfx_world_mesh_attr(kf._h, b.ctypes.data_as(C.c_void_p), len(b), None, 0, C.byref(soup_n)) == -1
            assert texts[what] in L.kfx_last_error().decode(), what  # the same text as the soup call's
        bp = bricks.ctypes.data_as(C.c_void_p)
        assert L.kfx_world_mesh_indexed(kf._h, None, 3, vp, 40, tp, 40, C.byref(nv), C.byref(nt)) == -1
        assert L.kfx_world_mesh_indexed(kf._h, bp, -1, vp, 40, tp, 40, C.byref(nv), C.byref(nt)) == -1
        assert (nv.value, nt.value) == (-7, -7) and (verts.tobytes(), tris.tobytes()) == before


# ---- contract ------------------------------------------------------------------------------

def test_argument_errors(uploaded):
    kf, ref = uploaded("dense", EC.CRAFT_DIMS)
    keep, t, w, rgb = WC.sparse_world()
    bricks = WC.bricks_of(t, w, rgb, WC.SPARSE_BOX, keep)
    L = kfx.lib()
    verts = np.full(10, 0x5a, np.uint8).repeat(28).view(VDT)
    tris = np.full((10, 3), 0xa5a5a5a5, np.uint32)
    before = verts.tobytes(), tris.tobytes()
    vp, tp, bp = verts.ctypes.data_as(C.c_void_p), tris.ctypes.data_as(C.c_void_p), bricks.ctypes.data_as(C.c_void_p)
    nv, nt = C.c_int64(-7), C.c_int64(-7)
    rv, rt = C.byref(nv), C.byref(nt)
    for args in ((vp, 10, tp, 10, None, rt), (vp, 10, tp, 10, rv, None), (vp, -1, tp, 10, rv, rt), (vp, 10, tp, -1, rv, rt),
                 (None, 10, tp, 10, rv, rt), (vp, 10, None, 10, rv, rt)):
        assert L.kfx_extract_mesh_indexed(kf._h, *args) == -1, args
        assert L.kfx_world_mesh_indexed(kf._h, bp, len(bricks), *args) == -1, args
    assert (nv.value, nt.value) == (-7, -7) and (verts.tobytes(), tris.tobytes()) == before
    assert L.kfx_get_indexed_ms(kf._h, None) == -1
    assert L.kfx_save_mesh_indexed(kf._h, None) == -1 and L.kfx_save_world_mesh_indexed(kf._h, None, None) == -1


def test_slab_of_two_is_refused():
    keep, t, w, rgb = WC.sparse_world()
    bricks = WC.bricks_of(t, w, rgb, WC.SPARSE_BOX, keep)
    with KinectFusion(INTR, SC.params(64), slab=(0, 2)) as sl:
        for call in (sl.extract_mesh_indexed, sl.indexed_count, lambda: sl.world_mesh_indexed(bricks)):
            with pytest.raises(KfxError) as e:
                call()
            assert code_of(e) == -4


@pytest.mark.parametrize("overlap", [False, True])
def test_call_between_staged_frames(overlap):
    """Both calls in the middle of a staged sequence (no synchronize around them): poses, volume,
    graph mode and the pending status equal those of the run without them."""
    bgr, dep, _ = SC.frames(8)
    p = SC.params(64)
    keep, t, w, rgb = WC.sparse_world()
    bricks = WC.bricks_of(t, w, rgb, WC.SPARSE_BOX, keep)
    ref = IC.world_reference(p, WC.SPARSE_BOX, t, w, rgb)
    runs = []
    for with_calls in (False, True):
        with KinectFusion(INTR, p) as kf:
            kf.set_frame_overlap(overlap)
            kf.stage_frames(bgr, dep)
            for k in range(8):
                kf.pipeline_staged(k)
                if with_calls and k == 4:
                    mode = kf.graph_mode()
                    assert_world(kf, bricks, ref, "between staged frames")
                    verts, tris = kf.extract_mesh_indexed()
                    assert len(tris) > 0 and EC.same(verts[tris], kf.extract_mesh_attr())
                    assert kf.graph_mode() == mode
            status = kf.synchronize()
            runs.append((kf.pose_record.copy(), status, kf.volume_checksum(), kf.graph_mode(), kf.frame_count))
    assert runs[0][1] == KFX_OK
    assert np.array_equal(runs[0][0].view(np.uint32), runs[1][0].view(np.uint32))
    assert runs[0][1:] == runs[1][1:]


def test_timings_do_not_touch_each_other(uploaded):
    kf, ref = uploaded("dense", EC.CRAFT_DIMS)
    keep, t, w, rgb = WC.sparse_world()
    bricks = WC.bricks_of(t, w, rgb, WC.SPARSE_BOX, keep)
    kf.extract_mesh_attr()
    x0 = kf.extract_ms()
    kf.world_mesh(bricks)
    w0 = kf.world_ms()
    kf.extract_mesh_indexed()
    i0 = kf.indexed_ms()
    assert i0["table"] == 0.0 and i0["count"] > 0.0 and i0["verts"] > 0.0 and i0["tris"] > 0.0
    assert kf.extract_ms() == x0 and kf.world_ms() == w0
    kf.world_mesh_indexed(bricks)
    i1 = kf.indexed_ms()
    assert i1["table"] > 0.0 and kf.extract_ms() == x0 and kf.world_ms() == w0
    kf.extract_mesh_attr()
    kf.world_mesh(bricks)
    kf.extract_points_attr()
    assert kf.indexed_ms() == i1
    assert kf.indexed_count() == (len(ref.verts), len(ref.tris))
    i2 = kf.indexed_ms()
    assert i2["verts"] == 0.0 and i2["tris"] == 0.0 and i2["count"] > 0.0  # count only: no emit work


# ---- files ---------------------------------------------------------------------------------

def test_savers(tmp_path):
    dims = (64, 64, 64)
    p, rec, v, ref = IC.window_case("scene", dims)
    t, w, rgb = EC.scene(dims)
    window = WC.bricks_of(t, w, rgb, dims, ST.nonempty_bricks(t, w, WC.rgba(rgb), dims))
    extra = window[:3].copy()
    extra["b"][:, 0] += 8  # three bricks outside the window
    with KinectFusion(INTR, p) as kf, BrickStore() as store:
        kf.upload_tsdf(rec)
        store.put(extra)
        kf.save_mesh_indexed(str(tmp_path / "window.ply"))
        kfx.write_ply_mesh_indexed(str(tmp_path / "want.ply"), *kf.extract_mesh_indexed())
        text = open(tmp_path / "window.ply").read()
        assert text == open(tmp_path / "want.ply").read() == IC.ply_text(ref.verts, ref.tris)
        kf.save_world_mesh_indexed(str(tmp_path / "world.ply"), store)
        wv, wt = kf.world_mesh_indexed(kf.world_bricks(store))
        kfx.write_ply_mesh_indexed(str(tmp_path / "want_w.ply"), wv, wt)
        assert open(tmp_path / "world.ply").read() == open(tmp_path / "want_w.ply").read()
        assert len(wv) > len(ref.verts)
        kf.save_world_mesh_indexed(str(tmp_path / "alone.ply"))  # no store: the window's own world
        assert open(tmp_path / "alone.ply").read() == text
        kf.save_mesh_attr(str(tmp_path / "soup.ply"))
        print(f"PLY: soup {os.path.getsize(tmp_path / 'soup.ply')} bytes, indexed {os.path.getsize(tmp_path / 'window.ply')} bytes")
        assert os.path.getsize(tmp_path / "window.ply") < os.path.getsize(tmp_path / "soup.ply")


def test_runner_writes_the_indexed_meshes(tmp_path):
    """kfx_run's tenth and eleventh arguments against the binding's lossless follow loop, on the
    dataset of test_gpu_world.test_runner_writes_the_world_mesh."""
    import pngw
    from kfx.abi import default_params
    runner = os.path.join(os.path.dirname(kfx.LIB_PATH), "kfx_run")
    intr = SC.qvga()
    bgr, dep, _ = synth.sequence(5, intr, noise=True, dropout=0.01, amp_t=0.16, period=60.0)
    root = str(tmp_path / "ds")
    os.makedirs(os.path.join(root, "color"))
    os.makedirs(os.path.join(root, "depth"))
    for k in range(len(dep)):
        pngw.write_png(os.path.join(root, "color", f"{k:06d}.png"), bgr[k][:, :, ::-1], 8, 2, idat_parts=1)
        pngw.write_png(os.path.join(root, "depth", f"{k:06d}.png"), dep[k], 16, 0, idat_parts=1)
    with open(os.path.join(root, "intr.txt"), "w") as f:
        f.write(f"{intr.fx} 0 {intr.cx}\n0 {intr.fy} {intr.cy}\n0 0 1\n")
    p = default_params()
    dims = tuple(int(d) for d in p.volu_dims)
    ahead = float(np.float32(0.5) + np.float32(p.volu_range[2]) / np.float32(2))
    with KinectFusion(Intrinsics.from_any(intr), p) as kf, BrickStore() as store:
        for k in range(len(dep)):
            assert kf.pipeline(bgr[k], dep[k].astype(np.float32)) == KFX_OK
            s = kfx.shift_for_pose(p, kf.volume_pose, kf.getCurCameraPose(), ahead)
            if any(s):
                store.put(kf.evict_bricks(s))
                kf.shift_volume(s)
                kf.restore_bricks(store.take_window(kf.volume_origin, dims))
        held = len(store)
        n_window = kf.indexed_count()
        bricks = kf.world_bricks(store)
        wv, wt = kf.world_mesh_indexed(bricks)
        kf.save_mesh_indexed(str(tmp_path / "want.ply"))
        kf.save_world_mesh_indexed(str(tmp_path / "want_w.ply"), store)
    # (the bricks this short run leaves in the store hold free space only: no triangle of their own)
    assert held >= 1 and len(bricks) > held and len(wt) >= n_window[1] > 0
    out, out_w = tmp_path / "indexed.ply", tmp_path / "world_indexed.ply"
    r = subprocess.run([runner, root, str(tmp_path / "poses.txt"), "", "", "", "", str(tmp_path / "f.ply"), "stream", "",
                        str(out), str(out_w)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"indexed: (\d+) vertices, (\d+) triangles", r.stdout)
    mw = re.search(r"world indexed: (\d+) bricks, (\d+) vertices, (\d+) triangles", r.stdout)
    assert m and mw and "world:" not in r.stdout, r.stdout
    print(m.group(0), "/", mw.group(0))
    assert (int(m.group(1)), int(m.group(2))) == n_window
    assert tuple(int(g) for g in mw.groups()) == (len(bricks), len(wv), len(wt))
    assert open(out).read() == open(tmp_path / "want.ply").read()
    assert open(out_w).read() == open(tmp_path / "want_w.ply").read()
    # arguments one to nine alone: neither file, neither line
    r = subprocess.run([runner, root, str(tmp_path / "poses2.txt"), "", "", "", "", str(tmp_path / "f2.ply"), "stream", ""],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "indexed" not in r.stdout
