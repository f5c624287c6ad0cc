"""The world map on the GPU: kfx_world_points_attr, kfx_world_mesh_attr,
kfx_world_bricks and kfx_save_world_mesh against world_cases' references (extract_cases' numpy
restatement on the bricks' dense bounding box, absent bricks zero-filled), byte for byte."""
import ctypes as C
import re

import numpy as np
import pytest

import extract_cases as EC
import shift_cases as SC
import stream_cases as ST
import world_cases as WC
import kfx
from kfx import BRICK_DTYPE, KFX_OK, BrickStore, KinectFusion, KfxError, synth
from kfx.abi import Intrinsics

pytestmark = pytest.mark.gpu
VDT = EC.VDT


def new_kf(p):
    return KinectFusion(Intrinsics.from_any(synth.Intrinsics.qvga()), p)


def code_of(err) -> int:
    return int(re.search(r"failed \((-?\d+)\)", str(err.value)).group(1))


def assert_world(kf, bricks, pts, tri, what):
    gp, gt = kf.world_points(bricks), kf.world_mesh(bricks)
    assert EC.same(gp, pts), f"{what}: points: {EC.first_difference(gp, pts)}"
    assert EC.same(gt, tri), f"{what}: triangles: {EC.first_difference(gt, tri)}"
    assert kf.world_count(bricks) == len(pts) and kf.world_count(bricks, mesh=True) == len(tri), what
    return gp, gt


# ---- 1. random sparse world ---------------------------------------------------------------

def test_random_sparse_world():
    keep, t, w, rgb = WC.sparse_world()
    p = WC.window_params()
    assert min(WC.absent_face_neighbours(keep, WC.SPARSE_BOX)) >= 1
    got = []
    with new_kf(p) as kf:
        for base in WC.SPARSE_BASES:
            pts, tri, pe, te = WC.reference(p, WC.SPARSE_BOX, t, w, rgb, base)
            assert WC.seam_edges(pe).any() and WC.seam_edges(te).any()  # items across a brick seam
            bricks = WC.bricks_of(t, w, rgb, WC.SPARSE_BOX, keep, base)
            got.append(assert_world(kf, bricks, pts, tri, f"base {base}"))
        print(f"{len(bricks)} bricks, {len(pts)} points, {len(tri)} triangles, last call {kf.world_ms()}")
    for a, b in zip(got[0], got[1]):  # between the bases only the position differs
        assert a["normal"].tobytes() == b["normal"].tobytes() and a["bgra"].tobytes() == b["bgra"].tobytes()
        assert not np.array_equal(a["xyz"], b["xyz"])


# ---- 2. the 27-neighbourhood --------------------------------------------------------------

def test_every_neighbour_is_read():
    """3 x 3 x 3 bricks, negatives at the centre brick's corners: all present, then each of the 26
    neighbours absent in turn.  A wrong neighbour slot or halo offset shows in the centre brick's
    items (test_world_restatement.py: every removal changes the reference)."""
    p = WC.window_params()
    base = (3, -1, 2)
    with new_kf(p) as kf:
        for removed in [None] + [r for r in range(27) if r != 13]:
            keep, t, w, rgb = WC.neigh_world(removed)
            pts, tri, _, _ = WC.reference(p, WC.NEIGH_BOX, t, w, rgb, base)
            assert len(pts) > 0 and len(tri) > 0
            assert_world(kf, WC.bricks_of(t, w, rgb, WC.NEIGH_BOX, keep, base), pts, tri, f"without brick {removed}")


# ---- 3. the window alone ------------------------------------------------------------------

def test_window_identity():
    dims = (64, 64, 64)
    p, rec, v, pts, tri = EC.reference("scene", dims)
    with new_kf(p) as kf:
        kf.upload_tsdf(rec)
        bricks = kf.world_bricks()
        t, w, rgb = EC.scene(dims)
        want = WC.bricks_of(t, w, rgb, dims, ST.nonempty_bricks(t, w, WC.rgba(rgb), dims))
        assert bricks.tobytes() == want.tobytes()
        gm = kf.world_mesh(bricks)
        dm = kf.extract_mesh_attr()
        assert EC.same(gm, dm) and EC.same(gm, tri), EC.first_difference(gm, dm)
        gp, dp = kf.world_points(bricks), kf.extract_points_attr()
        assert EC.same(dp, pts)
        wp, _, pe, _ = WC.reference(p, dims, t, w, rgb)
        assert EC.same(gp, wp), EC.first_difference(gp, wp)
        top = pe[:, 2] == dims[2] - 1  # the two differ only in the slice FullScan6 never visits
        assert EC.same(gp[~top], dp) and len(gp) - len(dp) == int(top.sum())
        print(f"window: {len(dp)} points + {int(top.sum())} at z = Z - 1, {len(dm)} triangles")


# ---- 4. excursion, end to end -------------------------------------------------------------

def test_excursion_world():
    """stream_cases.excursion_reference's 12 frames through the lossless loop: the window returns,
    and what it dropped on the way back (33 bricks at b[0] = 8) stays in the store.  The world is
    the window and the store, with the surface across the seam x = 63 -> 64."""
    sp, _ = ST.excursion_reference()
    bgr, dep, _ = SC.frames(12)
    s = ST.EXCURSION
    dims = (64, 64, 64)
    p = SC.params(64)
    with new_kf(p) as kf, BrickStore() as store:
        for k in range(12):
            if k in (4, 8):
                sh = s if k == 4 else tuple(-x for x in s)
                store.put(kf.evict_bricks(sh))
                kf.shift_volume(sh)
                if k == 8:
                    kf.restore_bricks(store.take_window(kf.volume_origin, dims))
            assert kf.pipeline(bgr[k], dep[k]) == KFX_OK
        assert kf.synchronize() == KFX_OK
        held = len(store)
        bricks = kf.world_bricks(store)
        window = kf.world_bricks()
        assert len(store) == held and kf.volume_origin == tuple(sp.origin)
        gp, gt = kf.world_points(bricks), kf.world_mesh(bricks)
        n_win = (kf.extract_count(attr=True), kf.extract_count(mesh=True, attr=True))
    # the reference: StreamPipeline's final volume and store
    vol = sp.volume()
    win_ref = ST.evict_bricks_ref(*vol, dims, sp.origin, (64, 0, 0))
    assert window.tobytes() == win_ref.tobytes()
    both = {tuple(int(x) for x in b["b"][::-1]): b for b in sp.store.values()}
    n_store = len(both)
    both.update({tuple(int(x) for x in b["b"][::-1]): b for b in win_ref})
    want = np.array([both[k] for k in sorted(both)], BRICK_DTYPE)
    assert n_store == held > 0 and len(want) == len(win_ref) + n_store
    assert bricks.tobytes() == want.tobytes()
    pts, tri, pe, te = WC.reference_of_bricks(p, want)
    assert EC.same(gp, pts), EC.first_difference(gp, pts)
    assert EC.same(gt, tri), EC.first_difference(gt, tri)
    # not vacuous: the world holds more than the window, items cross the seam, none at z = 63
    base, box, _, _, _ = WC.box_of(want)
    assert base[0] == 0 and box[0] == 72 and box[2] == 64
    seam = (pe[:, 0] == 63) & (pe[:, 3] == 0)
    stored = pe[:, 0] >= 64
    print(f"store {n_store} bricks; world {len(pts)} points ({int(stored.sum())} from stored bricks, "
          f"{int(seam.sum())} across x = 63 -> 64), {len(tri)} triangles; window {n_win[0]} points, {n_win[1]} triangles")
    assert len(pts) > n_win[0] and len(tri) > n_win[1]
    assert seam.sum() > 0 and stored.sum() > 0 and not (pe[:, 2] == 63).any()


# ---- 5. contract --------------------------------------------------------------------------

def test_contract():
    keep, t, w, rgb = WC.sparse_world()
    p = WC.window_params()
    bricks = WC.bricks_of(t, w, rgb, WC.SPARSE_BOX, keep, (-2, 1, -3))
    pts, tri, _, _ = WC.reference(p, WC.SPARSE_BOX, t, w, rgb, (-2, 1, -3))
    L = kfx.lib()
    with new_kf(p) as kf:
        for cap in (1, len(pts) // 2, len(pts), len(pts) + 5):  # the prefix, and the total still reported
            assert EC.same(kf.world_points(bricks, cap=cap), pts[:cap]), cap
        for cap in (1, len(tri) // 3, len(tri) + 5):
            assert EC.same(kf.world_mesh(bricks, cap=cap), tri[:cap]), cap
        n = C.c_int64(-7)
        bp = bricks.ctypes.data_as(C.c_void_p)
        for name, total in (("kfx_world_points_attr", len(pts)), ("kfx_world_mesh_attr", len(tri))):
            fn = getattr(L, name)
            out = np.full(30, 0x5a, np.uint8).repeat(28).view(VDT)
            before = out.tobytes()
            o = out.ctypes.data_as(C.c_void_p)
            assert fn(kf._h, bp, len(bricks), o, 2, C.byref(n)) == 0 and n.value == total  # cap below the total
            assert fn(kf._h, bp, len(bricks), None, 0, C.byref(n)) == 0 and n.value == total  # cap 0: count only
            assert fn(kf._h, bp, len(bricks), o, 0, C.byref(n)) == 0 and n.value == total
            n.value = -7
            assert fn(kf._h, None, 0, o, 10, C.byref(n)) == 0 and n.value == 0  # n = 0
            assert fn(kf._h, bp, 0, o, 10, C.byref(n)) == 0 and n.value == 0
            assert kf.world_ms() == {"table": 0.0, "count": 0.0, "emit": 0.0}  # ... does no device work
            out[:] = np.full(30, 0x5a, np.uint8).repeat(28).view(VDT)
            bad = {}
            bad["unsorted"] = bricks.copy()
            bad["unsorted"][[3, 4]] = bad["unsorted"][[4, 3]]
            bad["duplicate"] = np.concatenate([bricks[:5], bricks[4:]])
            bad["reserved"] = bricks.copy()
            bad["reserved"]["reserved"][7] = 1
            bad["range"] = bricks.copy()
            bad["range"]["b"][-1, 2] = 1 << 20
            low = bricks.copy()
            low["b"][0, 2] = -(1 << 20)
            bad["range low"] = low
            for what, b in bad.items():
                n.value = -7
                r = fn(kf._h, b.ctypes.data_as(C.c_void_p), len(b), o, 10, C.byref(n))
                assert r == -1 and out.tobytes() == before and n.value == -7, what
            assert fn(kf._h, None, 3, o, 10, C.byref(n)) == -1  # a null list with n > 0
            assert fn(kf._h, bp, -1, o, 10, C.byref(n)) == -1
            assert fn(kf._h, bp, len(bricks), None, 5, C.byref(n)) == -1  # a cap without a buffer
            assert fn(kf._h, bp, len(bricks), o, -1, C.byref(n)) == -1
            assert out.tobytes() == before
        # the largest coordinates still in range
        far = bricks.copy()
        far["b"] += np.array([(1 << 20) - 1 - int(bricks["b"][:, k].max()) for k in range(3)])
        fp, ft, _, _ = WC.reference_of_bricks(p, far)
        assert_world(kf, far, fp, ft, "at the high end of the range")
        far["b"] -= np.array([int(far["b"][:, k].min()) + (1 << 20) - 1 for k in range(3)])
        fp, ft, _, _ = WC.reference_of_bricks(p, far)
        assert_world(kf, far, fp, ft, "at the low end of the range")
        kf.debug_force_index64(True)
        assert_world(kf, bricks, pts, tri, "force_index64")
        kf.debug_force_index64(False)
        # a world of one brick, and world_bricks' short buffer
        assert_world(kf, bricks[:1], *WC.reference_of_bricks(p, bricks[:1])[:2], "one brick")
    with KinectFusion(Intrinsics.from_any(synth.Intrinsics.qvga()), SC.params(64), slab=(0, 2)) as sl:
        with pytest.raises(KfxError) as e:
            sl.world_points(bricks, cap=4)
        assert code_of(e) == -4
        with pytest.raises(KfxError) as e:
            sl.world_bricks()
        assert code_of(e) == -4


def test_world_bricks_merge_and_save(tmp_path):
    """kfx_world_bricks: the window wins an equal coordinate, a short buffer writes nothing, store
    and volume stay; kfx_save_world_mesh writes kfx_world_mesh_attr's triangles."""
    dims = (64, 64, 64)
    p, rec, v, pts, tri = EC.reference("scene", dims)
    t, w, rgb = EC.scene(dims)
    window = WC.bricks_of(t, w, rgb, dims, ST.nonempty_bricks(t, w, WC.rgba(rgb), dims))
    extra = window[:6].copy()
    extra["b"][:3, 0] += 8   # three outside the window (x bricks 8..10) ...
    extra["weight"][3:] = 9  # ... and three on coordinates the window holds
    L = kfx.lib()
    with new_kf(p) as kf, BrickStore() as store:
        kf.upload_tsdf(rec)
        store.put(extra)
        held = store.copy()
        sum0 = kf.volume_checksum()
        got = kf.world_bricks(store)
        key = lambda b: tuple(int(x) for x in b["b"][::-1])
        both = {key(b): b for b in extra[:3]}
        both.update({key(b): b for b in window})
        want = np.array([both[k] for k in sorted(both)], BRICK_DTYPE)
        assert len(want) == len(window) + 3 and got.tobytes() == want.tobytes()
        assert len(store) == 6 and store.copy().tobytes() == held.tobytes()
        assert kf.volume_checksum() == sum0
        n = C.c_int64(-1)
        short = np.full(len(want) - 1, 7, np.uint8).repeat(3600).view(BRICK_DTYPE)
        before = short.tobytes()
        assert L.kfx_world_bricks(kf._h, store._h, short.ctypes.data_as(C.c_void_p), len(short), C.byref(n)) == 0
        assert n.value == len(want) and short.tobytes() == before
        assert L.kfx_world_bricks(kf._h, store._h, None, 0, None) == -1
        assert L.kfx_world_bricks(kf._h, store._h, None, 2, C.byref(n)) == -1
        # the mesh of window + store on disk = write_ply_mesh_attr of world_mesh
        gm = kf.world_mesh(want)
        kf.save_world_mesh(str(tmp_path / "world.ply"), store)
        kfx.write_ply_mesh_attr(str(tmp_path / "want.ply"), gm)
        assert open(tmp_path / "world.ply").read() == open(tmp_path / "want.ply").read()
        kf.save_world_mesh(str(tmp_path / "capped.ply"), store, cap=5)
        kfx.write_ply_mesh_attr(str(tmp_path / "want5.ply"), gm[:5])
        assert open(tmp_path / "capped.ply").read() == open(tmp_path / "want5.ply").read()
        kf.save_world_mesh(str(tmp_path / "window.ply"))  # no store: the window's own mesh
        kfx.write_ply_mesh_attr(str(tmp_path / "want_w.ply"), kf.extract_mesh_attr())
        assert open(tmp_path / "window.ply").read() == open(tmp_path / "want_w.ply").read()


@pytest.mark.parametrize("overlap", [False, True])
def test_world_call_between_staged_frames(overlap):
    """A world call in the middle of a staged sequence (no synchronize around it) changes nothing
    the frames see: poses, volume checksum and graph mode equal those of the run without it."""
    bgr, dep, _ = SC.frames(8)
    p = SC.params(64)
    keep, t, w, rgb = WC.sparse_world()
    bricks = WC.bricks_of(t, w, rgb, WC.SPARSE_BOX, keep)
    pts, tri, _, _ = WC.reference(p, WC.SPARSE_BOX, t, w, rgb)
    runs = []
    for with_world in (False, True):
        with new_kf(p) as kf:
            kf.set_frame_overlap(overlap)
            kf.stage_frames(bgr, dep)
            for k in range(8):
                kf.pipeline_staged(k)
                if with_world and k == 4:
                    mode = kf.graph_mode()
                    assert_world(kf, bricks, pts, tri, "between staged frames")
                    mine = kf.world_mesh(kf.world_bricks())
                    assert kf.graph_mode() == mode
            assert kf.synchronize() == KFX_OK
            runs.append((kf.pose_record.copy(), kf.volume_checksum(), kf.graph_mode(), kf.frame_count))
            if with_world:
                assert len(mine) > 0
    assert np.array_equal(runs[0][0].view(np.uint32), runs[1][0].view(np.uint32))
    assert runs[0][1:] == runs[1][1:]


# ---- 6. runner ----------------------------------------------------------------------------

def test_runner_writes_the_world_mesh(tmp_path):
    """kfx_run's ninth argument against the binding's lossless follow loop and save_world_mesh at
    the runner's parameters, on the dataset of test_gpu_stream.test_runner_streams_bricks (5
    frames, 512^3 over 3 m: the window moves on and leaves bricks in the store)."""
    import os
    import subprocess

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
        bricks = kf.world_bricks(store)
        n_tris = kf.world_count(bricks, mesh=True)
        n_window = kf.extract_count(mesh=True, attr=True)
        kf.save_world_mesh(str(tmp_path / "want.ply"), store)
    assert held >= 1 and len(bricks) > held and n_tris > 0
    out = tmp_path / "world.ply"
    r = subprocess.run([runner, root, str(tmp_path / "poses.txt"), "", "", "", "", str(tmp_path / "f.ply"), "stream",
                        str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"world: (\d+) bricks, (\d+) triangles", r.stdout)
    assert m, r.stdout
    print(m.group(0), f"(window alone {n_window} triangles, {held} bricks held)")
    assert (int(m.group(1)), int(m.group(2))) == (len(bricks), n_tris)
    assert open(out).read() == open(tmp_path / "want.ply").read()
    # without the ninth argument (or with an empty one) no world mesh is written
    r = subprocess.run([runner, root, str(tmp_path / "poses2.txt"), "", "", "", "", str(tmp_path / "f2.ply"), "stream", ""],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "world:" not in r.stdout
