"""The world view on the GPU (kfx_world_view_load / kfx_world_view): with the box
set to the window it equals kfx_render_view byte for byte; anywhere else it equals the oracle's
raycast on the dense assembly of the bricks (world_view_cases.py).  Everything is compared as
bytes over whole images; test_world_view_restatement.py shows what the inputs exercise."""
import ctypes as C
import re

import numpy as np
import pytest

import shift_cases as SC
import stream_cases as ST
import view_cases as VC
import world_view_cases as W
import kfx
from kfx import BRICK_DTYPE, KFX_FRAME_PREV, KFX_OK, BrickStore, KinectFusion, KfxError, synth
from kfx.abi import Intrinsics, Pose

pytestmark = pytest.mark.gpu
KINDS = W.KINDS
ERR_ARG, ERR_STATE = -1, -4


def new_kf(p, **kw):
    return KinectFusion(Intrinsics.from_any(synth.Intrinsics.qvga()), p, **kw)


def code_of(err) -> int:
    return int(re.search(r"failed \((-?\d+)\)", str(err.value)).group(1))


def same(a, b):
    return all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def check_refs(kf, refs, what=""):
    """Every view of `refs`, all three kinds with the maps, against the reference; returns the results."""
    out = {}
    for name, intr, pose, ref in refs:
        for kind in KINDS:
            got = kf.world_view(intr, pose, kind, maps=True)
            W.assert_view((kind, got), ref, f"{what} {name}")
            assert np.array_equal(kf.world_view(intr, pose, kind), got[0]), (what, name, kind)  # without the maps
            out[name, kind] = got
    return out


# ---- 1. window identity ---------------------------------------------------------------------

@pytest.mark.parametrize("force64", [False, True])
def test_window_identity(force64):
    """Both index widths of the record reads (and of k_view's voxel reads beside them)."""
    dims = 64
    with new_kf(VC.params(dims)) as kf:
        kf.upload_tsdf(W.fused_records(dims))
        kf.debug_force_index64(force64)
        bricks = kf.world_bricks()
        assert bricks.tobytes() == W.fused_bricks(dims).tobytes()
        kf.world_view_load(bricks, box=((0, 0, 0), (dims,) * 3))
        last = VC.fused(dims)[3][-1]
        for name, intr, pose in VC.views(last):
            ref = VC.reference(dims, intr, pose)
            for kind in KINDS:
                got = kf.world_view(intr, pose, kind, maps=True)
                dense = kf.render_view(intr, pose, kind, maps=True)
                assert same(got, dense), (name, kind)
                W.assert_view((kind, got), ref, name)
                if name == "miss":
                    assert not got[0].any() and not got[3].any()
        ms = kf.world_view_ms()
        assert ms["load"] > 0.0 and ms["render"] > 0.0


def test_window_identity_after_a_shift():
    """The first 5 frames of the excursion: the origin is (8, 0, 0), the box the window, the list
    the window's bricks alone.  A wrong box pose moves every sample."""
    bgr, dep, _ = SC.frames(12)
    with new_kf(SC.params(64)) as kf:
        for k in range(5):
            if k == 4:
                kf.shift_volume(ST.EXCURSION)
            assert kf.pipeline(bgr[k], dep[k]) == KFX_OK
        assert kf.volume_origin == ST.EXCURSION
        bricks = kf.world_bricks()
        kf.world_view_load(bricks, box=(kf.volume_origin, (64, 64, 64)))
        last = kf.pose_record[-1]
        hits = 0
        for name, intr, pose in VC.views(last)[:4]:
            for kind in KINDS:
                got = kf.world_view(intr, pose, kind, maps=True)
                assert same(got, kf.render_view(intr, pose, kind, maps=True)), (name, kind)
                hits += int((got[3] != 0).sum())
        assert hits > 10000


# ---- 2. sparse world against the oracle -------------------------------------------------------

@pytest.mark.parametrize("force64", [False, True])
def test_sparse_world(force64):
    got = []
    with new_kf(W.sparse_params()) as kf:
        kf.debug_force_index64(force64)
        for base in W.SPARSE_BASES:
            kf.world_view_load(W.sparse_bricks(base))  # the default box
            got.append(check_refs(kf, W.sparse_refs(base), f"base {base}"))
    # the camera moved with the world: maps, normal image and coloured pixels are the same bytes
    a, b = got
    for (name, _, _, ref) in W.sparse_refs(W.SPARSE_BASES[0]):
        for kind in KINDS:
            assert same(a[name, kind][1:], b[name, kind][1:]), (name, kind)
        assert np.array_equal(a[name, "normal"][0], b[name, "normal"][0]), name
        col = ref["coloured"]
        assert col.any() and np.array_equal(a[name, "color"][0][col], b[name, "color"][0][col]), name


# ---- 3. far-apart clusters --------------------------------------------------------------------

def test_far_apart_clusters():
    with new_kf(W.cluster_params()) as kf:
        kf.world_view_load(W.cluster_bricks())
        check_refs(kf, W.cluster_refs(), "clusters")


# ---- 4. excursion, end to end -----------------------------------------------------------------

def test_excursion_world_view():
    p, world, win = W.excursion_world()
    bgr, dep, _ = SC.frames(12)
    s = ST.EXCURSION
    with new_kf(p) as kf, BrickStore() as store:
        for k in range(12):
            if k in (4, 8):
                sh = s if k == 4 else tuple(-x for x in s)
                store.put(kf.evict_bricks(sh))
                kf.shift_volume(sh)
                if k == 8:
                    kf.restore_bricks(store.take_window(kf.volume_origin, (64, 64, 64)))
            assert kf.pipeline(bgr[k], dep[k]) == KFX_OK
        assert kf.synchronize() == KFX_OK
        bricks = kf.world_bricks(store)
        assert bricks.tobytes() == world.tobytes()
        kf.world_view_load(bricks)
        got = check_refs(kf, W.excursion_refs(), "excursion")
        # the picture the feature exists for: the window alone shows less
        for name, intr, pose, ref in W.excursion_refs():
            dense_ts = kf.render_view(intr, pose, "color", maps=True)[3]
            assert 0 < (dense_ts != 0).sum() < (got[name, "color"][3] != 0).sum(), name


# ---- 5. box semantics ---------------------------------------------------------------------------

def test_box_semantics():
    """An explicit box smaller than the list, with dims that are no multiple of 8: the bricks
    outside it and the voxels past it are ignored (the result is the filtered list's, and the
    oracle's on the cropped assembly; candidates at the box's faces have NaN normals)."""
    p = VC.params(64)
    bricks = W.fused_bricks(64)
    box = ((8, 8, 0), (48, 45, 61))
    inside = W.filtered(bricks, *box)
    assert 0 < len(inside) < len(bricks)
    last = VC.fused(64)[3][-1]
    views = [v for v in VC.views(last) if v[0] in ("off", "qvga")]
    with new_kf(p) as kf:
        res = []
        for lst in (bricks, inside):
            kf.world_view_load(lst, box=box)
            res.append([kf.world_view(intr, pose, kind, maps=True) for _, intr, pose in views for kind in KINDS])
        for a, b in zip(*res):
            assert same(a, b)
        refs = [(name, intr, pose, W.reference(p, bricks, intr, pose, box=box)) for name, intr, pose in views]
        assert all(r[3]["hit"].sum() > 1000 for r in refs)
        check_refs(kf, refs, "box")
        # the box is part of the result: the same bricks in the window's box give another image
        kf.world_view_load(inside, box=((0, 0, 0), (64, 64, 64)))
        assert not same(kf.world_view(views[0][1], views[0][2], "normal", maps=True), res[0][1])


# ---- 6. snapshot and isolation ------------------------------------------------------------------

def test_snapshot_and_isolation():
    bgr, dep, _ = SC.frames(12)
    A, B = W.sparse_bricks((0, 0, 0)), W.cluster_bricks()
    p = SC.params(64)
    last = np.eye(4, dtype=np.float32)
    cams = [VC.make_view(VC.VIEW_ODD, last), VC.make_view(VC.VIEW_QVGA, last)]

    def render(kf):
        return [kf.world_view(i, q, kind, maps=True) for i, q in cams for kind in KINDS]

    with new_kf(p) as kf:
        kf.world_view_load(A, box=((0, 0, 0), (40, 32, 24)))
        first = render(kf)
        assert any((r[3] != 0).any() for r in first)
        assert len(kf.world_mesh(B)) > 0 and len(kf.world_points(B)) > 0  # the extraction's own buffers
        for k in range(3):
            assert kf.pipeline(bgr[k], dep[k]) == KFX_OK
        kf.shift_volume((8, 0, 0))
        assert kf.pipeline(bgr[3], dep[3]) == KFX_OK
        kf.reset()
        for a, b in zip(first, render(kf)):
            assert same(a, b)
        mesh = kf.world_mesh(B)
        kf.world_view_load(B)
        second = render(kf)
        assert kf.world_mesh(B).tobytes() == mesh.tobytes()  # and the load leaves them alone
        with new_kf(p) as fresh:
            fresh.world_view_load(B)
            for a, b in zip(second, render(fresh)):
                assert same(a, b)
        kf.world_view_load(np.zeros(0, BRICK_DTYPE))  # n = 0 unloads
        with pytest.raises(KfxError) as e:
            kf.world_view(*cams[0])
        assert code_of(e) == ERR_STATE


# ---- 7. the tracker is left alone ---------------------------------------------------------------

def _state(kf):
    maps = [kf.frame_maps(KFX_FRAME_PREV, l)[1:] for l in range(kf.params.pyramid_height)]
    return kf.pose_record, maps, kf.volume_checksum()


@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("graph", [0, 1])
def test_world_view_does_not_disturb_tracking(graph, overlap):
    intr, bgr, dep = VC.scene()
    world = W.sparse_bricks((0, 0, 0))
    big_i, big_p = VC.make_view(VC.VIEW_BIG, np.eye(4, dtype=np.float32))
    states = []
    for with_views in (True, False):
        with new_kf(VC.params(64)) as kf:
            kf.set_graph_mode(graph)
            kf.set_frame_overlap(overlap)
            for k in range(VC.N_FRAMES):
                assert kf.pipeline(bgr[k], dep[k]) == KFX_OK
                if with_views:
                    kf.world_view_load(world if k % 2 else kf.world_bricks())
                    for kind in KINDS:
                        kf.world_view(big_i, big_p, kind, maps=(kind == "color"))
            assert kf.synchronize() == KFX_OK
            states.append(_state(kf))
    (pa, ma, ca), (pb, mb, cb) = states
    assert len(pa) == VC.N_FRAMES and np.array_equal(pa, pb) and ca == cb
    for (v0, n0), (v1, n1) in zip(ma, mb):
        assert np.array_equal(v0.view(np.uint32), v1.view(np.uint32))
        assert np.array_equal(n0.view(np.uint32), n1.view(np.uint32))


def test_world_view_leaves_pending_tracking_status():
    intr, bgr, dep = VC.scene()
    with new_kf(VC.params(64)) as kf:
        kf.world_view_load(W.cluster_bricks())
        kf.pipeline_async(bgr[0], dep[0])
        kf.pipeline_async(bgr[1], dep[1])
        kf.pipeline_async(bgr[2], np.zeros_like(dep[2]))  # no depth: the frame is dropped, the volume reset
        kf.world_view(kf.intr, np.eye(4, dtype=np.float32), "phong")
        assert kf.synchronize() == kfx.KFX_TRACKING_LOST
        assert kf.synchronize() == KFX_OK


# ---- 8. argument table ----------------------------------------------------------------------------

def test_argument_table():
    L = kfx.lib()
    good = W.sparse_bricks((0, 0, 0))
    cam_i, cam_p = W.sparse_views((0, 0, 0))[1][1:]
    I3 = C.c_int * 3

    def load(kf, b, n=None, origin=None, dims=None):
        b = np.ascontiguousarray(b, BRICK_DTYPE)
        return L.kfx_world_view_load(kf._h, b.ctypes.data_as(C.c_void_p) if b is not None and len(b) else None,
                                     len(b) if n is None else n, None if origin is None else I3(*origin),
                                     None if dims is None else I3(*dims))

    def edit(fn):
        b = good.copy()
        fn(b)
        return b

    far = np.zeros(2, BRICK_DTYPE)
    far["b"][0], far["b"][1] = (-(1 << 20) + 1,) * 3, ((1 << 20) - 1,) * 3
    with new_kf(W.sparse_params()) as kf:
        assert load(kf, good) == KFX_OK
        before = kf.world_view(cam_i, cam_p, "color", maps=True)
        assert (before[3] != 0).any()
        refused = [
            ("n < 0", dict(b=good, n=-1)),
            ("null list", dict(b=good[:0], n=3)),
            ("reserved", dict(b=edit(lambda b: b["reserved"].__setitem__(5, 1)))),
            ("descending", dict(b=good[::-1])),
            ("duplicate", dict(b=np.concatenate([good[:4], good[3:]]))),
            ("coordinate 2^20", dict(b=edit(lambda b: b["b"].__setitem__((len(b) - 1, 2), 1 << 20)))),
            ("origin without dims", dict(b=good, origin=(0, 0, 0))),
            ("dims without origin", dict(b=good, dims=(40, 32, 24))),
            ("origin % 8", dict(b=good, origin=(0, 4, 0), dims=(40, 32, 24))),
            ("origin 2^23", dict(b=good, origin=(1 << 23, 0, 0), dims=(40, 32, 24))),
            ("origin -2^23", dict(b=good, origin=(0, 0, -(1 << 23)), dims=(40, 32, 24))),
            ("dims 0", dict(b=good, origin=(0, 0, 0), dims=(40, 0, 24))),
            ("dims < 0", dict(b=good, origin=(0, 0, 0), dims=(-8, 32, 24))),
            ("dims > 2^15", dict(b=good, origin=(0, 0, 0), dims=(40, (1 << 15) + 1, 24))),
            ("box > 2^26 bricks", dict(b=good, origin=(0, 0, 0), dims=(1 << 15, 1 << 15, 8 * 4 + 1))),
            ("default box too large", dict(b=far)),
        ]
        for what, kw in refused:
            assert load(kf, **kw) == ERR_ARG, what
            assert kfx.lib().kfx_last_error()
            after = kf.world_view(cam_i, cam_p, "color", maps=True)  # the previous world is kept
            assert same(before, after), what
        # the limits themselves are accepted
        assert load(kf, good, origin=((1 << 23) - 8, 0, 0), dims=(1 << 15, 8, 8)) == KFX_OK
        assert load(kf, good, origin=(0, 0, 0), dims=(1 << 15, 1 << 15, 8 * 4)) == KFX_OK
        assert load(kf, good) == KFX_OK and same(before, kf.world_view(cam_i, cam_p, "color", maps=True))
        # kfx_world_view's own checks are kfx_render_view's
        out = np.zeros(3 * cam_i.width * cam_i.height, np.uint8)
        op = out.ctypes.data_as(C.POINTER(C.c_uint8))
        P = Pose.from_matrix(cam_p)

        def view(i=cam_i, q=P, kind=0, o=op):
            return L.kfx_world_view(kf._h, C.byref(i) if i is not None else None, C.byref(q) if q is not None else None,
                                    kind, o, None, None, None)

        bad_p = Pose.from_matrix(cam_p)
        bad_p.t[1] = float("nan")
        assert view() == KFX_OK
        assert view(i=None) == ERR_ARG and view(q=None) == ERR_ARG and view(o=None) == ERR_ARG
        assert view(kind=3) == ERR_ARG and view(kind=-1) == ERR_ARG and view(q=bad_p) == ERR_ARG
        for bad in (Intrinsics(0, 48, 60.0, 60.0, 31.5, 23.5), Intrinsics(1 << 14, (1 << 12) + 1, 60.0, 60.0, 31.5, 23.5),
                    Intrinsics(64, 48, 0.0, 60.0, 31.5, 23.5), Intrinsics(64, 48, 60.0, float("inf"), 31.5, 23.5),
                    Intrinsics(64, 48, 60.0, 60.0, float("nan"), 23.5)):
            assert view(i=bad) == ERR_ARG
        assert L.kfx_get_world_view_ms(kf._h, None) == ERR_ARG
        # n = 0 unloads, with a box or without; then there is nothing to render
        assert load(kf, good[:0], origin=(0, 0, 0), dims=(8, 8, 8)) == KFX_OK
        assert view() == ERR_STATE
        assert load(kf, good) == KFX_OK and view() == KFX_OK
        assert load(kf, good[:0]) == KFX_OK and view() == ERR_STATE
    with new_kf(VC.params(64), slab=(0, 2)) as sl:
        assert load(sl, good) == ERR_STATE
        assert L.kfx_world_view(sl._h, C.byref(cam_i), C.byref(P), 0, op, None, None, None) == ERR_STATE


# ---- 9. saver and runner ----------------------------------------------------------------------------

def test_save_world_view(tmp_path):
    p, world, _ = W.excursion_world()
    _, intr, pose = W.excursion_views()[1]
    with new_kf(p) as kf, BrickStore() as store:
        kf.restore_bricks(world)          # the window's part lands in the volume ...
        store.put(world[world["b"][:, 0] >= 8])  # ... the rest waits in the store
        assert len(store) > 0
        path = tmp_path / "world.ppm"
        kf.save_world_view(str(path), intr, pose, "color", store)
        kf.world_view_load(kf.world_bricks(store))
        img = kf.world_view(intr, pose, "color")
        window_only = tmp_path / "window.ppm"
        kf.save_world_view(str(window_only), intr, pose, "color")
    head = b"P6\n%d %d\n255\n" % (intr.width, intr.height)
    data = open(path, "rb").read()
    assert data.startswith(head) and img.any()
    assert data[len(head):] == img[:, :, ::-1].tobytes()  # RGB in the file, B G R in the image
    assert open(window_only, "rb").read() != data


def test_runner_writes_the_world_view(tmp_path):
    """kfx_run's twelfth argument against the binding's lossless follow loop and save_world_view at
    the runner's parameters (test_gpu_world.test_runner_writes_the_world_mesh's dataset)."""
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
    ds = kfx.Dataset(root)
    p = default_params()
    dims = tuple(int(d) for d in p.volu_dims)
    ahead = float(np.float32(0.5) + np.float32(p.volu_range[2]) / np.float32(2))
    with KinectFusion(ds.intrinsics, p) as kf, BrickStore() as store:
        for k in range(len(ds)):
            c, d = ds.read(k)
            assert kf.pipeline(c, d) == KFX_OK
            s = kfx.shift_for_pose(p, kf.volume_pose, kf.getCurCameraPose(), ahead)
            if any(s):
                store.put(kf.evict_bricks(s))
                kf.shift_volume(s)
                kf.restore_bricks(store.take_window(kf.volume_origin, dims))
        assert len(store) >= 1
        kf.save_world_view(str(tmp_path / "want.ppm"), ds.intrinsics, kf.pose_record[0], "color", store)
    ds.close()
    out = tmp_path / "world_view.ppm"
    r = subprocess.run([runner, root, str(tmp_path / "poses.txt"), "", "", "", "", str(tmp_path / "f.ply"), "stream",
                        "", "", "", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"world view: load [\d.]+ ms, render [\d.]+ ms", r.stdout), r.stdout
    data = open(out, "rb").read()
    assert data.startswith(b"P6\n320 240\n255\n") and any(data[15:])
    assert data == open(tmp_path / "want.ppm", "rb").read()
