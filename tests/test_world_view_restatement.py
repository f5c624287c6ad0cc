"""The world view's references checked on the CPU (world_view_cases.py): on the
window's own box the builder reproduces view_cases.reference, and the sparse, cluster and
excursion inputs have the properties they were chosen for."""
import numpy as np

import shift_cases as SC
import stream_cases as ST
import view_cases as VC
import world_cases as WC
import world_view_cases as W

MAPS = ("vmap", "nmap", "ts", "phong", "normal", "color")


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def test_window_box_reproduces_the_view_reference():
    """Box = the window: same dims, so the window's own range, pose and contents.  All six views of
    view_cases, maps and the three images."""
    p = VC.params(64)
    bricks = W.fused_bricks(64)
    assert 0 < len(bricks) < 512  # the window has empty bricks: the assembly fills them with 0
    last = VC.fused(64)[3][-1]
    some = 0
    for name, intr, pose in VC.views(last):
        want = VC.reference(64, intr, pose)
        got = W.reference(p, bricks, intr, pose, box=((0, 0, 0), (64, 64, 64)))
        for k in MAPS + ("hit", "coloured"):
            assert same(got[k], want[k]), (name, k)
        some += int(want["coloured"].sum())
    assert some > 0


def test_box_pose_is_the_shift_formula():
    p = W.sparse_params()
    for o in ((0, 0, 0), (-24, 8, 16)):
        pb = W.box_params(p, o, (40, 32, 24))
        want = SC.volume_pose(p, o)
        assert list(pb.volu_pose.R) == list(want.R) and list(pb.volu_pose.t) == list(want.t)
        d = np.array(o, np.float64) * np.array(W.SPARSE_VS)
        assert np.array_equal(np.array(want.t[:]), np.array([-0.5 - d[1], 0.25 + d[0], 0.125 + d[2]]))  # exact: R0 is used
    assert list(W.box_range(p, (32, 24, 9))[:2]) == [p.volu_range[0], p.volu_range[1]]


def test_assembly_crops_and_filters():
    b = W.sparse_bricks((0, 0, 0))
    t, c = W.assemble(b, (8, 0, 0), (29, 32, 21))
    full, cf = W.assemble(b, (0, 0, 0), W.SPARSE_BOX)
    X, Y, Z = W.SPARSE_BOX
    assert np.array_equal(t.reshape(21, 32, 29), full.reshape(Z, Y, X)[:21, :, 8:37])
    assert np.array_equal(c.reshape(21, 32, 29, 4), cf.reshape(Z, Y, X, 4)[:21, :, 8:37])
    f = W.filtered(b, (8, 0, 0), (29, 32, 21))
    assert 0 < len(f) < len(b) and f["b"][:, 0].min() == 1 and f["b"][:, 0].max() == 4
    t2, _ = W.assemble(f, (8, 0, 0), (29, 32, 21))
    assert np.array_equal(t, t2)


def _first_and_resumed(p, ref, intr, bricks):
    cl, crossed = W.march(p, ref, intr, W.present_cells(ref, bricks))
    hit, ts = ref["hit"], ref["ts"]
    cand = cl > 0
    step = WC.voxel_size(p)[0]
    first = hit & cand & (ts >= cl - step) & (ts < cl)
    resumed = cand & (~hit | (ts >= cl))
    assert not (hit & ~cand).any() and np.array_equal(first | resumed, cand) and not (first & resumed).any()
    return first, resumed, crossed


def test_sparse_world_has_its_properties():
    p = W.sparse_params()
    keep, t, w, rgb, crossing, clear = W.sparse_scene()
    tb = ST.to_bricks(t, W.SPARSE_BOX)[:, :, 0]
    assert len(crossing) == 4 and len(clear) == 3 and not keep[list(crossing + clear)].any() and keep.sum() == 60 - 7
    assert (tb[keep] < 0).any() and (tb[keep] > 0).any()
    bricks = W.sparse_bricks((0, 0, 0))
    assert W.default_box(bricks) == ((-8, -8, -8), (56, 48, 40))
    assert W.default_box(W.sparse_bricks(W.SPARSE_BASES[1])) == ((-24, 0, -32), (56, 48, 40))
    vs = WC.voxel_size(p)
    seam = behind = nan_resumed = later = 0
    kept = keep.reshape(3, 4, 5)
    for name, intr, pose, ref in W.sparse_refs((0, 0, 0)):
        assert (intr.width, intr.height) in ((97, 61), (200, 152), (160, 120), (128, 96))
        hit = ref["hit"]
        assert hit.sum() > 500 and (~hit).sum() > 500, name
        first, resumed, crossed = _first_and_resumed(p, ref, intr, bricks)
        g = np.floor(ref["P"] / vs).astype(np.int64)[hit] - 8  # list voxels (one brick of padding)
        gb = g >> 3
        inside = ((gb >= 0) & (gb < np.array([5, 4, 3]))).all(1)
        cells = set(map(tuple, gb[inside]))
        # hits on both sides of a seam between two present bricks (x = 15 | 16 and any other x seam)
        seam += sum(1 for (bx, by, bz) in cells if (bx + 1, by, bz) in cells and kept[bz, by, bx] and kept[bz, by, bx + 1] and
                    ((g[:, 0] == 8 * bx + 7) & (gb[:, 1] == by) & (gb[:, 2] == bz)).any() and
                    ((g[:, 0] == 8 * bx + 8) & (gb[:, 1] == by) & (gb[:, 2] == bz)).any())
        behind += int((crossed & hit).sum())          # a ray crosses an absent brick and hits behind it
        nan_resumed += int(resumed.sum())             # a candidate whose normal is NaN: the march goes on
        later += int((resumed & hit).sum())           # ... and finds a surface further along
    assert seam > 0 and behind > 100 and nan_resumed > 100 and later > 0, (seam, behind, nan_resumed, later)


def test_sparse_world_moves_with_its_camera():
    """Between the two bases list and camera move together by whole bricks; cam2vol is then the
    same bit for bit, so the maps, the normal image and every coloured pixel are.  The Phong image
    is lit from a fixed world position and seen from the camera's, and differs."""
    a, b = (W.sparse_refs(base) for base in W.SPARSE_BASES)
    for (name, _, pa, ra), (_, _, pb, rb) in zip(a, b):
        assert not np.array_equal(pa, pb)
        assert list(ra["c2v"].R) == list(rb["c2v"].R) and list(ra["c2v"].t) == list(rb["c2v"].t), name
        for k in ("ts", "vmap", "nmap", "normal", "coloured"):
            assert same(ra[k], rb[k]), (name, k)
        assert same(ra["color"][ra["coloured"]], rb["color"][rb["coloured"]]), name


def test_clusters_are_seen_across_the_gap():
    p = W.cluster_params()
    b = W.cluster_bricks()
    origin, dims = W.default_box(b)
    assert dims == (8 * (W.CLUSTER_GAP + 6), 32, 32) and len(b) == 16
    vs = WC.voxel_size(p)
    for name, intr, pose, ref in W.cluster_refs():
        hit = ref["hit"]
        gx = np.floor(ref["P"][..., 0] / vs[0]).astype(np.int64)[hit]
        assert (gx < 32).sum() > 50 and (gx >= dims[0] - 32).sum() > 50, name  # both clusters
        _, _, crossed = _first_and_resumed(p, ref, intr, b)
        assert (crossed & hit).sum() > 30, name  # through absent cells to a surface behind them


def test_excursion_world_shows_what_the_window_lost():
    p, world, win = W.excursion_world()
    sp, _ = ST.excursion_reference()
    assert tuple(sp.origin) == (0, 0, 0) and len(world) > len(win) > 0
    vs = WC.voxel_size(p)
    for name, intr, pose, ref in W.excursion_refs():
        hit = ref["hit"]
        wx = np.floor(ref["P"][..., 0] / vs[0]).astype(np.int64) + ref["origin"][0]  # world voxel x of the hit's cell
        assert (hit & (wx >= 64)).sum() > 1000, name  # in bricks of the store, outside the window
        window = W.reference(p, win, intr, pose, box=((0, 0, 0), (64, 64, 64)))  # what kfx_render_view shows
        assert 0 < window["hit"].sum() < hit.sum(), name
