"""The references of the bricks that leave and re-enter the moving volume on the
CPU: stream_cases' numpy restatement of kfx_evict_bricks / kfx_restore_bricks against the
roll-and-clear of shift_cases, and StreamPipeline over an excursion of the window, which is the
condition that lets test_gpu_stream.py's pipeline test fail."""
import numpy as np
import pytest

import shift_cases as SC
import stream_cases as ST
from kfx import BRICK_DTYPE

DIMS = [(64, 64, 64), (128, 64, 32), (64, 40, 44)]


shift_table = ST.shift_table


def neg(s):
    return tuple(-x for x in s)


def round_trip_ref(vol, dims, s, back=None):
    """evict(s), shift(s), shift(back), restore: ((t, w, c), restored count, bricks evicted)."""
    back = neg(s) if back is None else back
    ev = ST.evict_bricks_ref(*vol, dims, (0, 0, 0), s)
    mid = SC.shift_soa(*vol, dims, s)
    end = SC.shift_soa(*mid, dims, back)
    origin = tuple(s[k] + back[k] for k in range(3))
    out, n = ST.restore_ref(*end, dims, origin, ev)
    return out, n, ev, mid


def test_brick_layout():
    assert BRICK_DTYPE.itemsize == 3600
    assert [BRICK_DTYPE.fields[k][1] for k in ("b", "reserved", "tsdf", "weight", "rgb")] == [0, 12, 16, 1040, 1552]
    dims = (16, 8, 12)
    n = int(np.prod(dims))
    a = np.arange(n, dtype=np.int32)
    b = ST.to_bricks(a, dims)
    assert b.shape == (4, 512, 1)
    # brick (cx, cy, cz) = (1, 0, 1), voxel (dx, dy, dz) = (3, 5, 2)
    assert b[2 + 1, 64 * 2 + 8 * 5 + 3, 0] == (8 + 2) * 128 + 5 * 16 + 8 + 3
    assert (b[2:, 256:] == 0).all()  # slices 12..15 do not exist
    assert np.array_equal(ST.from_bricks(b, dims), a)
    assert np.array_equal(ST.brick_coords(dims), [[0, 0, 0], [1, 0, 0], [0, 0, 1], [1, 0, 1]])


@pytest.mark.parametrize("dims", DIMS)
def test_sparse_volume_has_empty_and_barely_filled_bricks(dims):
    t, w, c = ST.sparse_volume(dims)
    ne = ST.nonempty_bricks(t, w, c, dims)
    tb, wb, cb = ST.to_bricks(t, dims), ST.to_bricks(w, dims), ST.to_bricks(c, dims, 4)
    only_c = ne & ~tb.any((1, 2)) & ~wb.any((1, 2)) & ((cb != 0).sum((1, 2)) == 1)
    only_t = ne & ~cb.any((1, 2)) & ~wb.any((1, 2)) & ((tb != 0).sum((1, 2)) == 1) & (tb.max((1, 2)) > 0)
    only_w = ne & ~cb.any((1, 2)) & ~tb.any((1, 2)) & ((wb != 0).sum((1, 2)) == 1)
    assert only_c.sum() == only_t.sum() == only_w.sum() == 1
    assert 0 < (~ne).sum() < ne.size
    X, Y, Z = dims
    assert t.size == w.size == X * Y * Z and c.size == 4 * X * Y * Z


@pytest.mark.parametrize("dims", DIMS)
def test_evict_shift_back_restore_gives_the_volume_back(dims):
    vol = ST.sparse_volume(dims)
    ne = ST.nonempty_bricks(*vol, dims)
    exact = 0
    for s in shift_table(dims):
        out, n, ev, mid = round_trip_ref(vol, dims, s)
        drop = ST.dropped_bricks(dims, s)
        assert len(ev) == n == int((drop & ne).sum()), s  # back at the origin every brick lands
        assert np.array_equal(ev["b"], ST.brick_coords(dims)[drop & ne]), s
        order = np.lexsort((ev["b"][:, 0], ev["b"][:, 1], ev["b"][:, 2]))
        assert np.array_equal(order, np.arange(len(ev))), s
        # the way back drops only voxels whose source the way out had already dropped (mid[v] = 0 wherever
        # v + s lies outside), so -s itself loses nothing and the round trip is exact for every s
        lv = SC.leaving(dims, neg(s))
        for a, per in zip(mid, (1, 1, 4)):
            assert not np.asarray(a).reshape(-1, per)[lv].any(), s
        for a, b, name in zip(out, vol, ("tsdf", "weight", "rgb")):
            assert np.array_equal(a, b), (s, name)
        exact += 1
    assert exact == len(shift_table(dims))


def test_partial_return_lands_the_nearer_layer_only():
    dims = (64, 64, 64)
    vol = ST.sparse_volume(dims)
    out, n, ev, _ = round_trip_ref(vol, dims, (16, 0, 0), back=(-8, 0, 0))
    near = ev["b"][:, 0] == 1  # world layer 1 is window layer 0 at origin (8, 0, 0)
    assert 0 < n == int(near.sum()) < len(ev)
    want, n2 = ST.restore_ref(*SC.shift_soa(*vol, dims, (8, 0, 0)), dims, (8, 0, 0), ev[near])
    assert n2 == n
    for a, b in zip(out, want):
        assert np.array_equal(a, b)
    cx = ST.brick_coords(dims)[:, 0]
    for a, b, per in zip(out, vol, (1, 1, 4)):  # layer 0 of the window holds the original's layer 1
        assert np.array_equal(ST.to_bricks(a, dims, per)[cx == 0], ST.to_bricks(b, dims, per)[cx == 1])


def test_excursion_tracks_and_restores():
    sp, _ = ST.excursion_reference()
    print(f"excursion {ST.EXCURSION}: {sp.n_out} bricks out, {sp.n_in} restored, {len(sp.store)} held")
    assert sp.frame_count == 13 and len(sp.poses) == 12  # all 12 frames tracked
    assert sp.n_out >= 1 and sp.n_in >= 1
    assert sp.origin == (0, 0, 0)


def test_restore_changes_what_the_tracker_sees():
    """The condition that makes test_gpu_stream.py's excursion test able to fail: with the
    re-entered slab left empty, frame 8's level-0 model map and the final volume differ."""
    sp, pv8 = ST.excursion_reference()
    lossy, lv8 = ST.excursion_reference(stream=False)
    differ = (np.nan_to_num(pv8).view(np.uint32) != np.nan_to_num(lv8).view(np.uint32)).any(-1)
    nt = int((sp.vol.tsdf != lossy.vol.tsdf).sum())
    print(f"frame 8 model map: {int(differ.sum())} pixels differ; final volume: {nt} tsdf values differ")
    assert differ.sum() > 0 and nt > 0
    assert not np.array_equal(sp.pose_matrices().view(np.uint32), lossy.pose_matrices().view(np.uint32))


def test_free_space_excursion_tracks():
    """(0, 0, 8) and back: the bricks in front of the scene, which hold no negative tsdf."""
    sp, _ = ST.excursion_reference(ST.FREE_EXCURSION)
    print(f"excursion {ST.FREE_EXCURSION}: {sp.n_out} bricks out, {sp.n_in} restored")
    assert sp.frame_count == 13 and sp.n_out >= 1 and sp.n_in >= 1
    bgr, dep, _ = SC.frames(12)
    ref = ST.StreamPipeline(SC.qvga(), SC.params(64))
    for k in range(4):
        assert ref.process(bgr[k], dep[k]) == 0
    ev = ST.evict_bricks_ref(*ref.volume(), ref.dims, ref.origin, ST.FREE_EXCURSION)
    assert len(ev) >= 1 and (ev["tsdf"] >= 0).all()
