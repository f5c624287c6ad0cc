"""The volumes of extract_cases.py, on the CPU: the restatement holds on each of them (restate()
compares its positions with the oracle's extraction bit for bit), and each holds what
test_gpu_extract_paths.py uses it for."""
import numpy as np
import pytest

import extract_cases as EC
import shift_cases as SC


def test_dense_is_the_crafted_recipe(oracle_lib):
    t, w, rgb = EC.dense(EC.CRAFT_DIMS)
    rec = EC.crafted_records()
    assert np.array_equal(t, rec["tsdf"]) and np.array_equal(w, rec["weight"]) and np.array_equal(rgb, rec["rgb"])
    assert EC.records(t, w, rgb).tobytes() == rec.tobytes()
    _, _, v, pts, tri = EC.reference("dense", EC.CRAFT_DIMS)
    assert len(pts) > 1000 and len(tri) > 1000
    p0 = EC.crafted_params()
    assert bytes(EC.params_for(EC.CRAFT_DIMS)) == bytes(p0)


@pytest.mark.parametrize("name", ["dense", "scene"])
def test_sweep_volumes(oracle_lib, name):
    """136 x 120 x 42: every brick of `dense` holds a negative (no wave skips), most of `scene`'s
    hold none; both have items in the last chunk's single slice."""
    p, rec, v, pts, tri = EC.reference(name, EC.SWEEP_DIMS)
    X, Y, Z = EC.SWEEP_DIMS
    assert (X // 8) * (Y // 8) == 255 and Z - 1 == 5 * 8 + 1
    assert len(pts) > 5000 and len(tri) > 5000
    assert len(set(v.vs.tolist())) == 3 and not np.array_equal(v.R, np.eye(3, dtype=np.float32).ravel())
    e = EC.point_edges(v)
    assert (e[:, 2] == Z - 2).any()  # the last chunk's only slice
    chunk_set, clear = EC.tile_classes(EC.SWEEP_DIMS, rec["tsdf"])
    print(f"{name}: {len(pts)} points, {len(tri)} triangles, {chunk_set.mean():.3f} of the bricks set, "
          f"{clear.mean():.3f} of the tiles certainly clear")
    if name == "dense":
        assert chunk_set.all() and not clear.any()
    else:
        assert chunk_set.mean() < 0.5 and clear.any()
        assert (rec["weight"] == 0).mean() > 0.03 and (rec["rgb"] == 0).all(1).mean() > 0.15
        assert (rec["tsdf"] == 32767).mean() > 0.5 and not (rec["tsdf"] == 0).any()


@pytest.mark.parametrize("K", EC.UNITS)
def test_scene_mixes_clear_and_set_tiles_in_a_wave(K):
    """For every forced K, some wave's K consecutive tiles of one chunk hold a tile that is
    certainly clear and one that is certainly set: the lane-per-unit test, the ballot loop and
    the zero count of a clear unit all run in one wave.  (K = 1: a wave has one tile, so the two
    kinds can only meet in one chunk, in different waves.)"""
    t = EC.scene(EC.SWEEP_DIMS)[0]
    if K == 1:
        chunk_set, clear = EC.tile_classes(EC.SWEEP_DIMS, t)
        assert clear.any() and chunk_set.any(1).any()
        return
    groups = EC.mixed_groups(EC.SWEEP_DIMS, t, K)
    print(f"K = {K}: {len(groups)} mixed groups, first {groups[:3]}")
    assert len(groups) >= 1
    assert 255 % K  # the last wave is ragged (`dense` gives every one of its tiles work)


def test_scan_volume(oracle_lib):
    """256 x 128 x 136: 8704 units = three blocks of the offset scan, with items in each block."""
    _, _, v, pts, tri = EC.reference("scene", EC.SCAN_DIMS)
    X, Y, Z = EC.SCAN_DIMS
    ntiles, nchunks = (X // 8) * (Y // 8), (Z - 1 + 7) // 8
    assert ntiles * nchunks == 8704 and (8704 + 4095) // 4096 == 3
    for items in (EC.point_edges(v), EC.mesh_edges(v, EC.check_edge_numbering())[::3]):
        unit = (items[:, 2] // 8) * ntiles + (items[:, 1] // 8) * (X // 8) + items[:, 0] // 8
        assert set(np.unique(unit // 4096)) == {0, 1, 2}
    assert len(pts) > 10000 and len(tri) > 10000


def _counts_at(v, positions):
    """Points and triangles per listed negative: the items with an edge end / a vertex on an edge from there."""
    e = EC.point_edges(v)
    x, y, z, axis = e.T
    b = np.stack([x + (axis == 0), y + (axis == 1), z + (axis == 2)], 1)
    m = EC.mesh_edges(v, EC.check_edge_numbering())
    mb = np.stack([m[:, 0] + (m[:, 3] == 0), m[:, 1] + (m[:, 3] == 1), m[:, 2] + (m[:, 3] == 2)], 1)
    out = []
    for pos in positions:
        pos = np.array(pos)
        npts = int(((e[:, :3] == pos).all(1) | (b == pos).all(1)).sum())
        verts = (m[:, :3] == pos).all(1) | (mb == pos).all(1)
        out.append((npts, int(verts.reshape(-1, 3).any(1).sum())))
    return out


def test_isolated_volumes(oracle_lib):
    dims = EC.ISOLATED_DIMS
    p = EC.params_for(dims)
    inner, border = EC.isolated_interior(), EC.isolated_border()
    assert len(inner) == 9 and sorted((x & 7, y & 7, z & 7) for x, y, z in inner) == sorted(EC.ISOLATED_LOCAL)
    bricks = np.array([(x >> 3, y >> 3, z >> 3) for x, y, z in inner])
    for i in range(len(bricks)):  # alone in the 5 x 5 x 5 brick neighbourhood, whose inner 3 x 3 x 3 is inside
        d = np.abs(bricks - bricks[i]).max(1)
        assert (np.delete(d, i) >= 3).all()
        assert (bricks[i] >= 1).all() and (8 * (bricks[i] + 2) <= np.array(dims)).all()
    v = EC.volume(p, *EC.isolated(dims, inner))
    pts, tri = EC.restate(v)
    assert _counts_at(v, inner) == [(6, 8)] * 9
    assert len(pts) == 54 and len(tri) == 72
    # ISOLATED_SHIFT and back: the rim returns unobserved, the negatives with all their neighbours
    s = EC.ISOLATED_SHIFT
    there = SC.shift_soa(v.q.ravel(), v.w.ravel(), np.zeros(4 * v.q.size, np.uint8), dims, s)
    t2, w2, _ = SC.shift_soa(*there, dims, tuple(-x for x in s))
    assert (w2 == 0).any() and np.array_equal(np.nonzero(t2 < 0)[0], np.nonzero(v.q.ravel() < 0)[0])
    v2 = EC.volume(p, t2, w2, EC.isolated(dims, inner)[2])
    assert _counts_at(v2, inner) == [(6, 8)] * 9
    v = EC.volume(p, *EC.isolated(dims, border))
    pts, tri = EC.restate(v)
    counts = _counts_at(v, border)
    print("border negatives (points, triangles):", counts)
    # A corner voxel keeps its three inward edges and one cube; (0, 0, Z - 2) has a fourth edge and
    # a second cube above it.  The last two are neighbours along z: no crossing between them, the
    # slice z = Z - 1 is never visited for points, and the top cube cuts both off with one quad.
    assert counts == [(3, 1), (3, 1), (3, 1), (4, 2), (3, 3), (0, 2)]
    assert len(pts) == 16 and len(tri) == 8
