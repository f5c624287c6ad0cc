"""References of the world map, shared by test_world_restatement.py (CPU) and
test_gpu_world.py.

The reference of kfx_world_points_attr / kfx_world_mesh_attr is extract_cases' numpy restatement
run on the dense bounding box of the bricks, absent bricks zero-filled (weight 0: unobserved), at
the context's voxel size and creation pose.  For the points the box is padded by one empty brick
layer at high z, so that the slice FullScan6 never visits holds nothing; the cubes that reach out
of the box would read absent bricks and yield nothing, so the mesh needs no padding.  The
restatement's canonical order (z // 8, tile, z & 7, lane, minor) is the world order (brick, dz,
lane, minor) for a box of bricks.  Positions are checked against the oracle as EC.restate does;
for a box whose base is not 0 only xyz is recomputed, from the world index."""
import functools

import numpy as np

import extract_cases as EC
import oracle as O
import stream_cases as ST
from kfx import BRICK_DTYPE
from kfx.abi import Pose

f32 = np.float32


def voxel_size(p):
    """vs_k = volu_range[k] / (float)volu_dims[k] of a context's parameters."""
    return (np.array([p.volu_range[k] for k in range(3)], f32) /
            np.array([int(p.volu_dims[k]) for k in range(3)], np.int32).astype(f32)).astype(f32)


def rgba(rgb):
    """(N, 3) colours -> the flat (4N,) bytes stream_cases' brick helpers take."""
    c = np.zeros((len(rgb), 4), np.uint8)
    c[:, :3] = rgb
    return c.reshape(-1)


def brick_mask_to_voxels(keep, box):
    """(bricks,) bool in to_bricks' order -> (Z*Y*X,) bool."""
    b = np.broadcast_to(np.asarray(keep, bool)[:, None, None], (len(keep), 512, 1))
    return ST.from_bricks(np.ascontiguousarray(b), box).astype(bool)


def zero_absent(t, w, rgb, box, keep):
    """The arrays with every voxel of a brick outside `keep` unobserved (0, 0, 0)."""
    m = brick_mask_to_voxels(keep, box)
    return np.where(m, t, 0).astype(np.int16), np.where(m, w, 0).astype(np.int16), np.where(m[:, None], rgb, 0).astype(np.uint8)


def bricks_of(t, w, rgb, box, keep, base=(0, 0, 0)):
    """The bricks `keep` of the box as (N,) BRICK_DTYPE, ascending, at world brick base `base`."""
    keep = np.asarray(keep, bool)
    out = np.zeros(int(keep.sum()), BRICK_DTYPE)
    out["b"] = ST.brick_coords(box)[keep] + np.array(base, np.int64)
    out["tsdf"] = ST.to_bricks(t, box)[keep, :, 0]
    out["weight"] = ST.to_bricks(w, box)[keep, :, 0]
    out["rgb"] = ST.to_bricks(rgba(rgb), box, 4)[keep]
    return out


def box_of(bricks):
    """The dense bounding box of (N,) BRICK_DTYPE bricks: (base bricks, box dims, t, w, rgb (N, 3)),
    absent bricks zero-filled."""
    b = np.asarray(bricks["b"], np.int64)
    base = b.min(0)
    nb = b.max(0) - base + 1
    box = tuple(int(8 * n) for n in nb)
    n = int(np.prod(nb))
    tb, wb, cb = np.zeros((n, 512, 1), np.int16), np.zeros((n, 512, 1), np.int16), np.zeros((n, 512, 4), np.uint8)
    q = b - base
    i = (q[:, 2] * nb[1] + q[:, 1]) * nb[0] + q[:, 0]
    tb[i, :, 0], wb[i, :, 0], cb[i] = bricks["tsdf"], bricks["weight"], bricks["rgb"]
    c = ST.from_bricks(cb, box, 4).reshape(-1, 4)[:, :3]
    return tuple(int(x) for x in base), box, ST.from_bricks(tb, box), ST.from_bricks(wb, box), c


def vol_at(p, box, t, w, rgb) -> EC.Vol:
    """The restatement's view of a box at the context's voxel size and creation pose."""
    v = EC.Vol(box, (1.0, 1.0, 1.0), p.volu_pose, t, w, rgba(rgb).reshape(-1, 4))
    v.vs = voxel_size(p)
    return v


def pad_top(box, t, w, rgb):
    """One empty brick layer at high z."""
    X, Y, Z = box
    n = 8 * X * Y
    return ((X, Y, Z + 8), np.concatenate([t, np.zeros(n, np.int16)]), np.concatenate([w, np.zeros(n, np.int16)]),
            np.concatenate([rgb, np.zeros((n, 3), np.uint8)]))


def vertices_at(v: EC.Vol, e, base=(0, 0, 0)):
    """EC.vertices of the edges e with the position recomputed from the world index w = 8 base +
    (x, y, z): V_k = ((float)w_k + 0.5f) * vs_k, the interpolation of extract_voxel, p = R V + t."""
    out = EC.vertices(v, e)
    x, y, z, axis = e.T
    xb, yb, zb = x + (axis == 0), y + (axis == 1), z + (axis == 2)
    Fa, Fb = v.F[z, y, x], v.F[zb, yb, xb]
    V = [((c + 8 * int(base[k])).astype(np.int32).astype(f32) + f32(0.5)) * v.vs[k] for k, c in enumerate((x, y, z))]
    Va = np.choose(axis, V)
    Vn = Va + v.vs[axis]
    d_inv = f32(1) / (np.abs(Fa) + np.abs(Fb))
    cc = (Va * np.abs(Fb) + Vn * np.abs(Fa)) * d_inv
    pt = [np.where(axis == k, cc, V[k]).astype(f32) for k in range(3)]
    wv = EC._rmul(v.R, pt)
    out["xyz"] = np.stack([wv[k] + v.t[k] for k in range(3)], 1)
    return out


def reference(p, box, t, w, rgb, base=(0, 0, 0)):
    """(points (N,), triangles (M, 3), point edges, triangle edges) of the world whose bounding box
    holds the arrays t, w, rgb (absent bricks zero-filled) at world brick base `base`.  The edges are
    (x, y, z, axis) rows in box coordinates."""
    tab = EC.check_edge_numbering()
    v = vol_at(p, box, t, w, rgb)
    vp = vol_at(p, *pad_top(box, t, w, rgb))
    pe, te = EC.point_edges(vp), EC.mesh_edges(v, tab)
    # the oracle sees the padded volume for the points (it too skips the top slice) and the box for the mesh
    p0, t0 = EC.vertices(vp, pe), EC.vertices(v, te).reshape(-1, 3)
    ovol = O.Volume(vp.dims, (1.0, 1.0, 1.0))
    ovol.voxel_size = np.array(vp.vs, f32)
    pose = Pose()
    pose.R[:], pose.t[:] = [float(a) for a in v.R], [float(a) for a in v.t]
    op, n = O.extract_points(ovol, pose, tsdf=vp.q.ravel(), weight=vp.w.ravel())
    assert n == len(op) == len(p0) and np.array_equal(p0["xyz"].view(np.uint32), op.view(np.uint32))
    ovol = O.Volume(v.dims, (1.0, 1.0, 1.0))
    ovol.voxel_size = np.array(v.vs, f32)
    om, n = O.extract_mesh(ovol, pose, tsdf=v.q.ravel(), weight=v.w.ravel())
    assert n == len(om) == len(t0) and np.array_equal(t0["xyz"].view(np.uint32), om.view(np.uint32))
    if not any(base):
        return p0, t0, pe, te
    return vertices_at(vp, pe, base), vertices_at(v, te, base).reshape(-1, 3), pe, te


def reference_of_bricks(p, bricks):
    """reference() of a brick list (its bounding box, its own base)."""
    base, box, t, w, rgb = box_of(bricks)
    return reference(p, box, t, w, rgb, base)


def seam_edges(e):
    """(N,) bool: the edges a -> b = a + e_axis whose ends lie in two bricks."""
    return e[np.arange(len(e)), e[:, 3]] % 8 == 7


# ---- the cases ---------------------------------------------------------------------

def window_params():
    """The small window context the list tests run on: extract_cases' rotated pose and three
    different voxel sizes (20 x 15 x 30 mm)."""
    return EC.params_for((32, 24, 16))


SPARSE_BOX = (40, 32, 24)  # 5 x 4 x 3 bricks
SPARSE_BASES = ((0, 0, 0), (-2, 1, -3))


@functools.lru_cache(maxsize=None)
def sparse_world(seed=11):
    """EC.dense at SPARSE_BOX with about half of the bricks taken out by a seeded mask, as
    stream_cases.sparse_volume does: (keep, t, w, rgb) with the absent bricks zero-filled."""
    t, w, rgb = EC.dense(SPARSE_BOX)
    n = int(np.prod(ST.brick_counts(SPARSE_BOX)))
    keep = np.random.default_rng(seed).integers(0, 2, n).astype(bool)
    t, w, rgb = zero_absent(t, w, rgb, SPARSE_BOX, keep)
    for a in (keep, t, w, rgb):
        a.setflags(write=False)
    return keep, t, w, rgb


def absent_face_neighbours(keep, box):
    """Per face direction (-x, +x, -y, +y, -z, +z): kept bricks whose neighbour there lies inside the
    box and is absent."""
    nx, ny, nz = ST.brick_counts(box)
    k = np.asarray(keep, bool).reshape(nz, ny, nx)
    out = []
    for axis in (2, 1, 0):  # x, y, z of the (z, y, x) array
        for s in (-1, 1):
            a = [slice(None)] * 3
            b = [slice(None)] * 3
            a[axis] = slice(1, None) if s < 0 else slice(0, -1)
            b[axis] = slice(0, -1) if s < 0 else slice(1, None)
            out.append(int((k[tuple(a)] & ~k[tuple(b)]).sum()))
    return out


NEIGH_BOX = (24, 24, 24)  # 3 x 3 x 3 bricks
# negatives at the centre brick's 8 corners and one inside it
NEIGH_NEG = tuple((8 + lx, 8 + ly, 8 + lz) for lx, ly, lz in EC.ISOLATED_LOCAL)


def neigh_world(removed=None):
    """EC.isolated on 3 x 3 x 3 bricks, brick index `removed` (0..26, not the centre 13) absent:
    (keep, t, w, rgb)."""
    t, w, rgb = EC.isolated(NEIGH_BOX, NEIGH_NEG)
    keep = np.ones(27, bool)
    if removed is not None:
        assert removed != 13
        keep[removed] = False
    return (keep,) + zero_absent(t, w, rgb, NEIGH_BOX, keep)
