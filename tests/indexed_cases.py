"""The indexed mesh's reference, shared by test_indexed_cases.py (CPU) and
test_gpu_indexed.py.

The reference is built from extract_cases' restatement of the triangle soup, which is checked
against the oracle: the distinct (x, y, z, axis) rows of EC.mesh_edges are the vertices, ordered by
the canonical position of the owner voxel, and a triangle corner's index is its row's rank.  The
used-edge predicate of include/kfx.h is restated here on its own (used_edges) and must give the
same set.  The world form works on the dense bounding box with absent bricks zeroed, as
world_cases.reference does: an absent brick owns no used edge, so the dense canonical order
restricted to the listed bricks is the list order."""
import collections
import functools

import numpy as np

import extract_cases as EC
import world_cases as WC

Indexed = collections.namedtuple("Indexed", "verts tris edges corner_edges")
CLASSES = ("x", "y", "z", "xy", "xz", "yz")  # a corner's owner brick minus its cube's brick


def edge_rank_key(v: EC.Vol, e):
    """A scalar that ascends with EC._canonical(x, y, z, axis)."""
    x, y, z, axis = (e[:, k].astype(np.int64) for k in range(4))
    ntiles = (v.dims[0] // 8) * (v.dims[1] // 8)
    tile = (y // 8) * (v.dims[0] // 8) + x // 8
    return ((((z // 8) * ntiles + tile) * 8 + (z & 7)) * 64 + (y & 7) * 8 + (x & 7)) * 3 + axis


def reference(v: EC.Vol, base=None) -> Indexed:
    """verts (V,), tris (T, 3) uint32, the vertices' edges (V, 4) and the soup's (3T, 4)."""
    tab = EC.check_edge_numbering()
    ce = EC.mesh_edges(v, tab)
    if len(ce) == 0:
        return Indexed(np.zeros(0, EC.VDT), np.zeros((0, 3), np.uint32), np.zeros((0, 4), np.int64), ce)
    ue = np.unique(ce, axis=0)
    ue = ue[EC._canonical(v, ue[:, 0], ue[:, 1], ue[:, 2], ue[:, 3])]
    key = edge_rank_key(v, ue)
    assert np.all(np.diff(key) > 0)
    verts = EC.vertices(v, ue) if base is None else WC.vertices_at(v, ue, base)
    ck = edge_rank_key(v, ce)
    tris = np.searchsorted(key, ck)
    assert np.array_equal(key[tris], ck)
    return Indexed(verts, tris.astype(np.uint32).reshape(-1, 3), ue, ce)


def used_edges(v: EC.Vol):
    """The used-edge predicate of include/kfx.h, (N, 4) rows (x, y, z, axis) sorted as np.unique sorts:
    the ends differ in sign and one of the up to four cubes around the edge is complete."""
    X, Y, Z = v.dims
    w = v.w > 0
    comp = np.ones((Z - 1, Y - 1, X - 1), bool)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
        comp &= w[dz:Z - 1 + dz, dy:Y - 1 + dy, dx:X - 1 + dx]
    cp = np.zeros((Z + 1, Y + 1, X + 1), bool)  # cp[z + 1, y + 1, x + 1] = cube (x, y, z) is complete; False outside
    cp[1:Z, 1:Y, 1:X] = comp
    neg = v.F < 0
    out = []
    for axis in range(3):
        ar = 2 - axis  # the array axis
        n = [Z, Y, X]
        n[ar] -= 1     # b = a + e_axis exists
        a = tuple(slice(0, m) for m in n)
        b = tuple(slice(int(k == ar), m + int(k == ar)) for k, m in enumerate(n))
        cross = neg[a] != neg[b]
        around = np.zeros_like(cross)
        others = [k for k in range(3) if k != ar]
        for s in (0, 1):
            for t in (0, 1):
                off = [1, 1, 1]  # cp's offset; the cube at a - s e_j - t e_k
                off[others[0]] -= s
                off[others[1]] -= t
                around |= cp[tuple(slice(o, o + m) for o, m in zip(off, n))]
        z, y, x = np.nonzero(cross & around)
        out.append(np.stack([x, y, z, np.full(len(x), axis)], 1))
    e = np.concatenate(out).astype(np.int64)
    return np.unique(e, axis=0) if len(e) else e


def corner_classes(v: EC.Vol):
    """Per class of CLASSES: the triangle corners whose owner voxel lies in the brick at that offset
    from the brick of the corner's cube.  Restates EC.mesh_edges with the cube kept."""
    tab = EC.check_edge_numbering()
    X, Y, Z = v.dims
    cfg = np.zeros((Z - 1, Y - 1, X - 1), np.int64)
    ok = np.ones(cfg.shape, bool)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
        s = (slice(dz, Z - 1 + dz), slice(dy, Y - 1 + dy), slice(dx, X - 1 + dx))
        ok &= v.w[s] > 0
        cfg |= (v.F[s] < 0).astype(np.int64) << c
    nt = np.where(ok, tab[cfg, 0].astype(np.int64), 0)
    z, y, x = np.nonzero(nt)
    n = nt[z, y, x]
    cube = np.repeat(np.arange(len(z)), 3 * n)
    k = np.arange(len(cube)) - np.repeat(np.cumsum(3 * n) - 3 * n, 3 * n)
    e = tab[cfg[z, y, x][cube], 1 + k].astype(np.int64)
    lo = EC.LOWER[e >> 2, e & 3]
    q = np.stack([x[cube], y[cube], z[cube]], 1)
    o = q + np.stack([lo & 1, (lo >> 1) & 1, lo >> 2], 1)
    own = np.stack([o[:, 0], o[:, 1], o[:, 2], e >> 2], 1)
    order = EC._canonical(v, q[:, 0], q[:, 1], q[:, 2], k)
    assert np.array_equal(own[order], EC.mesh_edges(v, tab))  # the same corners
    d = o // 8 - q // 8
    assert d.min(initial=0) >= 0 and d.max(initial=0) <= 1 and not (d.sum(1) == 3).any()
    return {name: int((d == [int(c in name) for c in "xyz"]).all(1).sum()) for name in CLASSES}


def equal_pairs(verts):
    """Distinct vertices (edges) that hold the same 28 bytes."""
    raw = np.ascontiguousarray(verts).view(np.uint8).reshape(len(verts), -1)
    return len(raw) - len(np.unique(raw, axis=0))


# ---- the cases -----------------------------------------------------------------------

def vol_of(builder, dims, pose=None) -> EC.Vol:
    t, w, rgb = builder(tuple(dims)) if callable(builder) else builder
    return EC.volume(EC.params_for(dims), t, w, rgb, pose)


@functools.lru_cache(maxsize=None)
def window_case(name, dims):
    """(params, records, Vol, Indexed) of EC.dense / EC.scene / the isolated volumes at dims."""
    dims = tuple(dims)
    if name in ("dense", "scene"):
        t, w, rgb = {"dense": EC.dense, "scene": EC.scene}[name](dims)
    else:
        pos = {"interior": EC.isolated_interior, "border": EC.isolated_border}[name](dims)
        t, w, rgb = EC.isolated(dims, pos)
    p = EC.params_for(dims)
    v = EC.volume(p, t, w, rgb)
    return p, EC.records(t, w, rgb), v, reference(v)


def world_reference(p, box, t, w, rgb, base=(0, 0, 0)) -> Indexed:
    """reference() of a world whose bounding box holds t, w, rgb (absent bricks zero-filled)."""
    return reference(WC.vol_at(p, box, t, w, rgb), base)


def world_reference_of_bricks(p, bricks) -> Indexed:
    base, box, t, w, rgb = WC.box_of(bricks)
    return world_reference(p, box, t, w, rgb, base)


# every window fixture test_gpu_indexed.py uploads: (builder name, dims)
DEPTHS = (9, 13, 41)
WINDOW_FIXTURES = ([("dense", EC.CRAFT_DIMS), ("scene", (40, 32, 24))] + [("dense", (24, 16, z)) for z in DEPTHS] +
                   [("dense", EC.SWEEP_DIMS), ("scene", EC.SWEEP_DIMS), ("scene", EC.SCAN_DIMS),
                    ("interior", EC.ISOLATED_DIMS), ("border", EC.ISOLATED_DIMS)])


def ply_text(verts, tris):
    """kfx_write_ply_mesh_indexed's file."""
    head = ("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\n"
            "property uchar blue\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n") % (len(verts), len(tris))
    lines = ["%g %g %g %g %g %g %d %d %d\n" % (*v["xyz"], *v["normal"], v["bgra"][2], v["bgra"][1], v["bgra"][0]) for v in verts]
    lines += ["3 %d %d %d\n" % tuple(t) for t in np.asarray(tris).reshape(-1, 3)]
    return head + "".join(lines)
