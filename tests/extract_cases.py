"""The extraction's numpy restatement and the volumes it is run on, shared by
test_gpu_extract_attr.py, test_extract_cases.py (CPU) and test_gpu_extract_paths.py.

The restatement follows the definitions in include/kfx.h.  The oracle has no
colours or normals, so the restatement is first checked against it where it
can be: its positions must equal O.extract_points / O.extract_mesh bit for bit
(which fixes the canonical order, the triangle table and the edge numbering);
the normals and colours are then compared bit for bit with the library's, from
the same volume."""
import functools

import numpy as np

import oracle as O
from kfx import VERTEX_DTYPE
from kfx.abi import Pose, default_params

f32 = np.float32
DIV = f32(0.0000305185)  # kDivShortMax
VDT = np.dtype(VERTEX_DTYPE)
# lower corners of the 4 edges of an axis, ascending (corner = dx | dy << 1 | dz << 2)
LOWER = np.array([[0, 2, 4, 6], [0, 1, 4, 5], [0, 1, 2, 3]])


# ---- the restatement ---------------------------------------------------------

class Vol:
    """A downloaded volume: tsdf / weight int16 and the 24-bit packed colour, [z, y, x]."""

    def __init__(self, dims, range_m, pose: Pose, t, w, c):
        X, Y, Z = (int(d) for d in dims)
        self.dims = (X, Y, Z)
        self.range = tuple(float(r) for r in range_m)
        self.vs = (np.array(range_m, f32) / np.array(dims, np.int32).astype(f32)).astype(f32)
        self.R = np.array(pose.R[:], f32)
        self.t = np.array(pose.t[:], f32)
        self.q = np.asarray(t, np.int16).reshape(Z, Y, X)
        self.w = np.asarray(w, np.int16).reshape(Z, Y, X)
        c = np.asarray(c, np.uint8).reshape(Z, Y, X, 4).astype(np.int64)
        self.c = c[..., 0] | (c[..., 1] << 8) | (c[..., 2] << 16)
        self.F = self.q.astype(f32) * DIV


def _canonical(v: Vol, x, y, z, *minor):
    """Order of the items: (z // 8, tile, z & 7, lane, minor keys...)."""
    tile = (y // 8) * (v.dims[0] // 8) + x // 8
    lane = (y & 7) * 8 + (x & 7)
    return np.lexsort(tuple(reversed((z // 8, tile, z & 7, lane) + minor)))


def point_edges(v: Vol):
    """(x, y, z, axis) of every FullScan6 crossing, canonical order."""
    X, Y, Z = v.dims
    ok = (v.w != 0) & (v.F != f32(1))
    out = []
    for axis in range(3):
        hi = [Z - 1, Y, X]  # the + neighbour must exist (z + 1 always: z < Z - 1)
        if axis < 2:
            hi[2 - axis] -= 1
        a = (slice(0, hi[0]), slice(0, hi[1]), slice(0, hi[2]))
        sh = [0, 0, 0]
        sh[2 - axis] = 1
        b = tuple(slice(s.start + d, s.stop + d) for s, d in zip(a, sh))
        Fa, Fb = v.F[a], v.F[b]
        hit = ok[a] & ok[b] & (((Fa > 0) & (Fb < 0)) | ((Fa < 0) & (Fb > 0)))
        z, y, x = np.nonzero(hit)
        out.append(np.stack([x, y, z, np.full(len(x), axis)], 1))
    e = np.concatenate(out).astype(np.int64)
    return e[_canonical(v, e[:, 0], e[:, 1], e[:, 2], e[:, 3])]


def mesh_edges(v: Vol, tab):
    """(x, y, z, axis) of voxel a of every triangle vertex, canonical order, 3 rows per triangle."""
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
    first = np.repeat(np.cumsum(3 * n) - 3 * n, 3 * n)
    k = np.arange(len(cube)) - first  # 3 * triangle + vertex
    e = tab[cfg[z, y, x][cube], 1 + k].astype(np.int64)
    axis = e >> 2
    lo = LOWER[axis, e & 3]
    xa, ya, za = x[cube] + (lo & 1), y[cube] + ((lo >> 1) & 1), z[cube] + (lo >> 2)
    order = _canonical(v, x[cube], y[cube], z[cube], k)
    return np.stack([xa, ya, za, axis], 1)[order]


def _rmul(R, p):
    return [R[3 * i] * p[0] + R[3 * i + 1] * p[1] + R[3 * i + 2] * p[2] for i in range(3)]


def _gradient(v: Vol, x, y, z):
    q = [x, y, z]
    Fq = v.F[z, y, x]
    g = []
    for k in range(3):
        side = []
        for s in (1, -1):
            n = list(q)
            n[k] = q[k] + s
            inside = (n[k] >= 0) & (n[k] < v.dims[k])
            n[k] = np.clip(n[k], 0, v.dims[k] - 1)
            valid = inside & (v.w[n[2], n[1], n[0]] != 0)
            side.append((valid, np.where(valid, v.F[n[2], n[1], n[0]], Fq)))
        (vh, hi), (vl, lo) = side
        d = hi - lo
        d = np.where(vh ^ vl, d * f32(2), d)
        g.append((d / v.vs[k]).astype(f32))
    return g


def vertices(v: Vol, e):
    """kfx_vertex records of the edges e = (x, y, z, axis) rows (voxel a, b = a + e_axis)."""
    x, y, z, axis = e.T
    xb, yb, zb = x + (axis == 0), y + (axis == 1), z + (axis == 2)
    out = np.zeros(len(e), VDT)
    Fa, Fb = v.F[z, y, x], v.F[zb, yb, xb]
    # position: the plain calls' arithmetic
    V = [(c.astype(f32) + f32(0.5)) * v.vs[k] for k, c in enumerate((x, y, z))]
    Va = np.choose(axis, V)
    Vn = Va + v.vs[axis]
    d_inv = f32(1) / (np.abs(Fa) + np.abs(Fb))
    cc = (Va * np.abs(Fb) + Vn * np.abs(Fa)) * d_inv
    p = [np.where(axis == k, cc, V[k]).astype(f32) for k in range(3)]
    w = _rmul(v.R, p)
    out["xyz"] = np.stack([w[k] + v.t[k] for k in range(3)], 1)
    # normal
    ga, gb = _gradient(v, x, y, z), _gradient(v, xb, yb, zb)
    m = [ga[k] * np.abs(Fb) + gb[k] * np.abs(Fa) for k in range(3)]
    w = _rmul(v.R, m)
    l = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    assert l.dtype == f32
    with np.errstate(invalid="ignore", divide="ignore"):
        out["normal"] = np.stack([np.where(l == 0, f32(0), w[k] / l) for k in range(3)], 1)
    # colour
    ta, tb = np.abs(v.q[z, y, x].astype(np.int64)), np.abs(v.q[zb, yb, xb].astype(np.int64))
    assert np.all(ta + tb > 0)
    ca, cb = v.c[z, y, x], v.c[zb, yb, xb]
    both, one = (ca != 0) & (cb != 0), (ca != 0) ^ (cb != 0)
    for j in range(3):
        aj, bj = (ca >> (8 * j)) & 255, (cb >> (8 * j)) & 255
        blend = (aj * tb + bj * ta + ((ta + tb) >> 1)) // (ta + tb)
        out["bgra"][:, j] = np.where(both, blend, np.where(one, aj | bj, 0))
    out["bgra"][:, 3] = np.where(both | one, 255, 0)
    return out


def check_edge_numbering():
    """O.mc_table() is the triangle table; an edge e has axis e >> 2 and its
    lower corner is the (e & 3)-th corner, ascending, with the axis bit clear."""
    tab = O.mc_table()
    assert tab.shape == (256, 16) and tab[0, 0] == 0 and tab[255, 0] == 0 and int(tab[:, 0].max()) <= 5
    assert int(tab[:, 1:].max()) == 11
    for axis in range(3):
        assert list(LOWER[axis]) == [c for c in range(8) if not (c >> axis) & 1]
    return tab


def restate(v: Vol):
    """(points (N,), triangles (M, 3)) of the restatement, after checking its
    positions against the oracle's extraction of the same volume."""
    tab = check_edge_numbering()
    ovol = O.Volume(v.dims, v.range)
    assert np.array_equal(ovol.voxel_size, v.vs)
    pose = Pose()
    pose.R[:], pose.t[:] = [float(a) for a in v.R], [float(a) for a in v.t]
    t, w = v.q.ravel(), v.w.ravel()
    pts = vertices(v, point_edges(v))
    op, n = O.extract_points(ovol, pose, tsdf=t, weight=w)
    assert n == len(op) == len(pts)
    assert np.array_equal(pts["xyz"].view(np.uint32), op.view(np.uint32))
    tri = vertices(v, mesh_edges(v, tab)).reshape(-1, 3)
    om, n = O.extract_mesh(ovol, pose, tsdf=t, weight=w)
    assert n == len(om) == len(tri)
    assert np.array_equal(tri["xyz"].view(np.uint32), om.view(np.uint32))
    return pts, tri


def same(a, b):
    """Records equal byte for byte."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype == VDT and a.shape == b.shape and a.tobytes() == b.tobytes()


def first_difference(a, b):
    if a.shape != b.shape:
        return "shapes %s %s" % (a.shape, b.shape)
    a, b = a.ravel(), b.ravel()
    for f in ("xyz", "normal", "bgra"):
        bad = np.nonzero((a[f].view(np.uint8).reshape(len(a), -1) != b[f].view(np.uint8).reshape(len(b), -1)).any(1))[0]
        if len(bad):
            return "%s: %d of %d differ, first at %d: %s vs %s" % (f, len(bad), len(a), bad[0], a[f][bad[0]], b[f][bad[0]])
    return "equal"


# ---- the crafted volume ----------------------------------------------------------

CRAFT_DIMS, CRAFT_RANGE = (32, 24, 16), (0.64, 0.36, 0.48)


def crafted_params():
    p = default_params(dims=32, range_m=0.64)
    for i in range(3):
        p.volu_dims[i] = CRAFT_DIMS[i]
        p.volu_range[i] = CRAFT_RANGE[i]
    a, b = 0.3, -0.2  # a rotated, shifted volume pose: R is not the identity
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    m = np.eye(4)
    m[:3, :3] = Rz @ Rx
    m[:3, 3] = [-0.3, 0.1, 0.5]
    p.volu_pose = Pose.from_matrix(m)
    return p


def crafted_records():
    rng = np.random.default_rng(20240607)
    n = int(np.prod(CRAFT_DIMS))
    rec = np.zeros(n, np.dtype([("tsdf", "<i2"), ("weight", "<i2"), ("rgb", "u1", 3), ("pad", "u1")]))
    t = rng.integers(-3000, 3001, n)
    u = rng.random(n)
    t[u < 0.05] = 0
    t[(u >= 0.05) & (u < 0.10)] = 32767
    rec["tsdf"] = t
    rec["weight"] = np.where(rng.random(n) < 0.2, 0, rng.integers(1, 65, n))
    rgb = rng.integers(0, 256, (n, 3))
    u = rng.random(n)
    rgb[u < 0.2] = 0
    rgb[(u >= 0.2) & (u < 0.22)] = [0, 0, 1]  # near-black, but coloured
    rgb[(u >= 0.22) & (u < 0.24)] = [1, 0, 0]
    rec["rgb"] = rgb
    return rec


# ---- volume builders ---------------------------------------------------------------
# Each returns (tsdf (N,) int16, weight (N,) int16, rgb (N, 3) uint8), x fastest, read-only;
# records() makes the upload of them, volume() the restatement's view.

CRAFT_SEED = 20240607


def params_for(dims, pose: Pose | None = None):
    """crafted_params() (rotated pose, three different voxel sizes: 20 x 15 x 30 mm) at `dims`."""
    p = crafted_params()
    for i in range(3):
        p.volu_dims[i] = int(dims[i])
        p.volu_range[i] = CRAFT_RANGE[i] / CRAFT_DIMS[i] * int(dims[i])
    if pose is not None:
        p.volu_pose = pose
    return p


def records(t, w, rgb):
    """The reference's 8-byte voxel records (what upload_tsdf takes)."""
    rec = np.zeros(len(t), np.dtype([("tsdf", "<i2"), ("weight", "<i2"), ("rgb", "u1", 3), ("pad", "u1")]))
    rec["tsdf"], rec["weight"], rec["rgb"] = t, w, rgb
    return rec


def volume(p, t, w, rgb, pose: Pose | None = None) -> Vol:
    """The restatement's view of a builder's volume under the parameters p (pose: in place of p's)."""
    c = np.zeros((len(t), 4), np.uint8)
    c[:, :3] = rgb
    dims = tuple(int(d) for d in p.volu_dims)
    return Vol(dims, tuple(float(r) for r in p.volu_range), p.volu_pose if pose is None else pose, t, w, c)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def dense(dims, seed=CRAFT_SEED):
    """crafted_records()'s recipe at any dims: random signs in every brick, 5 % tsdf 0, 5 % tsdf
    32767 (F = 1), 20 % weight 0, 20 % never coloured and two near-black colours."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(dims))
    t = rng.integers(-3000, 3001, n)
    u = rng.random(n)
    t[u < 0.05] = 0
    t[(u >= 0.05) & (u < 0.10)] = 32767
    w = np.where(rng.random(n) < 0.2, 0, rng.integers(1, 65, n))
    rgb = rng.integers(0, 256, (n, 3))
    u = rng.random(n)
    rgb[u < 0.2] = 0
    rgb[(u >= 0.2) & (u < 0.22)] = [0, 0, 1]
    rgb[(u >= 0.22) & (u < 0.24)] = [1, 0, 0]
    return _frozen(t.astype(np.int16), w.astype(np.int16), rgb.astype(np.uint8))


@functools.lru_cache(maxsize=None)
def scene(dims):
    """An analytic distance field in voxel units: a slanted plane and two spheres, each a shell 3
    voxels thick (negative within 1.5 voxels of the surface, so neither has a far interior),
    truncated at 3 voxels and quantised as tests/test_mesh.py does, 0 replaced by 1.  Farther than
    4.5 voxels from every surface the tsdf is +32767: most bricks hold no negative value.  The
    plane rises 0.9 voxels per x and 0.3 per y, so it crosses only a band of the column tiles; the
    spheres sit in opposite corners, the smaller one against the high x face.
    Weights 1..64 with 5 % zero; random colours with 20 % never coloured."""
    X, Y, Z = (int(d) for d in dims)
    gz, gy, gx = (np.arange(n, dtype=np.float64) + 0.5 for n in (Z, Y, X))
    z, y, x = np.meshgrid(gz, gy, gx, indexing="ij")
    plane = ((z - 0.5 * Z) - 0.9 * (x - 0.5 * X) - 0.3 * (y - 0.5 * Y)) / np.sqrt(1 + 0.9 ** 2 + 0.3 ** 2)
    spheres = [((0.16 * X, 0.27 * Y, 0.3 * Z), 0.2 * Z + 0.7), ((X - 4.2, 0.71 * Y, 0.68 * Z), 0.15 * Z + 0.4)]
    d = np.abs(plane)
    for (cx, cy, cz), r in spheres:
        d = np.minimum(d, np.abs(np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) - r))
    d -= 1.5
    q = np.clip((np.clip(d / 3.0, -1, 1) * 32767).astype(np.int32), -32767, 32767)
    q[q == 0] = 1
    rng = np.random.default_rng(77)
    n = X * Y * Z
    w = np.where(rng.random(n) < 0.05, 0, rng.integers(1, 65, n))
    rgb = rng.integers(0, 256, (n, 3))
    rgb[rng.random(n) < 0.2] = 0
    return _frozen(q.ravel().astype(np.int16), w.astype(np.int16), rgb.astype(np.uint8))


def isolated(dims, positions):
    """tsdf +1000, weight 1 and a colour everywhere, tsdf -1000 at each voxel of `positions`."""
    X, Y, Z = (int(d) for d in dims)
    n = X * Y * Z
    t = np.full(n, 1000, np.int16)
    for x, y, z in positions:
        assert 0 <= x < X and 0 <= y < Y and 0 <= z < Z
        t[(z * Y + y) * X + x] = -1000
    rgb = np.random.default_rng(5).integers(1, 256, (n, 3)).astype(np.uint8)
    return _frozen(t, np.ones(n, np.int16), rgb)


# brick-local coordinates of the interior negatives: the brick's eight corners and one inside
ISOLATED_LOCAL = tuple((lx, ly, lz) for lz in (0, 7) for ly in (0, 7) for lx in (0, 7)) + ((3, 4, 5),)
# The isolated volume: 12 x 7 x 8.5 bricks.  Z is no multiple of 8, and two equal slabs meet at
# z = 32, directly above the negatives of brick layer 3 with local z = 7.
ISOLATED_DIMS = (96, 56, 68)
# A shift whose way there and back the interior negatives survive with every neighbour: it drops
# the brick layers x < 8, y >= Y - 8 and z < 16, which return unobserved (weight 0).
ISOLATED_SHIFT = (8, -8, 16)


def isolated_interior(dims=ISOLATED_DIMS):
    """One negative per entry of ISOLATED_LOCAL, in bricks on a lattice of pitch 3: each is the
    only negative of its 5 x 5 x 5 brick neighbourhood, and all of that brick's 26 neighbours are
    whole bricks of the volume that ISOLATED_SHIFT and its opposite leave alone."""
    nb = [int(d) // 8 for d in dims]  # whole bricks
    lattice = [(bx, by, bz) for bz in range(3, nb[2] - 1, 3) for by in range(1, nb[1] - 2, 3)
               for bx in range(2, nb[0] - 1, 3)]
    assert len(lattice) >= len(ISOLATED_LOCAL), dims
    return tuple((8 * bx + lx, 8 * by + ly, 8 * bz + lz) for (bx, by, bz), (lx, ly, lz) in zip(lattice, ISOLATED_LOCAL))


def isolated_border(dims=ISOLATED_DIMS):
    """Negatives on the volume's own corners and faces (z = Z - 1 is the slice FullScan6 never visits)."""
    X, Y, Z = (int(d) for d in dims)
    return ((0, 0, 0), (X - 1, 0, 0), (0, Y - 1, 0), (0, 0, Z - 2), (X - 1, Y - 1, Z - 2), (X - 1, Y - 1, Z - 1))


# ---- what the GPU tests force, and the tiles that make it matter ---------------------

UNITS = (1, 2, 4, 8, 16, 32, 64)  # every K of kfx_debug_extract_units
# 17 x 15 = 255 tiles: the last wave is ragged for every K > 1; 41 swept slices: 6 chunks, the last of one slice
SWEEP_DIMS = (136, 120, 42)
# 32 x 16 tiles x 17 chunks = 8704 units: three blocks of the offset scan, K = 1
SCAN_DIMS = (256, 128, 136)


def tile_classes(dims, t):
    """Per 8-slice chunk c and column tile: set[c, tile] = the tile holds a negative tsdf in the
    chunk's slices (its brick bit is certainly set), clear[tile] = no tile of its 3 x 3
    neighbourhood holds a negative at any z (its bit is certainly clear in every chunk; the
    occupancy marks are a superset of the negatives, so nothing else is certain)."""
    X, Y, Z = (int(d) for d in dims)
    neg = np.asarray(t).reshape(Z, Y // 8, 8, X // 8, 8) < 0
    per_slice = neg.any(axis=(2, 4))  # (Z, ty, tx)
    nc = (Z + 7) // 8
    chunk_set = np.stack([per_slice[8 * c:8 * c + 8].any(0) for c in range(nc)])
    col = per_slice.any(0)
    pad = np.pad(col, 1)
    near = np.zeros_like(col)
    for dy in range(3):
        for dx in range(3):
            near |= pad[dy:dy + col.shape[0], dx:dx + col.shape[1]]
    return chunk_set.reshape(nc, -1), ~near.ravel()


def mixed_groups(dims, t, K):
    """(chunk, first tile) of the groups of K consecutive tiles (one wave's units) that hold both
    a certainly clear and a certainly set tile."""
    chunk_set, clear = tile_classes(dims, t)
    out = []
    for c in range(len(chunk_set)):
        for t0 in range(0, chunk_set.shape[1], K):
            if chunk_set[c, t0:t0 + K].any() and clear[t0:t0 + K].any():
                out.append((c, t0))
    return out


@functools.lru_cache(maxsize=None)
def reference(name, dims):
    """(params, records, Vol, points, triangles) of the builder `name` ("dense" / "scene") at dims."""
    t, w, rgb = {"dense": dense, "scene": scene}[name](tuple(dims))
    p = params_for(dims)
    v = volume(p, t, w, rgb)
    pts, tri = restate(v)
    return p, records(t, w, rgb), v, pts, tri
