"""Attributed extraction (kfx_extract_points_attr / kfx_extract_mesh_attr and
the savers on top) against a numpy restatement of the definitions in
include/kfx.h.  The oracle has no colours or normals, so the restatement is
first checked against it where it can be: its positions must equal
O.extract_points / O.extract_mesh bit for bit (which fixes the canonical order,
the triangle table and the edge numbering); the normals and colours are then
compared bit for bit with the library's, from the same downloaded volume."""
import numpy as np
import pytest

import oracle as O
from kfx import VERTEX_DTYPE, KinectFusion, pipeline_group, synth
from kfx.abi import Intrinsics, Pose, default_params

pytestmark = pytest.mark.gpu

f32 = np.float32
L_VOL = 2.048
DIV = f32(0.0000305185)  # kDivShortMax
CAP = 200_000  # above every total here (buffers and the library's pool are sized by the cap)
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


# ---- volumes -------------------------------------------------------------------

@pytest.fixture(scope="module")
def fused():
    intr = synth.Intrinsics.qvga()
    bgr, dep, _ = synth.sequence(5, intr, noise=True, dropout=0.01)
    p = default_params(dims=128, range_m=L_VOL)
    kf = KinectFusion(Intrinsics.from_any(intr), p)
    for k in range(len(dep)):
        kf.pipeline(bgr[k], dep[k].astype(np.float32))
    v = Vol(kf.dims, (L_VOL,) * 3, p.volu_pose, *kf.volume_soa())
    pts, tri = restate(v)
    yield kf, p, (bgr, dep, intr), v, pts, tri
    kf.close()


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


@pytest.fixture(scope="module")
def crafted():
    intr = synth.Intrinsics.qvga()
    p = crafted_params()
    kf = KinectFusion(Intrinsics.from_any(intr), p)
    rec = crafted_records()
    kf.upload_tsdf(rec)
    t, w, c = kf.volume_soa()
    assert np.array_equal(t, rec["tsdf"]) and np.array_equal(w, rec["weight"])
    assert np.array_equal(c.reshape(-1, 4)[:, :3], rec["rgb"])
    v = Vol(CRAFT_DIMS, CRAFT_RANGE, p.volu_pose, t, w, c)
    pts, tri = restate(v)
    yield kf, p, intr, rec, v, pts, tri
    kf.close()


# ---- 1, 2: the fused volume ------------------------------------------------------

def test_fused_points(fused):
    kf, _, _, _, pts, _ = fused
    g = kf.extract_points_attr(CAP)
    assert g.dtype == VDT and g.shape == (len(pts),)
    assert np.array_equal(g["xyz"].view(np.uint32), kf.extract_points(CAP).view(np.uint32))
    assert same(g, pts), first_difference(g, pts)


def test_fused_mesh(fused):
    kf, _, _, _, _, tri = fused
    g = kf.extract_mesh_attr(CAP)
    assert g.dtype == VDT and g.shape == (len(tri), 3)
    assert np.array_equal(g["xyz"].view(np.uint32), kf.extract_mesh(CAP).view(np.uint32))
    assert same(g, tri), first_difference(g, tri)


def test_fused_volume_is_not_vacuous(fused):
    """The fixture exercises what test 1 compares: most points coloured, many
    colours, one-sided gradients, and normals that face the camera (which
    looks at the surface from the origin side in every frame)."""
    _, _, _, v, pts, tri = fused
    e = point_edges(v)
    assert len(pts) > 10000 and len(tri) > 10000
    assert (pts["bgra"][:, 3] == 255).mean() >= 0.95
    x, y, z, axis = e.T
    xb, yb, zb = x + (axis == 0), y + (axis == 1), z + (axis == 2)
    cols = np.concatenate([v.c[z, y, x], v.c[zb, yb, xb]])
    assert len(np.unique(cols[cols != 0])) >= 100
    sx, sy, sz = (np.concatenate(a) for a in ((x, xb), (y, yb), (z, zb)))
    surf = np.unique(np.stack([sx, sy, sz], 1), axis=0)
    one_sided = np.zeros(len(surf), bool)
    for k in range(3):
        valid = []
        for s in (1, -1):
            n = [surf[:, 0].copy(), surf[:, 1].copy(), surf[:, 2].copy()]
            n[k] += s
            inside = (n[k] >= 0) & (n[k] < v.dims[k])
            n[k] = np.clip(n[k], 0, v.dims[k] - 1)
            valid.append(inside & (v.w[n[2], n[1], n[0]] != 0))
        one_sided |= valid[0] ^ valid[1]
    share = one_sided.mean()
    facing = ((pts["normal"] * -pts["xyz"]).sum(1) > 0).mean()
    zero = (pts["normal"] == 0).all(1).mean()
    print("coloured %.4f one-sided %.4f facing %.4f zero normals %.4f" %
          ((pts["bgra"][:, 3] == 255).mean(), share, facing, zero))
    assert share >= 0.05
    assert facing >= 0.95


# ---- 3: the crafted volume -------------------------------------------------------

def test_crafted_points(crafted):
    kf, _, _, _, v, pts, _ = crafted
    assert len(pts) > 1000
    g = kf.extract_points_attr(CAP)
    assert np.array_equal(g["xyz"].view(np.uint32), kf.extract_points(CAP).view(np.uint32))
    assert same(g, pts), first_difference(g, pts)
    # the branches the volume is there for
    e = point_edges(v)
    x, y, z, axis = e.T
    xb, yb, zb = x + (axis == 0), y + (axis == 1), z + (axis == 2)
    ncol = (v.c[z, y, x] != 0).astype(int) + (v.c[zb, yb, xb] != 0)
    assert all((ncol == k).sum() > 20 for k in (0, 1, 2))
    assert set(np.unique(pts["bgra"][:, 3])) == {0, 255}
    for k, c in enumerate((x, y, z)):  # gradients at all six faces
        assert (c == 0).any() and (np.stack([xb, yb, zb])[k] == v.dims[k] - 1).any()
    assert len(set(v.vs.tolist())) == 3


def test_crafted_mesh(crafted):
    kf, _, _, _, v, _, tri = crafted
    assert len(tri) > 1000
    g = kf.extract_mesh_attr(CAP)
    assert np.array_equal(g["xyz"].view(np.uint32), kf.extract_mesh(CAP).view(np.uint32))
    assert same(g, tri), first_difference(g, tri)
    e = mesh_edges(v, O.mc_table())
    x, y, z, axis = e.T
    zero_end = (v.q[z, y, x] == 0) | (v.q[z + (axis == 2), y + (axis == 1), x + (axis == 0)] == 0)
    assert zero_end.sum() > 20  # F = 0 endpoints (a cube corner with tsdf 0 is outside)


# ---- 4: cap and paths --------------------------------------------------------------

@pytest.mark.parametrize("mesh", [False, True])
def test_cap_and_passes(mesh, fused):
    kf, _, _, _, pts, tri = fused
    want = tri if mesh else pts
    fn = kf.extract_mesh_attr if mesh else kf.extract_points_attr
    one = fn(CAP)
    assert kf.extract_ms()["passes"] == 1
    capped = fn(cap=1234)
    assert kf.extract_ms()["passes"] == 2  # the pool overflows: count + emit
    assert len(capped) == 1234 and same(capped, want[:1234]), first_difference(capped, want[:1234])
    kf.set_extract_passes(2)
    try:
        two = fn(CAP)
        ms = kf.extract_ms()
        assert ms["passes"] == 2 and ms["emit"] > 0
        two_capped = fn(cap=1234)
    finally:
        kf.set_extract_passes(1)
    assert same(one, want) and same(two, one), first_difference(two, one)
    assert same(two_capped, capped)
    assert kf.extract_count(mesh, attr=True) == kf.extract_count(mesh) == len(want)


# ---- 5: slabs ------------------------------------------------------------------------

def test_fused_slabs_concatenate(fused):
    kf, p, (bgr, dep, intr), _, pts, tri = fused
    for world, mesh, want in ((3, False, pts), (2, True, tri)):
        members = [KinectFusion(Intrinsics.from_any(intr), p, slab=(r, world)) for r in range(world)]
        try:
            for k in range(len(dep)):
                pipeline_group(members, bgr[k], dep[k].astype(np.float32))
            parts = [m.extract_mesh_attr(CAP) if mesh else m.extract_points_attr(CAP) for m in members]
        finally:
            for m in members:
                m.close()
        assert all(len(x) > 0 for x in parts)
        got = np.concatenate(parts)
        assert same(got, want), first_difference(got, want)


def test_crafted_slabs_concatenate(crafted):
    _, p, intr, rec, _, pts, tri = crafted
    # 8-slice slabs need explicit cuts (the equal partition asks for 16 slices per slab)
    members = [KinectFusion(Intrinsics.from_any(intr), p, slab=(r, 2), cuts=[0, 8, 16]) for r in range(2)]
    try:
        assert [m.slab_info() for m in members] == [(0, 12, 0, 8), (4, 12, 8, 16)]
        for m in members:
            m.upload_tsdf(rec)
        gp = [m.extract_points_attr(CAP) for m in members]
        gm = [m.extract_mesh_attr(CAP) for m in members]
    finally:
        for m in members:
            m.close()
    assert all(len(x) > 0 for x in gp + gm)
    assert same(np.concatenate(gp), pts), first_difference(np.concatenate(gp), pts)
    assert same(np.concatenate(gm), tri), first_difference(np.concatenate(gm), tri)


# ---- 6: save and index64 ---------------------------------------------------------------

PLY_PROPS = ("property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\n"
             "property float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n")


def _vertex_lines(v):
    v = v.ravel()
    xyz, nrm, c = v["xyz"].astype(np.float64), v["normal"].astype(np.float64), v["bgra"].astype(int)
    return "".join("%g %g %g %g %g %g %d %d %d\n" % (*xyz[i], *nrm[i], c[i, 2], c[i, 1], c[i, 0])
                   for i in range(len(v)))


def test_save_files(crafted, tmp_path):
    kf, _, _, _, _, pts, tri = crafted
    path = tmp_path / "cloud.ply"
    kf.save_pointcloud_attr(str(path))
    assert path.read_text() == ("ply\nformat ascii 1.0\nelement vertex %d\n" % len(pts) + PLY_PROPS + "end_header\n"
                                + _vertex_lines(pts))
    kf.save_pointcloud_attr(str(path), 100)
    assert path.read_text().splitlines()[2] == "element vertex 100"
    path = tmp_path / "mesh.ply"
    kf.save_mesh_attr(str(path))
    assert path.read_text() == ("ply\nformat ascii 1.0\nelement vertex %d\n" % (3 * len(tri)) + PLY_PROPS
                                + "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(tri)
                                + _vertex_lines(tri)
                                + "".join("3 %d %d %d\n" % (3 * i, 3 * i + 1, 3 * i + 2) for i in range(len(tri))))


def test_index64_outputs_equal(crafted):
    kf, _, _, _, _, pts, tri = crafted
    kf.debug_force_index64(True)
    try:
        gp, gm = kf.extract_points_attr(CAP), kf.extract_mesh_attr(CAP)
    finally:
        kf.debug_force_index64(False)
    assert same(gp, pts) and same(gm, tri)


# ---- the runner's two new arguments ------------------------------------------------------

def test_runner_writes_coloured_cloud_and_mesh(tmp_path):
    """kfx_run <dataset> poses cloud colored_cloud colored_mesh: the two new
    files are the bytes the binding's savers write after the same frames; the
    first three arguments behave as before."""
    import os
    import subprocess

    from PIL import Image

    import kfx
    intr = synth.Intrinsics.qvga()
    bgr, dep, _ = synth.sequence(4, intr, noise=True, dropout=0.01)
    root = str(tmp_path / "ds")
    os.makedirs(os.path.join(root, "color"))
    os.makedirs(os.path.join(root, "depth"))
    for k in range(len(dep)):
        Image.fromarray(np.ascontiguousarray(bgr[k][:, :, ::-1])).save(os.path.join(root, "color", f"{k:06d}.png"))
        Image.fromarray(dep[k]).save(os.path.join(root, "depth", f"{k:06d}.png"))
    with open(os.path.join(root, "intr.txt"), "w") as f:
        f.write(f"{intr.fx} 0 {intr.cx}\n0 {intr.fy} {intr.cy}\n0 0 1\n")
    kf = KinectFusion(Intrinsics.from_any(intr), default_params())  # the runner's parameters
    for k in range(len(dep)):
        kf.pipeline(bgr[k], dep[k].astype(np.float32))
    want = {}
    for name, save in (("cloud", kf.save_pointcloud), ("ccloud", kf.save_pointcloud_attr), ("cmesh", kf.save_mesh_attr)):
        save(str(tmp_path / ("want_" + name)))
        want[name] = open(tmp_path / ("want_" + name), "rb").read()
    kf.close()
    runner = os.path.join(os.path.dirname(kfx.LIB_PATH), "kfx_run")
    r = subprocess.run([runner, root, str(tmp_path / "poses.txt")] + [str(tmp_path / n) for n in want],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "end!" in r.stdout, r.stdout + r.stderr
    assert want["ccloud"].startswith(b"ply\nformat ascii 1.0\nelement vertex ") and b"property uchar red" in want["ccloud"][:400]
    assert b"element face " in want["cmesh"][:400] and len(want["ccloud"]) > 100000
    for name in want:
        assert open(tmp_path / name, "rb").read() == want[name], name
