"""Attributed extraction (kfx_extract_points_attr / kfx_extract_mesh_attr and
the savers on top) against a numpy restatement of the definitions in
include/kfx.h (tests/extract_cases.py).  The oracle has no colours or normals, so the restatement is
first checked against it where it can be: its positions must equal
O.extract_points / O.extract_mesh bit for bit (which fixes the canonical order,
the triangle table and the edge numbering); the normals and colours are then
compared bit for bit with the library's, from the same downloaded volume."""
import numpy as np
import pytest

import oracle as O
from extract_cases import (CRAFT_DIMS, CRAFT_RANGE, VDT, Vol, crafted_params, crafted_records, first_difference,
                           mesh_edges, point_edges, restate, same)
from kfx import KinectFusion, pipeline_group, synth
from kfx.abi import Intrinsics, default_params

pytestmark = pytest.mark.gpu

L_VOL = 2.048
CAP = 200_000  # above every total here (buffers and the library's pool are sized by the cap)


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
