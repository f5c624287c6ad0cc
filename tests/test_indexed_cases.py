"""The indexed mesh's reference on the CPU (indexed_cases.py): on every fixture test_gpu_indexed.py
uses, the reference's verts[tris] is the oracle-checked soup of extract_cases, the used-edge
predicate of include/kfx.h gives the same vertex set, and the fixtures hold what the GPU tests use
them for.  Then the PLY writer, which needs the library but no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import extract_cases as EC
import indexed_cases as IC
import stream_cases as ST
import world_cases as WC

VDT = EC.VDT


def check_reference(v: EC.Vol, ref: IC.Indexed, soup, what):
    assert ref.tris.dtype == np.uint32 and ref.verts.dtype == VDT
    assert EC.same(ref.verts[ref.tris], soup), f"{what}: {EC.first_difference(ref.verts[ref.tris], soup)}"
    used = IC.used_edges(v)
    assert np.array_equal(used, np.unique(ref.corner_edges, axis=0)), what  # the predicate names the same edges
    assert len(used) == len(ref.verts) and len(np.unique(ref.edges, axis=0)) == len(ref.edges)  # no edge twice
    assert 0 < len(ref.verts) < 3 * len(ref.tris), what
    assert int(ref.tris.max()) == len(ref.verts) - 1 and len(np.unique(ref.tris)) == len(ref.verts)  # every vertex used


def not_point_edges(v, ref):
    pe = {tuple(r) for r in EC.point_edges(v)}
    return sum(tuple(r) not in pe for r in ref.edges)


@pytest.mark.parametrize("name,dims", IC.WINDOW_FIXTURES, ids=lambda a: a if isinstance(a, str) else "x".join(map(str, a)))
def test_window_fixtures(oracle_lib, name, dims):
    p, rec, v, ref = IC.window_case(name, tuple(dims))
    soup = EC.reference(name, tuple(dims))[4] if name in ("dense", "scene") else EC.restate(v)[1]
    check_reference(v, ref, soup, f"{name} {dims}")
    cls = IC.corner_classes(v)
    extra = not_point_edges(v, ref)
    print(f"{name} {dims}: T {len(ref.tris)}, 3T {3 * len(ref.tris)}, V {len(ref.verts)}, corners by owner brick {cls}, "
          f"{extra} vertices on no point edge, {IC.equal_pairs(ref.verts)} vertices with another's bytes")
    if name == "dense" and tuple(dims) in (EC.CRAFT_DIMS, EC.SWEEP_DIMS):
        assert all(cls[c] > 0 for c in IC.CLASSES), cls  # every way a corner's owner lies in another brick
        assert extra > 0                                  # the vertex pass cannot be built on the point test
    if tuple(dims) == EC.CRAFT_DIMS:
        assert (len(ref.tris), len(ref.verts)) == (5878, 6935)
        assert IC.equal_pairs(ref.verts) > 0  # a tsdf == 0 end: distinct edges, the same 28 bytes, never welded
    if dims[0:2] == (24, 16):  # the depth volumes: a short last chunk, and the top slice's +x / +y edges in use
        top = ref.edges[:, 2] == dims[2] - 1
        assert top.any() and set(ref.edges[top, 3]) == {0, 1}
    if name in ("interior", "border"):
        # an isolated negative with every neighbour: 6 vertices and 8 triangles; the owners of the -x / -y / -z
        # ones lie in voxels (and for local 0 in bricks) that hold nothing negative
        t = np.asarray(EC.isolated(tuple(dims), {"interior": EC.isolated_interior, "border": EC.isolated_border}[name](tuple(dims)))[0])
        negs = np.argwhere(t.reshape(dims[2], dims[1], dims[0]) < 0)
        if name == "interior":
            assert (len(ref.verts), len(ref.tris)) == (6 * len(negs), 8 * len(negs))
            brick_neg = {tuple(int(c) // 8 for c in zyx[::-1]) for zyx in negs}
            owners = {tuple(int(c) // 8 for c in e[:3]) for e in ref.edges}
            assert len(owners - brick_neg) >= 12, "too few owners in bricks that hold nothing negative"
        else:  # on the volume's faces and corners: the cubes and owners that do not exist
            assert len(ref.verts) > 0 and (ref.edges[:, :3].min(0) == 0).all()


def test_scene_24(oracle_lib):
    p, rec, v, ref = IC.window_case("scene", (40, 32, 24))
    assert (len(ref.tris), len(ref.verts)) == (6389, 4508)


def test_world_fixtures(oracle_lib):
    p = WC.window_params()
    keep, t, w, rgb = WC.sparse_world()
    got = []
    for base in WC.SPARSE_BASES:
        soup = WC.reference(p, WC.SPARSE_BOX, t, w, rgb, base)[1]
        ref = IC.world_reference(p, WC.SPARSE_BOX, t, w, rgb, base)
        check_reference(WC.vol_at(p, WC.SPARSE_BOX, t, w, rgb), ref, soup, f"sparse world at {base}")
        got.append(ref)
    assert np.array_equal(got[0].tris, got[1].tris) and not np.array_equal(got[0].verts["xyz"], got[1].verts["xyz"])
    assert got[0].verts["normal"].tobytes() == got[1].verts["normal"].tobytes()
    cls = IC.corner_classes(WC.vol_at(p, WC.SPARSE_BOX, t, w, rgb))
    assert all(cls[c] > 0 for c in IC.CLASSES), cls
    # no vertex is owned by an absent brick: the dense canonical order is the list order
    owner = (got[0].edges[:, :3] // 8)
    nb = ST.brick_counts(WC.SPARSE_BOX)
    assert keep[(owner[:, 2] * nb[1] + owner[:, 1]) * nb[0] + owner[:, 0]].all()
    seen = set()
    for removed in [None] + [r for r in range(27) if r != 13]:
        keep, t, w, rgb = WC.neigh_world(removed)
        soup = WC.reference(p, WC.NEIGH_BOX, t, w, rgb, (3, -1, 2))[1]
        ref = IC.world_reference(p, WC.NEIGH_BOX, t, w, rgb, (3, -1, 2))
        check_reference(WC.vol_at(p, WC.NEIGH_BOX, t, w, rgb), ref, soup, f"without brick {removed}")
        seen.add((len(ref.verts), ref.tris.tobytes()))
    assert len(seen) > 1  # a removed neighbour changes the mesh


def test_window_identity_fixture(oracle_lib):
    """The 64^3 scene holds no crossing in its top slice's +x / +y edges: there the world of the
    window's bricks and the window give the same indexed mesh."""
    dims = (64, 64, 64)
    p, rec, v, ref = IC.window_case("scene", dims)
    check_reference(v, ref, EC.reference("scene", dims)[4], "scene 64")
    t, w, rgb = EC.scene(dims)
    wr = IC.world_reference(p, dims, t, w, rgb)
    assert EC.same(wr.verts, ref.verts) and np.array_equal(wr.tris, ref.tris)


# ---- the PLY writer ---------------------------------------------------------------------

def quad():
    v = np.zeros(4, VDT)
    v["xyz"] = [[0, 0, 0], [1, 0, 0.5], [1, 1, 1e-7], [0, 1, -2.25]]
    v["normal"] = [[0, 0, 1], [0, 0, 1], [0.6, 0, 0.8], [0, 0, 1]]
    v["bgra"] = [[1, 2, 3, 255], [0, 0, 0, 0], [255, 128, 7, 255], [9, 8, 7, 255]]
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.uint32)


def test_ply_writer_text(kfx_lib, tmp_path):
    v, t = quad()
    path = str(tmp_path / "quad.ply")
    kfx_lib.write_ply_mesh_indexed(path, v, t)
    want = ("ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
            "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\n"
            "property uchar blue\nelement face 2\nproperty list uchar int vertex_indices\nend_header\n"
            "0 0 0 0 0 1 3 2 1\n1 0 0.5 0 0 1 0 0 0\n1 1 1e-07 0.6 0 0.8 7 128 255\n0 1 -2.25 0 0 1 7 8 9\n"
            "3 0 1 2\n3 0 2 3\n")
    assert open(path).read() == want == IC.ply_text(v, t)
    kfx_lib.write_ply_mesh_indexed(path, v[:0], t[:0])  # an empty mesh is a file with no elements
    assert open(path).read() == IC.ply_text(v[:0], t[:0])


def test_ply_writer_errors_leave_no_file(kfx_lib, tmp_path):
    v, t = quad()
    L = kfx_lib.lib()
    vp, tp = v.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p)
    bad = t.copy()
    bad[1, 2] = 4  # an index >= n_verts
    cases = {"index": (vp, 4, bad.ctypes.data_as(C.c_void_p), 2), "null verts": (None, 4, tp, 2), "null tris": (vp, 4, None, 2),
             "negative verts": (vp, -1, tp, 2), "negative tris": (vp, 4, tp, -1)}
    for what, (a, na, b, nb) in cases.items():
        path = tmp_path / (what.replace(" ", "_") + ".ply")
        assert L.kfx_write_ply_mesh_indexed(str(path).encode(), a, na, b, nb) == -1, what
        assert L.kfx_last_error() and not os.path.exists(path), what
    assert L.kfx_write_ply_mesh_indexed(None, vp, 4, tp, 2) == -1
    assert L.kfx_write_ply_mesh_indexed(str(tmp_path / "ok.ply").encode(), vp, 4, tp, 2) == 0
