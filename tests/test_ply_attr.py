"""kfx_write_ply_attr / kfx_write_ply_mesh_attr (host only): the exact ASCII PLY
text of attributed vertices — header with x y z nx ny nz and uchar red green
blue, lines "%g %g %g %g %g %g %d %d %d" with red = the record's r, and for the
mesh the face element and faces "3 3i 3i+1 3i+2" of kfx_write_ply_mesh."""
import numpy as np

HEAD = ("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
        "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\n"
        "property uchar blue\n")


def _records(kfx):
    v = np.zeros(6, np.dtype(kfx.VERTEX_DTYPE))
    v["xyz"] = [[0, 0, 0], [1, -2.5, 3.25], [1e-7, 123456.789, -0.333333343], [1e10, -1e-10, 7],
                [0.1, 0.2, 0.3], [-1, -1, -1]]
    v["normal"] = [[0, 0, 1], [0.6, -0.8, 0], [0.577350259, 0.577350259, -0.577350259], [0, 0, 0],
                   [-1, 0, 0], [1e-8, 1, 0]]
    v["bgra"] = [[1, 2, 3, 255], [255, 0, 0, 255], [0, 255, 0, 255], [0, 0, 0, 0], [10, 20, 30, 255],
                 [0, 0, 1, 255]]
    return v


def _lines(v):
    return "".join("%g %g %g %g %g %g %d %d %d\n" % (*(float(a) for a in r["xyz"]), *(float(a) for a in r["normal"]),
                                                    int(r["bgra"][2]), int(r["bgra"][1]), int(r["bgra"][0]))
                   for r in v)


def test_vertex_record_layout(kfx_lib):
    dt = np.dtype(kfx_lib.VERTEX_DTYPE)
    assert dt.itemsize == 28
    assert [dt.fields[k][1] for k in ("xyz", "normal", "bgra")] == [0, 12, 24]


def test_write_ply_attr_text(kfx_lib, tmp_path):
    v = _records(kfx_lib)
    path = tmp_path / "cloud.ply"
    kfx_lib.write_ply_attr(str(path), v)
    text = path.read_text()
    assert text == HEAD % 6 + "end_header\n" + _lines(v)
    assert text.splitlines()[13] == "0 0 0 0 0 1 3 2 1"  # red = r = bgra[2]
    kfx_lib.write_ply_attr(str(path), v[:0])
    assert path.read_text() == HEAD % 0 + "end_header\n"


def test_write_ply_mesh_attr_text(kfx_lib, tmp_path):
    v = _records(kfx_lib).reshape(2, 3)
    path = tmp_path / "mesh.ply"
    kfx_lib.write_ply_mesh_attr(str(path), v)
    want = (HEAD % 6 + "element face 2\nproperty list uchar int vertex_indices\nend_header\n" + _lines(v.ravel())
            + "3 0 1 2\n3 3 4 5\n")
    assert path.read_text() == want
