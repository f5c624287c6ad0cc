"""CPU checks behind the free-viewpoint render tests (view_cases.py): the numpy
restatement of the hit vertex reproduces the oracle's vmap bit for bit, the
trilinear corners the colour blend reads lie in the volume, the scene exercises
both the blend and its Phong fallback, and kfx_write_ppm writes what it says."""
import numpy as np
import pytest

import view_cases as VC


@pytest.mark.parametrize("dims", VC.DIMS)
def test_restated_vertex_reproduces_oracle_vmap(dims, oracle_lib):
    p = VC.params(dims)
    last = VC.fused(dims)[3][-1]
    hits, both = {}, 0
    for name, intr, pose in VC.views(last):
        ref = VC.reference(dims, intr, pose)
        hit = ref["hit"]
        hits[name] = int(hit.sum())
        P, org = VC.restate_vertex(p, intr, pose, ref["ts"])
        v = VC.restate_vmap(p, pose, P, org)
        assert np.array_equal(v[hit].view(np.uint32), ref["vmap"][hit].view(np.uint32)), name
        g, q, d = VC.corners(p, P)
        assert (g[hit] >= 0).all() and (g[hit] + 1 < d).all(), name
        assert (q[hit] >= 0).all() and (q[hit] <= 255).all(), name
        assert not ref["vmap"][~hit].any() and not ref["nmap"][~hit].any()
        n_col, n_bare = int(ref["coloured"].sum()), int((hit & ~ref["coloured"]).sum())
        both += n_col >= 1000 and n_bare >= 100
    # the GPU comparisons are not vacuous: surfaces in the first three views,
    # and one view at least with both blended pixels and Phong fallbacks
    assert all(hits[n] >= 1000 for n in ("off", "odd", "qvga")), hits
    assert hits["miss"] == 0, hits
    assert both >= 1, hits


def test_write_ppm_bytes(tmp_path, kfx_lib):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (7, 13, 3), dtype=np.uint8)
    path = tmp_path / "v.ppm"
    kfx_lib.write_ppm(str(path), img)
    want = b"P6\n13 7\n255\n" + np.ascontiguousarray(img[:, :, ::-1]).tobytes()
    assert open(path, "rb").read() == want
    assert kfx_lib.lib().kfx_write_ppm(str(path).encode(), None, 13, 7) == -1
    assert kfx_lib.lib().kfx_write_ppm(str(tmp_path / "no" / "dir.ppm").encode(),
                                       img.ctypes.data_as(kfx_lib.C.POINTER(kfx_lib.C.c_uint8)), 13, 7) == -1
