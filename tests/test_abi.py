"""C-ABI boundary checks that need no GPU: the library builds for gfx950,
loads, exports every entry point include/kfx.h declares, and its host-side
defaults match the reference's default_params (kinectfusion.cpp:167-190)."""
import ctypes as C
import os
import re

import numpy as np

import kfx
from kfx.abi import Params, default_params

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kfx.h")


def declared_symbols():
    src = open(HDR).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(kfx_[a-z0-9_]+)\s*\(", src)))


def test_header_and_binding_agree():
    assert declared_symbols() == sorted(kfx.EXPORTS)


def test_library_exports_every_declared_symbol(kfx_lib):
    L = C.CDLL(kfx_lib.LIB_PATH)
    missing = [s for s in declared_symbols() if not hasattr(L, s)]
    assert not missing, missing
    assert kfx_lib.lib().kfx_abi_version() == 2


def test_library_is_gfx950_code_object(kfx_lib):
    data = open(kfx_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in data
    assert b"k_integrate" in data and b"k_raycast" in data and b"k_icp_acc" in data


def test_default_params_match_reference(kfx_lib):
    p = Params()
    assert kfx_lib.lib().kfx_default_params(C.byref(p)) == 0
    q = default_params(dims=512, range_m=3.0)
    assert bytes(p) == bytes(q)
    assert p.pyramid_height == 3 and list(p.icp_iter_count)[:3] == [4, 5, 10]
    assert np.float32(p.volu_trun_dist) == np.float32(2.1) * np.float32(3.0) / np.float32(512)


def test_create_rejects_bad_arguments(kfx_lib):
    from kfx.abi import Intrinsics
    h = C.c_void_p()
    p = default_params(dims=64)
    bad = Intrinsics(321, 240, 1.0, 1.0, 0.0, 0.0)
    assert kfx_lib.lib().kfx_create(C.byref(bad), C.byref(p), 0, C.byref(h)) == -1
    p2 = default_params(dims=60)
    good = Intrinsics(320, 240, 262.5, 262.5, 159.5, 119.5)
    assert kfx_lib.lib().kfx_create(C.byref(good), C.byref(p2), 0, C.byref(h)) == -1
    assert b"multiples of 8" in kfx_lib.lib().kfx_last_error()


def test_create_argument_table(kfx_lib):
    """The edges of what create_impl accepts (its checks come before the device
    query, so no GPU is needed): each rejected configuration returns
    KFX_ERR_ARG, each accepted boundary gets past the checks (KFX_OK with a
    device, KFX_ERR_NO_DEVICE without one)."""
    from kfx.abi import Intrinsics
    KFX_ERR_ARG, KFX_ERR_NO_DEVICE = -1, -5
    L = kfx_lib.lib()

    def create(w, h, **kw):
        p = default_params(dims=64, range_m=2.048)
        geo = {k: kw.pop(k) for k in ("fx", "fy", "cx", "cy") if k in kw}
        for k, v in kw.items():
            if k == "icp_iter_count":
                for i, n in enumerate(v):
                    p.icp_iter_count[i] = n
            else:
                setattr(p, k, v)
        intr = Intrinsics(w, h, geo.get("fx", 0.8 * w), geo.get("fy", geo.get("fx", 0.8 * w)),
                          geo.get("cx", (w - 1) / 2.0), geo.get("cy", (h - 1) / 2.0))
        h_ = C.c_void_p()
        rc = L.kfx_create(C.byref(intr), C.byref(p), 0, C.byref(h_))
        if rc == 0:
            L.kfx_destroy(h_)
        return rc

    rejected = [
        (328, 248, dict(pyramid_height=4)),                         # 328 = 8 * 41: no multiple of 16
        (324, 240, dict(pyramid_height=3)),                         # 324 = 4 * 81: no multiple of 8
        (320, 240, dict(bfilter_kernel_size=0)),
        (320, 240, dict(bfilter_kernel_size=16)),
        (16, 12, dict(pyramid_height=2, bfilter_kernel_size=15)),   # level 1 is 8x6: 6 rows <= r = 7
        (320, 240, dict(dfilter_dist=0.0)),
        (320, 240, dict(dfilter_dist=30.5)),
        (320, 240, dict(dfilter_dist=float("nan"))),
        (320, 240, dict(icp_iter_count=[4, -1, 10, 0])),
        (320, 240, dict(pyramid_height=0)),
        (320, 240, dict(pyramid_height=5)),
        # the ICP sums' exactness (icp_exact_pixels): the farthest vertex, 1 m of margin included, must stay
        # below 45.25 m (a 1024-pixel block), and pixels x that bound squared below 2^31 (the int64 totals)
        (320, 240, dict(dfilter_dist=30.0, fx=178.0)),              # corner at 45.04 m, 46.04 with margin
        (2048, 2048, dict(dfilter_dist=17.0)),                      # 2^22 px x 23.7^2 m^2 >= 2^31
        (320, 240, dict(icp_dist_threshold=1.5)),                   # the residual row entry would exceed the bound
        (320, 240, dict(fx=0.0)),
        (320, 240, dict(fx=-256.0)),
        (320, 240, dict(fy=float("nan"))),
        (320, 240, dict(cx=float("inf"))),
        (320, 240, dict(cy=float("nan"))),
    ]
    for w, h, kw in rejected:
        assert create(w, h, **kw) == KFX_ERR_ARG, (w, h, kw)
        assert L.kfx_last_error()
    accepted = [
        (24, 16, dict(pyramid_height=1, bfilter_kernel_size=15)),
        (16, 16, dict(pyramid_height=2, bfilter_kernel_size=15)),   # level 1 is 8x8 > r = 7
        (32, 32, dict(pyramid_height=3, bfilter_kernel_size=7)),
        (64, 48, dict(pyramid_height=4, bfilter_kernel_size=11)),   # level 3 is 8x6 > r = 5
        (40, 24, dict(pyramid_height=3, bfilter_kernel_size=5)),
        (320, 240, dict(dfilter_dist=30.0)),
        (320, 240, dict(bfilter_kernel_size=1)),
        (320, 240, dict(icp_iter_count=[0, 0, 0, 0])),
        (320, 240, dict(dfilter_dist=30.0, fx=190.0)),              # corner at 43.48 m, 44.48 with margin
        (2048, 2048, dict(dfilter_dist=15.0)),                      # 2^22 px x 21.0^2 m^2 < 2^31
        (320, 240, dict(icp_dist_threshold=1.0)),
        (320, 240, dict(icp_dist_threshold=-1.0)),                  # admits nothing: legal
        (320, 240, dict(cx=-40.0, cy=300.0)),                       # a principal point outside the image is legal
    ]
    for w, h, kw in accepted:
        assert create(w, h, **kw) in (0, KFX_ERR_NO_DEVICE), (w, h, kw, L.kfx_last_error())


def test_product_build_refuses_experiment_macros():
    """make ARCH=gfx950 with -DKFX_* macros is refused for the product library
    (experiments build into lib/var_<name>), and the shipped library source
    holds none of the dropped experiment switches."""
    import subprocess
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slam-kinectfusion_amd")
    r = subprocess.run(["make", "-n", "-C", pkg, "ARCH=gfx950", "EXTRA=-DKFX_INT_CERT=1"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "var_" in (r.stdout + r.stderr)
    import glob
    files = sorted(glob.glob(os.path.join(pkg, "csrc", "*.hip")) + glob.glob(os.path.join(pkg, "csrc", "*.h")))
    assert len(files) >= 3
    src = "".join(open(f).read() for f in files)
    for m in ("KFX_INT_ZCLASS", "KFX_INT_CERT", "KFX_INT_DEDUP", "KFX_INT_LEAN", "KFX_INT_PLAN", "KFX_INT_PRIO",
              "KFX_RAY_PRIO", "KFX_ICP_XCOARSE", "KFX_INT_EXP", "KFX_PLAN_EXP", "KFX_RAY_NOREPLAY",
              "KFX_RAY_NONORMAL", "KFX_RAY_PIPE", "KFX_RAY_FFREPLAY", "KFX_RAY_FF_MIN", "KFX_RAY_FAKE_REPLAY",
              "KFX_RAY_LDS", "wrong values"):
        assert m not in src, m
    # settled A/B switches: the shipped source has only the side that was kept
    # (whole names: the tunables KFX_RAY_HINT_T0 and KFX_INT_OCCL_CELLS stay)
    import re
    for m in ("KFX_INT_PK", "KFX_INT_BSKIP", "KFX_INT_LDALL", "KFX_INT_OCCL", "KFX_ICP_HIER", "KFX_ICP_XCD",
              "KFX_RAY_NG", "KFX_RAY_N32", "KFX_RAY_EXIT", "KFX_RAY_CHAIN", "KFX_RAY_SLAB_SKIP", "KFX_RAY_HINT",
              "KFX_EXTRACT_SKIP", "KFX_PREP_AFTER_ICP", "KFX_PREP_AFTER_INT", "KFX_PREP_SIG", "KFX_ORDER_OFF_PATH",
              "KFX_FREE_ELIDE"):
        assert not re.search(r"\b" + m + r"\b", src), m


def test_adapter_header_compiles_and_links(tmp_path):
    """adapter/kinectfusion.h (the reference's kf::kinectfusion over the C-ABI)
    compiled with a main.cpp-like driver against stand-ins for the few OpenCV
    core types it uses (OpenCV is not in this image) and linked to libkfx.so.
    Without a GPU the program reports the missing device and exits 2."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    stub = os.path.join(root, "tests", "adapter_stub")
    lib = os.path.join(root, "slam-kinectfusion_amd", "lib")
    exe = str(tmp_path / "main_like")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", stub,
                        "-I", os.path.join(root, "slam-kinectfusion_amd", "adapter"),
                        os.path.join(stub, "main_like.cpp"), "-o", exe, "-L", lib, "-lkfx",
                        f"-Wl,-rpath,{lib}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    import torch
    if not torch.cuda.is_available():
        p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert p.returncode == 2 and "kinectfusion:" in p.stderr
