"""The host-only brick store of the moving volume (csrc/kfx_brick_store.cpp):
through libkfx against a dict restatement, and as the stand-alone program
tests/brickstore/store_check.cpp, compiled together with the store's source plain and under
ASan + UBSan and run directly.  No GPU anywhere."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from kfx import BRICK_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "tests", "brickstore", "store_check.cpp"),
       os.path.join(ROOT, "slam-kinectfusion_amd", "csrc", "kfx_brick_store.cpp")]
BUILDS = {
    "O2": ["-O2"],
    "asan_ubsan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}


def bricks(coords, seed):
    rng = np.random.default_rng(seed)
    out = np.zeros(len(coords), BRICK_DTYPE)
    out["b"] = coords
    out["tsdf"] = rng.integers(-32767, 32768, (len(coords), 512))
    out["weight"] = rng.integers(0, 256, (len(coords), 512))
    out["rgb"][:, :, :3] = rng.integers(0, 256, (len(coords), 512, 3))
    return out


def window_keys(held, origin, dims):
    lo = [o // 8 for o in origin]
    hi = [lo[k] + (dims[k] + 7) // 8 for k in range(3)]
    return sorted((k for k in held if all(lo[a] <= k[a] < hi[a] for a in range(3))), key=lambda k: (k[2], k[1], k[0]))


def test_put_replace_and_take_against_a_dict(kfx_lib):
    rng = np.random.default_rng(3)
    held = {}
    with kfx_lib.BrickStore() as st:
        assert len(st) == 0 and len(st.take_window((0, 0, 0), (64, 64, 64))) == 0
        for rnd in range(12):
            coords = rng.integers(-5, 9, (40, 3))  # repeats inside a batch and across batches
            b = bricks(coords, 100 + rnd)
            st.put(b)
            for r in b:
                held[tuple(int(x) for x in r["b"])] = r.copy()
            assert len(st) == len(held)
            # negative origins; dims that are no multiple of 8 (Z = 44: six bricks deep)
            origin = tuple(int(8 * x) for x in rng.integers(-5, 5, 3))
            dims = [(64, 64, 64), (128, 64, 32), (64, 40, 44), (8, 8, 1)][rnd % 4]
            want = window_keys(held, origin, dims)
            got = st.take_window(origin, dims)
            assert [tuple(int(x) for x in r["b"]) for r in got] == want, (origin, dims)
            assert got.tobytes() == np.array([held.pop(k) for k in want], BRICK_DTYPE).tobytes()
            assert len(st) == len(held)
            assert len(st.take_window(origin, dims)) == 0  # taken means gone
        assert len(held) > 0
        everything = st.take_window((-64, -64, -64), (160, 160, 160))
        assert len(everything) == len(held) and len(st) == 0
        order = np.lexsort((everything["b"][:, 0], everything["b"][:, 1], everything["b"][:, 2]))
        assert np.array_equal(order, np.arange(len(everything)))


def test_a_short_buffer_takes_nothing(kfx_lib):
    L = kfx_lib.lib()
    with kfx_lib.BrickStore() as st:
        b = bricks([(0, 0, 0), (1, 0, 0), (0, 1, 0), (7, 7, 7), (8, 0, 0)], 1)
        st.put(b)
        o, d, n = (C.c_int * 3)(0, 0, 0), (C.c_int * 3)(64, 64, 64), C.c_int64()
        out = np.full(4, 0xAB, np.uint8).repeat(3600).view(BRICK_DTYPE)
        assert L.kfx_brick_store_take_window(st._h, o, d, out.ctypes.data_as(C.c_void_p), 3, C.byref(n)) == 0
        assert n.value == 4 and len(st) == 5 and (out.view(np.uint8) == 0xAB).all()
        assert L.kfx_brick_store_take_window(st._h, o, d, None, 0, C.byref(n)) == 0 and n.value == 4 and len(st) == 5
        assert L.kfx_brick_store_take_window(st._h, o, d, out.ctypes.data_as(C.c_void_p), 4, C.byref(n)) == 0
        assert n.value == 4 and len(st) == 1
        assert out.tobytes() == b[[0, 1, 2, 3]].tobytes()  # (8, 0, 0) lies outside 64 voxels


def test_argument_errors(kfx_lib):
    L = kfx_lib.lib()
    assert L.kfx_brick_store_create(None) == -1
    with kfx_lib.BrickStore() as st:
        b = bricks([(0, 0, 0)], 2)
        p = b.ctypes.data_as(C.c_void_p)
        o, d, n = (C.c_int * 3)(0, 0, 0), (C.c_int * 3)(64, 64, 64), C.c_int64()
        assert L.kfx_brick_store_put(None, p, 1) == -1
        assert L.kfx_brick_store_put(st._h, None, 1) == -1
        assert L.kfx_brick_store_put(st._h, p, -1) == -1
        assert L.kfx_brick_store_put(st._h, None, 0) == 0
        assert L.kfx_brick_store_count(None, C.byref(n)) == -1 and L.kfx_brick_store_count(st._h, None) == -1
        assert L.kfx_brick_store_take_window(None, o, d, p, 1, C.byref(n)) == -1
        assert L.kfx_brick_store_take_window(st._h, None, d, p, 1, C.byref(n)) == -1
        assert L.kfx_brick_store_take_window(st._h, o, None, p, 1, C.byref(n)) == -1
        assert L.kfx_brick_store_take_window(st._h, o, d, p, 1, None) == -1
        assert L.kfx_brick_store_take_window(st._h, o, d, None, 1, C.byref(n)) == -1
        assert L.kfx_brick_store_take_window(st._h, o, d, p, -1, C.byref(n)) == -1
        assert L.kfx_brick_store_take_window(st._h, (C.c_int * 3)(0, 0, 12), d, p, 1, C.byref(n)) == -1
        assert b"multiples of 8" in L.kfx_last_error()
        assert L.kfx_brick_store_take_window(st._h, o, (C.c_int * 3)(64, 64, 0), p, 1, C.byref(n)) == -1
        assert L.kfx_brick_store_destroy(None) == -1
        assert len(st) == 0


@pytest.fixture(scope="module")
def executables(tmp_path_factory):
    out = {}
    for name, flags in BUILDS.items():
        out[name] = str(tmp_path_factory.mktemp("brickstore_" + name) / "store_check")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, *SRC, "-o", out[name]], check=True)
    return out


@pytest.mark.parametrize("build", list(BUILDS))
def test_standalone_store_check(executables, build):
    r = subprocess.run([executables[build]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    m = re.search(r"store_check ok: (\d+) puts, (\d+) taken in (\d+) windows, (\d+) refused takes", r.stdout)
    assert m, r.stdout
    print(r.stdout.strip())
    assert int(m.group(1)) > 500 and int(m.group(2)) > 100 and int(m.group(4)) > 10
