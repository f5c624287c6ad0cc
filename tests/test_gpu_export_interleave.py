"""The exports share one count / scan / emit driver: no state crosses between them.

smoke()'s run (QVGA, 64^3 over 2.048 m, 4 frames).  Each of extract_points, extract_mesh_attr,
evict_points((8, 0, 0)), evict_bricks((8, 0, 0)), world_points and world_mesh (of world_bricks())
alone on a fresh context gives the expected bytes.  Then on one context they run in two orders,
each at cap 0, half the total and the total: every result equals the expectation's prefix byte for
byte and every call reports the full count.  Around every call the timing getters of the other
kinds return what they returned before it; a zero shift evicts nothing and leaves a finite span;
and the pass count follows kfx_set_extract_passes as tests/test_gpu_extract_paths.py expects."""
import ctypes as C
import math

import numpy as np
import pytest

import kfx
from kfx import BRICK_DTYPE, KFX_OK, VERTEX_DTYPE, KinectFusion, synth
from kfx.abi import Intrinsics, default_params

pytestmark = pytest.mark.gpu
VDT = np.dtype(VERTEX_DTYPE)
SHIFT = (8, 0, 0)
KINDS = ("extract_points", "extract_mesh_attr", "evict_points", "evict_bricks", "world_points", "world_mesh")
ORDERS = (KINDS, ("world_mesh", "evict_bricks", "extract_mesh_attr", "world_points", "evict_points", "extract_points"))
# the getter a kind's call may change: (getter, key or None for all of it)
OWN = {"extract_points": ("extract_ms", None), "extract_mesh_attr": ("extract_ms", None),
       "evict_points": ("shift_ms", "evict"), "evict_bricks": ("stream_ms", "evict_bricks"),
       "world_points": ("world_ms", None), "world_mesh": ("world_ms", None)}


def run_frames():
    intr = synth.Intrinsics.qvga()
    bgr, dep, _ = synth.sequence(4, intr)
    kf = KinectFusion(Intrinsics.from_any(intr), default_params(dims=64, range_m=2.048), device=0)
    for k in range(len(dep)):
        assert kf.pipeline(bgr[k], dep[k].astype(np.float32)) == KFX_OK
    return kf


def call(kf, kind, cap, bricks=None):
    """(items written, total reported) of one C-ABI call with a buffer of cap items."""
    L, n = kfx.lib(), C.c_int64(-1)
    shape, dt = {"extract_points": ((cap, 3), np.float32), "extract_mesh_attr": ((cap, 3), VDT),
                 "evict_points": ((cap,), VDT), "evict_bricks": ((cap,), BRICK_DTYPE),
                 "world_points": ((cap,), VDT), "world_mesh": ((cap, 3), VDT)}[kind]
    out = np.zeros(shape, dt)
    o = out.ctypes.data_as(C.POINTER(C.c_float) if kind == "extract_points" else C.c_void_p) if cap > 0 else None
    if kind.startswith("extract"):
        r = getattr(L, "kfx_" + kind)(kf._h, o, cap, C.byref(n))
    elif kind.startswith("evict"):
        r = getattr(L, "kfx_" + kind)(kf._h, (C.c_int * 3)(*SHIFT), o, cap, C.byref(n))
    else:
        r = getattr(L, "kfx_" + kind + "_attr")(kf._h, bricks.ctypes.data_as(C.c_void_p), len(bricks), o, cap, C.byref(n))
    assert r == KFX_OK, (kind, cap, L.kfx_last_error())
    return out[:min(n.value, cap)], n.value


def getters(kf):
    return {"extract_ms": kf.extract_ms(), "shift_ms": kf.shift_ms(), "stream_ms": kf.stream_ms(),
            "world_ms": kf.world_ms()}


def others(snapshot, kind):
    """The snapshot without what a call of `kind` may change."""
    name, key = OWN[kind]
    s = {k: dict(v) for k, v in snapshot.items()}
    if key is None:
        del s[name]
    else:
        del s[name][key]
    return s


@pytest.fixture(scope="module")
def expected():
    want = {}
    for kind in KINDS:
        kf = run_frames()
        try:
            bricks = kf.world_bricks() if kind.startswith("world") else None
            total = call(kf, kind, 0, bricks)[1]
            items, again = call(kf, kind, total, bricks)
            assert again == total and len(items) == total
            want[kind] = items.copy()
        finally:
            kf.close()
    return want


def test_surface_is_not_empty(expected):
    for kind in KINDS:
        assert len(expected[kind]) >= 2, kind  # (so that half the total is a cap that cuts)
    print({k: len(v) for k, v in expected.items()})


@pytest.mark.parametrize("order", range(len(ORDERS)))
def test_interleaved_calls(expected, order):
    kf = run_frames()
    try:
        bricks = kf.world_bricks()
        for frac in (0, 1, 2):  # cap 0, half the total, the total
            for kind in ORDERS[order]:
                want = expected[kind]
                cap = len(want) * frac // 2
                before = getters(kf)
                got, total = call(kf, kind, cap, bricks)
                assert total == len(want), (kind, cap)
                assert got.tobytes() == want[:cap].tobytes(), (kind, cap)
                after = getters(kf)
                assert others(after, kind) == others(before, kind), (kind, cap)
                name, key = OWN[kind]
                own = after[name] if key is None else {key: after[name][key]}
                assert all(math.isfinite(v) and v >= 0 for v in own.values()), (kind, own)
    finally:
        kf.close()


def test_zero_shift_and_pass_count(expected):
    kf = run_frames()
    try:
        L, n = kfx.lib(), C.c_int64(-1)
        zero = (C.c_int * 3)(0, 0, 0)
        buf = np.zeros(4, VDT)
        before = getters(kf)
        assert L.kfx_evict_points(kf._h, zero, buf.ctypes.data_as(C.c_void_p), 4, C.byref(n)) == KFX_OK and n.value == 0
        ms = kf.shift_ms()["evict"]
        assert math.isfinite(ms) and ms >= 0
        assert others(getters(kf), "evict_points") == others(before, "evict_points")
        before = getters(kf)
        assert kf.evict_brick_count((0, 0, 0)) == 0
        ms = kf.stream_ms()["evict_bricks"]
        assert math.isfinite(ms) and ms >= 0
        assert others(getters(kf), "evict_bricks") == others(before, "evict_bricks")
        # a capped call under two passes, then under one: the pool overflows at a cap below the total
        for kind in ("extract_points", "extract_mesh_attr"):
            want = expected[kind]
            half = len(want) // 2
            kf.set_extract_passes(2)
            got, total = call(kf, kind, half)
            assert kf.extract_ms()["passes"] == 2 and total == len(want) and got.tobytes() == want[:half].tobytes()
            kf.set_extract_passes(1)
            got, total = call(kf, kind, half)
            assert kf.extract_ms()["passes"] == 2 and total == len(want) and got.tobytes() == want[:half].tobytes()
            got, total = call(kf, kind, len(want) + 5)  # room for every item: one pass
            assert kf.extract_ms()["passes"] == 1 and total == len(want) and got.tobytes() == want.tobytes()
            ms = kf.extract_ms()
            assert all(math.isfinite(ms[k]) and ms[k] >= 0 for k in ("count", "scan", "emit")) and ms["emit"] > 0
            assert call(kf, kind, 0)[1] == len(want)  # count only: no emit
            assert kf.extract_ms()["emit"] == 0.0
    finally:
        kf.close()
