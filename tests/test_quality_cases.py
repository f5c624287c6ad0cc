"""The quality record without a GPU: the crafted ICP cases reach every label at
every size (so the GPU parity in test_gpu_quality.py compares something), the
host-only kfx_quality_figures equals its numpy statement bit for bit, and the
record is the 64 bytes include/kfx.h says."""
import ctypes as C

import numpy as np
import pytest

import icp_cases as K
import kfx
import quality_cases as Q
from kfx.abi import IcpQuality

# identity-pose totals per label 0..4 over the case table (measured once on the numpy restatement)
TOTALS = {(32, 32): (7784, 121, 142, 76, 69), (80, 48): (15905, 67, 219, 96, 97), (96, 32): (23886, 145, 304, 114, 127)}


def record(n, sum_r2, max_abs_r=0.0, level=0):
    q = IcpQuality()
    for k in range(6):
        q.n[k] = n[k]
    q.sum_r2, q.max_abs_r, q.level = sum_r2, max_abs_r, level
    return q


def test_struct_is_64_bytes():
    assert C.sizeof(IcpQuality) == 64
    assert IcpQuality.sum_r2.offset == 48 and IcpQuality.max_abs_r.offset == 56 and IcpQuality.level.offset == 60


@pytest.mark.parametrize("size", Q.SIZES_1PX, ids=Q.sid)
def test_every_label_reached(size):
    w, h = size
    xe, ye = K.region(w, h)
    lo, hi = None, None
    for moved in (False, True):
        tot = [0] * 6
        for name in K.case_table():
            r = Q.crafted_ref(name, w, h, moved)
            assert r.n[5] == w * h - xe * ye
            acc = r.residual[r.label == 0]
            assert acc.size and np.isfinite(acc).all() and acc.any()
            assert r.sum_r2 > 0 and float(r.max_abs_r) == float(abs(acc).max())
            assert not r.residual[r.label != 0].any()
            for k in range(6):
                tot[k] += r.n[k]
            lo = r.sum_r2 if lo is None else min(lo, r.sum_r2)
            hi = r.sum_r2 if hi is None else max(hi, r.sum_r2)
        assert all(tot[k] > 0 for k in range(5)), tot
        if not moved:
            assert tuple(tot[:5]) == TOTALS[size]
    print(f"{w}x{h}: sum_r2 {lo} .. {hi}")


def test_label5_at_80x48():
    r = Q.crafted_ref("a_invalid", 80, 48, False)
    assert r.n[5] == 80 * 48 - 64 * 32
    assert (r.label[:, 64:] == 5).all() and (r.label[32:, :] == 5).all() and not (r.label[:32, :64] == 5).any()


def test_figures_bit_for_bit():
    recs = [Q.crafted_ref(name, w, h, moved) for name in K.case_table() for w, h in Q.SIZES_1PX
            for moved in (False, True)]
    cases = [(r.n, r.sum_r2) for r in recs]
    cases += [([0] * 6, 0), ([0, 5, 7, 9, 11, 13], 0), ([0, 0, 0, 0, 0, 100], 0), ([1000, 0, 24, 0, 0, 0], 0),
              ([3, 1, 2, 3, 4, 5], 1), ([2 ** 40, 0, 1, 0, 0, 0], 2 ** 62), ([7, 0, 0, 0, 0, 0], 2 ** 53 + 1)]
    for n, s in cases:
        assert kfx.quality_figures(record(n, s)) == Q.figures_np(n, s), (n, s)
    assert kfx.quality_figures(record([0] * 6, 0)) == (0.0, 0.0)
    assert kfx.quality_figures(record([0, 3, 4, 5, 6, 7], 99)) == (0.0, 0.0)
    fit, rmse = kfx.quality_figures(record([30, 5, 10, 0, 0, 0], 0))
    assert fit == 0.75 and rmse == 0.0


def test_figures_argument_errors():
    L = kfx.lib()
    a, b = C.c_double(), C.c_double()
    q = record([1, 0, 0, 0, 0, 0], 1)
    assert L.kfx_quality_figures(C.byref(q), C.byref(a), C.byref(b)) == 0
    assert L.kfx_quality_figures(None, C.byref(a), C.byref(b)) == -1
    assert L.kfx_quality_figures(C.byref(q), None, C.byref(b)) == -1
    assert L.kfx_quality_figures(C.byref(q), C.byref(a), None) == -1
    for k in range(6):
        bad = record([1] * 6, 1)
        bad.n[k] = -1
        assert L.kfx_quality_figures(C.byref(bad), C.byref(a), C.byref(b)) == -1
    assert L.kfx_last_error()


def test_chunk_rule():
    for w, h in [(32, 32), (80, 48), (160, 120), (320, 240), (640, 480), (1280, 720)]:
        for n in (1, 2, 3, 16, 27, 64, 130, 256, 4096, 65536):
            assert kfx.quality_chunk(w, h, n) == Q.chunk_np(w, h, n), (w, h, n)
    assert Q.chunk_np(160, 120, 256) == 9 and Q.chunk_np(320, 240, 130) == 16 and Q.chunk_np(80, 48, 130) == 1
    L = kfx.lib()
    assert L.kfx_quality_chunk(0, 4, 1) == -1 and L.kfx_quality_chunk(4, 4, 0) == -1
