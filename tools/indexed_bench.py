#!/usr/bin/env python3
"""Device time of the indexed mesh on the bench's C2 workload (640x480, 512^3 @ 4
mm): after 30 frames of the bench's sequence, origin (0, 0, 0), one process.  Per form, median of 5
after one warm-up:
  window: kfx_extract_mesh_indexed (kfx_get_indexed_ms) against kfx_extract_mesh_attr
          (kfx_get_extract_ms, the sum of its three figures) on the same volume;
  world:  kfx_world_mesh_indexed against kfx_world_mesh_attr (kfx_get_world_ms), both on
          kfx_world_bricks() (the window's non-empty bricks, no store).
The yardstick is always the existing call, never the new code against itself.  Next to the device
figures: V, T and 3T / V, the bytes downloaded (28 V + 12 T against 84 T), the wall time of the
whole call (the binding's: a count-only call to size the buffers, then the filling call, against
the soup's one call into a buffer of T triangles) and the PLY sizes of kfx_save_mesh_attr against
kfx_save_mesh_indexed.  Writes one JSON record.
usage: [KFX_LIB_PATH=...] python3 tools/indexed_bench.py [out.json [parent commit]]"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "slam-kinectfusion_amd"))
import kfx  # noqa: E402
from kfx import synth  # noqa: E402
from kfx.abi import Intrinsics, default_params  # noqa: E402

WARM_FRAMES, REPS = 30, 5
N = 512


def stats(xs):
    xs = sorted(float(x) for x in xs)
    return {"min": xs[0], "median": xs[len(xs) // 2], "max": xs[-1], "all": xs}


def form(indexed, indexed_ms, soup, soup_ms):
    """One form: the indexed call and its yardstick, alternating, REPS times after one warm-up."""
    ims, sms, iwall, swall = {}, {}, [], []
    n_tris = len(indexed()[1])
    for r in range(REPS + 1):
        t0 = time.perf_counter()
        verts, tris = indexed()
        t1 = time.perf_counter()
        a = indexed_ms()
        t2 = time.perf_counter()
        s = soup(n_tris)
        t3 = time.perf_counter()
        b = {k: v for k, v in soup_ms().items() if k != "passes"}
        if r:
            iwall.append((t1 - t0) * 1e3)
            swall.append((t3 - t2) * 1e3)
            for k, v in a.items():
                ims.setdefault(k, []).append(v)
            for k, v in b.items():
                sms.setdefault(k, []).append(v)
    V, T = len(verts), len(tris)
    assert len(s) == T and verts[tris].tobytes() == s.tobytes()  # the same mesh
    i, y = {k: stats(v) for k, v in ims.items()}, {k: stats(v) for k, v in sms.items()}
    return {"vertices": V, "triangles": T, "soup_vertices_per_vertex": 3 * T / V if V else None,
            "indexed_ms": i, "indexed_ms_total_median": sum(v["median"] for v in i.values()),
            "yardstick_ms": y, "yardstick_ms_total_median": sum(v["median"] for v in y.values()),
            "indexed_bytes_downloaded": 28 * V + 12 * T, "yardstick_bytes_downloaded": 84 * T,
            "indexed_call_wall_ms": stats(iwall), "yardstick_call_wall_ms": stats(swall)}


def main():
    intr = synth.Intrinsics.vga()
    p = default_params(dims=N, range_m=2.048)
    bgr, dep, _ = synth.sequence(48, intr, L=2.048, noise=True, traj_seed=7, dropout=0.005)
    kf = kfx.KinectFusion(Intrinsics.from_any(intr), p)
    kf.stage_frames(bgr, dep.astype(np.float32))
    for i in synth.ping_pong(48, WARM_FRAMES):
        kf.pipeline_staged(int(i))
    kf.synchronize()
    assert kf.volume_origin == (0, 0, 0)
    commit = sys.argv[2] if len(sys.argv) > 2 else ""  # (a copy of the tree without its history: give it)
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                    text=True).stdout.strip()
        except OSError:
            pass
    bricks = kf.world_bricks()
    out = {
        "workload": "C2 640x480, 512^3 @ 4 mm, %d frames of the bench sequence (ping-pong over 48)" % WARM_FRAMES,
        "commit_parent": commit, "libkfx_sha256": hashlib.sha256(open(kfx.LIB_PATH, "rb").read()).hexdigest(),
        "unit": ("ms, device time between HIP events, median of %d after one warm-up: indexed = kfx_get_indexed_ms (table, "
                 "count = counts + scans, verts = vertex emit, tris = index emit), yardstick = kfx_get_extract_ms of "
                 "kfx_extract_mesh_attr (window) / kfx_get_world_ms of kfx_world_mesh_attr (world); wall = the binding's whole "
                 "call, transfers included (indexed: the sizing call and the filling call)") % REPS,
        "window": form(kf.extract_mesh_indexed, kf.indexed_ms, kf.extract_mesh_attr, kf.extract_ms),
        "world_bricks": len(bricks),
        "world": form(lambda: kf.world_mesh_indexed(bricks), kf.indexed_ms, lambda cap: kf.world_mesh(bricks, cap), kf.world_ms),
    }
    with tempfile.TemporaryDirectory() as d:
        kf.save_mesh_attr(os.path.join(d, "soup.ply"), cap=out["window"]["triangles"])
        kf.save_mesh_indexed(os.path.join(d, "indexed.ply"))
        out["ply_bytes"] = {"kfx_save_mesh_attr": os.path.getsize(os.path.join(d, "soup.ply")),
                            "kfx_save_mesh_indexed": os.path.getsize(os.path.join(d, "indexed.ply"))}
    kf.close()
    text = json.dumps(out, indent=1)
    if len(sys.argv) > 1 and sys.argv[1]:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: {"V": v["vertices"], "T": v["triangles"], "indexed_ms": v["indexed_ms_total_median"],
                          "yardstick_ms": v["yardstick_ms_total_median"]} for k, v in out.items()
                      if isinstance(v, dict) and "vertices" in v} | {"ply_bytes": out["ply_bytes"]}))


if __name__ == "__main__":
    main()
