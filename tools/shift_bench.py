#!/usr/bin/env python3
"""Device time of the moving volume on the bench's C2 workload
(640x480, 512^3 @ 4 mm): after 30 frames of the bench's sequence, for each of
the shifts (0,0,8), (8,0,0), (0,8,0), (8,8,8) and (0,0,64): kfx_evict_points
(all of them first: it changes nothing), then kfx_shift_volume followed by the
restoring shift (which brings the pose back; the dropped slab stays empty, and
the time of the move does not depend on the contents), 5 repetitions after one
warm-up, HIP-event ms from kfx_get_shift_ms.  For comparison the only route without it, in the same
process: download_tsdf + upload_tsdf wall time (a new context with another
volu_pose comes on top).  Bytes moved = 7 bytes read and 7 written per voxel
that has a source in the volume, 7 written per cleared voxel (the occupancy
rebuild reads the 2-byte tsdf once more; it is part of the timed span).
Prints one JSON record.

Next to each shift, the bricks out and back in: kfx_evict_bricks
of the shift (count + scan + emit, kfx_get_stream_ms) and kfx_restore_bricks of
those bricks over the places they came from (the contents stay what they were;
the time of the restore does not depend on where the window stands), the same 5
repetitions after one warm-up, with the brick counts.  Bytes moved: the count
pass reads 512 B of a brick that shows a weight and all 3584 B of an empty one,
the emit pass reads 3584 B and writes 3600 B per brick; the restore reads 3600
B and writes 3584 B per brick and clears the settled bytes.  A second JSON
record, written to the third argument.

The world map, a third JSON record, written to the fourth
argument: after the 30 frames and before any shift, kfx_world_points_attr and
kfx_world_mesh_attr of kfx_world_bricks() (the window's non-empty bricks, no
store), device ms of the neighbour table, count + scan and emit from
kfx_get_world_ms, and next to them kfx_extract_points_attr /
kfx_extract_mesh_attr of the same window in the same process (kfx_get_extract_ms)
as the yardstick; median of 5 after one warm-up, with the brick count, the
items and the bytes read.  The upload of the records over PCIe (3600 B per
brick and call) is not in the device figures; the call's wall time is given
next to them.  With the first and third argument empty only this part runs.
usage: [KFX_LIB_PATH=...] python3 tools/shift_bench.py [out.json [parent commit [stream_out.json [world_out.json]]]]
       (an empty out.json skips that file)"""
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "slam-kinectfusion_amd"))
import kfx  # noqa: E402
from kfx import synth  # noqa: E402
from kfx.abi import Intrinsics, default_params  # noqa: E402

WARM_FRAMES, REPS = 30, 5
SHIFTS = ((0, 0, 8), (8, 0, 0), (0, 8, 0), (8, 8, 8), (0, 0, 64))
COPY_TBS = 6.29  # the measured device copy rate the floor is derived from
N = 512


def stats(xs):
    xs = sorted(float(x) for x in xs)
    return {"min": xs[0], "median": xs[len(xs) // 2], "max": xs[-1], "all": xs}


def world_bench(kf):
    """The world map against the dense extractors on the volume as it stands."""
    bricks = kf.world_bricks()
    n = len(bricks)
    negative = int((bricks["tsdf"].reshape(n, -1) < 0).any(1).sum())
    out = {"bricks": n, "bricks_with_a_negative_tsdf": negative, "record_bytes": 3600 * n}
    for mesh in (False, True):
        parts, wall, dense, items, ditems = {"table": [], "count": [], "emit": []}, [], {"count": [], "scan": [], "emit": []}, 0, 0
        passes = 0
        for r in range(REPS + 1):  # the first repetition warms up (buffers, events, kernels)
            t0 = time.perf_counter()
            items = len(kf.world_mesh(bricks) if mesh else kf.world_points(bricks))
            t1 = time.perf_counter()
            ms = kf.world_ms()
            ditems = len(kf.extract_mesh_attr() if mesh else kf.extract_points_attr())
            dms = kf.extract_ms()
            passes = dms["passes"]
            if r:
                wall.append((t1 - t0) * 1e3)
                for k in parts:
                    parts[k].append(ms[k])
                for k in dense:
                    dense[k].append(dms[k])
        w = {k: stats(v) for k, v in parts.items()}
        d = {k: stats(v) for k, v in dense.items()}
        out["mesh" if mesh else "points"] = {
            "items": items, "item_bytes_written": items * (84 if mesh else 28),
            "world_ms": w, "world_ms_total_median": sum(w[k]["median"] for k in w),
            "world_call_wall_ms": stats(wall),
            # the count pass gathers every brick's tile: 363 x-rows of 16 B of tsdf + 8 B of weight (each record is
            # read by up to 27 tiles; the repeats hit the caches); the emit pass gathers the bricks with items
            # only, 32 B of colour per row too
            "count_gather_bytes_requested": 363 * 24 * n, "emit_gather_bytes_per_brick_with_items": 363 * 56,
            "window_items": ditems, "window_extract_ms": d, "window_extract_passes": passes,
            "window_extract_ms_total_median": sum(d[k]["median"] for k in d),
        }
    return out


def main():
    intr = synth.Intrinsics.vga()
    p = default_params(dims=N, range_m=2.048)
    bgr, dep, _ = synth.sequence(48, intr, L=2.048, noise=True, traj_seed=7, dropout=0.005)
    kf = kfx.KinectFusion(Intrinsics.from_any(intr), p)
    kf.stage_frames(bgr, dep.astype(np.float32))
    for i in synth.ping_pong(48, WARM_FRAMES):
        kf.pipeline_staged(int(i))
    kf.synchronize()
    commit = sys.argv[2] if len(sys.argv) > 2 else ""  # (a copy of the tree without its history: give it)
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                    text=True).stdout.strip()
        except OSError:
            pass
    workload = "C2 640x480, 512^3 @ 4 mm, %d frames of the bench sequence (ping-pong over 48)" % WARM_FRAMES
    sha = hashlib.sha256(open(kfx.LIB_PATH, "rb").read()).hexdigest()
    if len(sys.argv) > 4 and sys.argv[4]:
        wout = {"workload": workload, "commit_parent": commit, "libkfx_sha256": sha,
                "unit": ("ms, device time between HIP events: world = neighbour table, count + scan, emit "
                         "(kfx_get_world_ms; neither the upload of the records nor the download of the items), window = "
                         "kfx_get_extract_ms of kfx_extract_*_attr; wall = the whole world call, upload and download included"),
                "world": world_bench(kf)}
        with open(sys.argv[4], "w") as f:
            f.write(json.dumps(wout, indent=1) + "\n")
        print(json.dumps({k: {"items": v["items"], "world_ms": v["world_ms_total_median"],
                              "window_ms": v["window_extract_ms_total_median"]}
                          for k, v in wout["world"].items() if isinstance(v, dict)}))
        if not (len(sys.argv) > 1 and sys.argv[1]) and not sys.argv[3]:
            kf.close()
            return
    nvox = N ** 3
    rec, evicted, evict_ms = {}, {}, {}
    for s in SHIFTS:  # every eviction before the first shift: it changes nothing, and the slabs still hold their surfaces
        ev, items = [], 0
        for r in range(REPS + 1):  # the first repetition warms up (first use creates the events, loads the kernels)
            items = len(kf.evict_points(s))
            if r:
                ev.append(kf.shift_ms()["evict"])
        evicted[str(s)], evict_ms[str(s)] = items, stats(ev)
    stream = {}
    for s in SHIFTS:  # the bricks of the same slabs, out and back over themselves: the volume stays as it is
        eb, rb, bricks = [], [], None
        for r in range(REPS + 1):
            bricks = kf.evict_bricks(s)
            if r:
                eb.append(kf.stream_ms()["evict_bricks"])
        for r in range(REPS + 1):
            assert kf.restore_bricks(bricks) == len(bricks)
            if r and len(bricks):  # (an empty list does no device work and leaves the last figure standing)
                rb.append(kf.stream_ms()["restore_bricks"])
        cells = (N // 8) ** 3 - int(np.prod([N // 8 - abs(x) // 8 for x in s]))
        nb = len(bricks)
        weighted = int((bricks["weight"].reshape(nb, 512) != 0).any(1).sum())
        e, h = stats(eb), (stats(rb) if rb else None)
        out_bytes = 512 * weighted + 3584 * (cells - weighted) + (3584 + 3600) * nb
        in_bytes = (3600 + 3584) * nb + (N // 8) ** 3
        stream[str(s)] = {"cells_dropped": cells, "bricks": nb, "record_bytes": 3600 * nb,
                          "evict_bricks_ms": e, "evict_bytes_moved": out_bytes,
                          "evict_achieved_TBps": out_bytes / (e["median"] * 1e-3) / 1e12 if e["median"] > 0 else 0.0,
                          "restore_bricks_ms": h, "restore_bytes_moved": in_bytes,
                          "restore_achieved_TBps": in_bytes / (h["median"] * 1e-3) / 1e12 if h and h["median"] > 0 else None}
    for s in SHIFTS:
        back = tuple(-x for x in s)
        kept = int(np.prod([N - abs(x) for x in s]))
        moved = 14 * kept + 7 * (nvox - kept)
        sh = []
        for r in range(REPS + 1):
            kf.shift_volume(s)
            ms = kf.shift_ms()["shift"]
            kf.shift_volume(back)
            if r:
                sh.append(ms)
        e, h, items = evict_ms[str(s)], stats(sh), evicted[str(s)]
        tbs = moved / (h["median"] * 1e-3) / 1e12
        rec[str(s)] = {"evict_ms": e, "evicted_items": items, "shift_ms": h, "bytes_moved": moved,
                       "achieved_TBps": tbs, "fraction_of_copy_rate": tbs / COPY_TBS,
                       "floor_ms_at_copy_rate": moved / (COPY_TBS * 1e12) * 1e3}
    assert kf.volume_origin == (0, 0, 0)
    route = []
    for _ in range(3):
        t0 = time.perf_counter()
        r = kf.download_tsdf()
        t1 = time.perf_counter()
        kf.upload_tsdf(r)
        t2 = time.perf_counter()
        route.append({"download_ms": (t1 - t0) * 1e3, "upload_ms": (t2 - t1) * 1e3, "total_ms": (t2 - t0) * 1e3})
    kf.close()
    out = {
        "workload": workload,
        "unit": "ms, device time between HIP events around the launches (kfx_get_shift_ms); the host route: wall ms",
        "commit_parent": commit,
        "libkfx_sha256": sha,
        "copy_rate_TBps": COPY_TBS,
        "shifts": rec,
        "host_route_download_upload": sorted(route, key=lambda x: x["total_ms"])[len(route) // 2],
        "host_route_bytes": 2 * 8 * nvox,
    }
    if len(sys.argv) > 3:
        sout = {k: out[k] for k in ("workload", "commit_parent", "libkfx_sha256", "copy_rate_TBps")}
        sout["unit"] = ("ms, device time between HIP events (kfx_get_stream_ms): evict_bricks = count + scan + emit "
                        "without the copy to the host, restore_bricks = memsets + launch without the upload")
        sout["set_against"] = "host_route_download_upload of profiles/shift_bench.json (145 ms)"
        sout["host_route_download_upload"] = out["host_route_download_upload"]
        sout["shifts"] = stream
        with open(sys.argv[3], "w") as f:
            f.write(json.dumps(sout, indent=1) + "\n")
    out["stream"] = {k: {"bricks": v["bricks"], "evict_bricks_ms": v["evict_bricks_ms"]["median"],
                         "restore_bricks_ms": v["restore_bricks_ms"] and v["restore_bricks_ms"]["median"]}
                     for k, v in stream.items()}
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1 and sys.argv[1]:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
