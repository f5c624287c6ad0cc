#!/usr/bin/env python3
"""Device time of kfx_world_view against kfx_render_view on the
bench's C2 workload (640x480, 512^3 @ 4 mm) after 20 frames of the bench's
sequence.  First record: world_bricks() loaded with the box set to the window,
so both calls produce the same bytes (checked here) and the ratio prices the
brick indirection alone: Phong, colour and colour plus maps at the tracked
pose, at tools/view_bench.py's off-trajectory and oblique views and at
1280x720, 5 repetitions each after a warm-up, min / median / max.  Second
record: the window moved by one shift with a brick store, the world (window
plus store) in its default box: a world larger than the window.  The load is
reported as device work (world_view_ms()["load"]) and as the wall time of the
whole call, upload included.  Prints one JSON record.
usage: [KFX_LIB_PATH=...] python3 tools/world_view_bench.py [out.json [parent commit]]"""
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

FRAMES, REPS = 20, 5
MODES = (("phong", False), ("color", False), ("color", True))


def rot(axis, ang):
    c, s = np.cos(ang), np.sin(ang)
    m = np.eye(4)
    i, j = {"x": (1, 2), "y": (2, 0)}[axis]
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def off_pose(last, tx, ay, ax):
    T = np.eye(4)
    T[:3, 3] = (tx, 0.05, -0.1)
    return (last.astype(np.float64) @ T @ rot("y", ay) @ rot("x", ax)).astype(np.float32)


def stats(xs):
    xs = sorted(float(x) for x in xs)
    return {"min": xs[0], "median": xs[len(xs) // 2], "max": xs[-1], "all": xs}


def timed(call, ms):
    call()  # warm-up (first use also allocates)
    out = []
    for _ in range(REPS):
        call()
        out.append(ms())
    return stats(out)


def load(kf, bricks, box):
    t0 = time.perf_counter()
    kf.world_view_load(bricks, box=box)
    wall = 1e3 * (time.perf_counter() - t0)
    return {"bricks": int(len(bricks)), "record_MB": len(bricks) * 3600 / 1e6, "device_ms": kf.world_view_ms()["load"],
            "wall_ms_with_upload": wall}


def main():
    intr = synth.Intrinsics.vga()
    I = Intrinsics.from_any(intr)
    p = default_params(dims=512, range_m=2.048)
    bgr, dep, _ = synth.sequence(48, intr, L=2.048, noise=True, traj_seed=7, dropout=0.005)
    order = synth.ping_pong(48, FRAMES)
    kf = kfx.KinectFusion(I, p)
    kf.stage_frames(bgr, dep.astype(np.float32))
    for i in order[:FRAMES]:
        kf.pipeline_staged(int(i))
    kf.synchronize()
    last = kf.pose_record[-1]

    def scaled(W, H, s):  # tools/view_bench.py's off-centre intrinsics
        return Intrinsics(W, H, float(intr.fx * s), float(intr.fy * s * 1.02), W / 2 - 0.5 + 3.25, H / 2 - 0.5 - 1.5)

    views = {
        "tracked_pose_640x480": (I, last),
        "off_trajectory_640x480": (scaled(640, 480, 0.55), off_pose(last, -0.45, 0.35, -0.1)),
        "oblique_640x480": (scaled(640, 480, 0.3), off_pose(last, 0.4, -0.3, 0.15)),
        "tracked_pose_1280x720": (Intrinsics.from_any(synth.Intrinsics.hd720()), last),
    }
    bricks = kf.world_bricks()
    first = {"load": load(kf, bricks, (kf.volume_origin, (512, 512, 512))), "views": {}}
    for name, (vi, vp) in views.items():
        rec = {}
        for kind, maps in MODES:
            key = kind + ("+maps" if maps else "")
            w = kf.world_view(vi, vp, kind, maps=maps)
            d = kf.render_view(vi, vp, kind, maps=maps)
            same = all(a.tobytes() == b.tobytes() for a, b in zip(w if maps else (w,), d if maps else (d,)))
            rec[key] = {
                "world_view": timed(lambda: kf.world_view(vi, vp, kind, maps=maps), lambda: kf.world_view_ms()["render"]),
                "render_view": timed(lambda: kf.render_view(vi, vp, kind, maps=maps), kf.view_ms),
                "same_bytes": bool(same),
            }
            rec[key]["ratio_of_medians"] = rec[key]["world_view"]["median"] / rec[key]["render_view"]["median"]
        rec["hit_fraction"] = float((kf.world_view(vi, vp, "phong", maps=True)[3] != 0).mean())
        first["views"][name] = rec

    # a world larger than the window: one shift, what it drops kept in a store
    shift = (64, 0, 0)
    second = {"shift": list(shift)}
    with kfx.BrickStore() as store:
        store.put(kf.evict_bricks(shift))
        kf.shift_volume(shift)
        world = kf.world_bricks(store)
        second["held_in_store"] = len(store)
        second["load"] = load(kf, world, None)
        vi, vp = views["tracked_pose_640x480"]
        rec = {}
        for kind, maps in MODES:
            rec[kind + ("+maps" if maps else "")] = {
                "world_view": timed(lambda: kf.world_view(vi, vp, kind, maps=maps), lambda: kf.world_view_ms()["render"]),
                "render_view_window_only": timed(lambda: kf.render_view(vi, vp, kind, maps=maps), kf.view_ms),
            }
        rec["hits_world"] = int((kf.world_view(vi, vp, "phong", maps=True)[3] != 0).sum())
        rec["hits_window"] = int((kf.render_view(vi, vp, "phong", maps=True)[3] != 0).sum())
        second["tracked_pose_640x480"] = rec
    kf.close()
    commit = sys.argv[2] if len(sys.argv) > 2 else ""  # (a copy of the tree without its history: give it)
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                    text=True).stdout.strip()
        except OSError:
            pass
    out = {
        "workload": "C2 640x480, 512^3 @ 4 mm, %d frames of the bench sequence (ping-pong over 48)" % FRAMES,
        "unit": "ms, device time between HIP events around the launch (load: around its memsets and kernel)",
        "commit_parent": commit,
        "libkfx_sha256": hashlib.sha256(open(kfx.LIB_PATH, "rb").read()).hexdigest(),
        "window_box": first,
        "window_plus_store": second,
    }
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
