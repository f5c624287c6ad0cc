#!/usr/bin/env python3
"""Device time of kfx_render_view on the bench's C2 workload
(640x480, 512^3 @ 4 mm): 20 frames of the bench's sequence, the last 5 of them
timed one by one for the yardstick (the frame's own raycast stage,
kernel_timing()["raycast"]: march + resize + 24 B/pixel of map stores), then
view_ms() of every type at the last tracked pose with the context's
intrinsics, at two off-trajectory views scaled to 640x480 and at one 1280x720
view, 5 repetitions each after a warm-up.  Prints one JSON record.
usage: [KFX_LIB_PATH=...] python3 tools/view_bench.py [out.json [parent commit]]"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "slam-kinectfusion_amd"))
import kfx  # noqa: E402
from kfx import synth  # noqa: E402
from kfx.abi import Intrinsics, default_params  # noqa: E402

FRAMES, TIMED, REPS = 20, 5, 5
KINDS = ("phong", "normal", "color")


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


def main():
    intr = synth.Intrinsics.vga()
    I = Intrinsics.from_any(intr)
    p = default_params(dims=512, range_m=2.048)
    bgr, dep, _ = synth.sequence(48, intr, L=2.048, noise=True, traj_seed=7, dropout=0.005)
    order = synth.ping_pong(48, FRAMES)
    kf = kfx.KinectFusion(I, p)
    kf.stage_frames(bgr, dep.astype(np.float32))
    for i in order[:FRAMES - TIMED]:
        kf.pipeline_staged(int(i))
    kf.synchronize()
    kf.set_kernel_timing(1, 8)
    ray = []
    for i in order[FRAMES - TIMED:]:
        kf.pipeline_staged(int(i))
        kf.synchronize()
        t = kf.kernel_timing()
        assert t["samples"] == 1, t
        ray.append(t["raycast"])
    kf.set_kernel_timing(0)
    last = kf.pose_record[-1]

    def scaled(W, H, s):  # the tests' off-centre intrinsics at scale s of the VGA focal lengths
        return Intrinsics(W, H, float(intr.fx * s), float(intr.fy * s * 1.02), W / 2 - 0.5 + 3.25, H / 2 - 0.5 - 1.5)

    views = {
        "tracked_pose_640x480": (I, last),
        "off_trajectory_640x480": (scaled(640, 480, 0.55), off_pose(last, -0.45, 0.35, -0.1)),
        "oblique_640x480": (scaled(640, 480, 0.3), off_pose(last, 0.4, -0.3, 0.15)),
        "tracked_pose_1280x720": (Intrinsics.from_any(synth.Intrinsics.hd720()), last),
    }
    rec = {}
    for name, (vi, vp) in views.items():
        rec[name] = {}
        for kind in KINDS:
            for maps in (False, True):
                img = kf.render_view(vi, vp, kind, maps=maps)  # warm-up (first use also allocates)
                ms = []
                for _ in range(REPS):
                    kf.render_view(vi, vp, kind, maps=maps)
                    ms.append(kf.view_ms())
                rec[name][kind + ("+maps" if maps else "")] = stats(ms)
        rec[name]["hit_fraction"] = float((img[3] != 0).mean())
    kf.close()
    y = stats(ray)
    v = rec["tracked_pose_640x480"]["phong"]
    commit = sys.argv[2] if len(sys.argv) > 2 else ""  # (a copy of the tree without its history: give it)
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                    text=True).stdout.strip()
        except OSError:
            pass
    out = {
        "workload": "C2 640x480, 512^3 @ 4 mm, %d frames of the bench sequence (ping-pong over 48)" % FRAMES,
        "unit": "ms, device time between HIP events around the launch",
        "commit_parent": commit,
        "libkfx_sha256": hashlib.sha256(open(kfx.LIB_PATH, "rb").read()).hexdigest(),
        "yardstick_raycast_stage": y,
        "yardstick_spread": y["max"] - y["min"],
        "views": rec,
        "expectation": "phong view at the tracked pose, no maps: median <= yardstick median + spread",
        "expectation_met": bool(v["median"] <= y["median"] + (y["max"] - y["min"])),
    }
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
