#!/usr/bin/env python3
"""Device time of the ICP residual / quality calls on the
bench's C2 workload (640x480, 512^3 @ 4 mm, 20 frames of the bench's sequence),
5 repetitions after a warm-up, min / median / max:
  - per level, k_icp_acc (kfx_stage_icp_accumulate, the yardstick) beside
    k_quality without and with the per-pixel stores, all three taken from ONE
    rocprofv3 kernel trace of the same child process (the same instrument);
    the HIP-event figure of kfx_get_quality_ms beside them
  - kfx_score_poses: device ms per pose at n = 1, 16, 256 per level, and the
    chunk (poses per block) the rule gave
  - kfx_score_view's view raycast beside kfx_get_view_ms of kfx_render_view
    for the same camera and intrinsics
  - the level-0 fitness / rmse ladder at the tracked pose and displaced ones
usage: python3 tools/quality_bench.py out.json [parent commit]
(the measuring run is a child under `rocprofv3 --kernel-trace`; with
QUALITY_BENCH_NOTRACE=1 it runs plainly and the trace figures are left out)"""
import csv
import glob
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "slam-kinectfusion_amd"))

FRAMES, REPS = 20, 5
BATCH = (1, 16, 256)


def stats(xs):
    xs = sorted(float(x) for x in xs)
    return {"min": xs[0], "median": xs[len(xs) // 2], "max": xs[-1], "all": xs}


def rot(axis, ang):
    c, s = np.cos(ang), np.sin(ang)
    m = np.eye(4)
    i, j = {"x": (1, 2), "y": (2, 0)}[axis]
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def child(out_path):
    import kfx
    from kfx import synth
    from kfx.abi import Intrinsics, Pose, default_params
    intr = synth.Intrinsics.vga()
    I = Intrinsics.from_any(intr)
    p = default_params(dims=512, range_m=2.048)
    bgr, dep, _ = synth.sequence(48, intr, L=2.048, noise=True, traj_seed=7, dropout=0.005)
    kf = kfx.KinectFusion(I, p)
    kf.stage_frames(bgr, dep.astype(np.float32))
    for i in synth.ping_pong(48, FRAMES):
        kf.pipeline_staged(int(i))
    assert kf.synchronize() == 0
    last = kf.pose_record[-1]
    ident = Pose.identity()
    rec = {"levels": {}, "batch": {}, "launches": []}
    # one launch order for the trace reader: per level (1 + REPS) x [k_icp_acc, k_quality<false>, k_quality<true>]
    for l in range(p.pyramid_height):
        ev = {"stats_only": [], "with_stores": []}
        for rep in range(REPS + 1):
            kf.stage_icp_accumulate(l, ident)
            q = kf.stage_icp_residuals(l, ident, maps=False)
            a = kf.quality_ms()["residuals"]
            kf.stage_icp_residuals(l, ident, maps=True)
            b = kf.quality_ms()["residuals"]
            rec["launches"] += [[l, "k_icp_acc", rep], [l, "k_quality<false>", rep], [l, "k_quality<true>", rep]]
            if rep:
                ev["stats_only"].append(a)
                ev["with_stores"].append(b)
        g = I.level(l)
        rec["levels"][str(l)] = {"size": [g.width, g.height], "record": list(q.fields()),
                                 "events_ms": {k: stats(v) for k, v in ev.items()}}
    rng = np.random.default_rng(3)
    for l in range(p.pyramid_height):
        g = I.level(l)
        rec["batch"][str(l)] = {}
        for n in BATCH:
            poses = []
            for k in range(n):
                m = rot("y", 2e-3 * rng.standard_normal()) @ rot("x", 2e-3 * rng.standard_normal())
                m[:3, 3] = 2e-3 * rng.standard_normal(3)
                poses.append(m.astype(np.float32))
            ms = []
            for rep in range(REPS + 1):
                kf.score_poses(l, poses)
                if rep:
                    ms.append(kf.quality_ms()["residuals"])
            s = stats(ms)
            rec["batch"][str(l)][str(n)] = {"chunk": kfx.quality_chunk(g.width, g.height, n), "ms": s,
                                            "ms_per_pose_median": s["median"] / n}
    # the view raycast of score_view beside render_view's, same camera, per level
    rec["score_view"] = {}
    for l in range(p.pyramid_height):
        sv, rv = [], []
        for rep in range(REPS + 1):
            kf.score_view(l, last)
            a = kf.quality_ms()["view"]
            kf.render_view(I.level(l), last, "normal", maps=True)
            if rep:
                sv.append(a)
                rv.append(kf.view_ms())
        rec["score_view"][str(l)] = {"score_view_raycast_ms": stats(sv), "render_view_normal_maps_ms": stats(rv)}
    # what the figure says: level-0 fitness at the tracked pose and away from it
    ladder = {"tracked pose": np.eye(4), "1 cm sideways": None, "5 cm sideways": None, "2 deg turn": rot("y", np.deg2rad(2)),
              "5 deg turn": rot("y", np.deg2rad(5))}
    for name, d in (("1 cm sideways", 0.01), ("5 cm sideways", 0.05)):
        ladder[name] = np.eye(4)
        ladder[name][0, 3] = d
    rec["ladder_level0"] = {}
    for name, d in ladder.items():
        q = kf.score_view(0, (last.astype(np.float64) @ d).astype(np.float32))
        fit, rmse = kfx.quality_figures(q)
        rec["ladder_level0"][name] = {"n": list(q.n[:]), "fitness": fit, "rmse_m": rmse}
    q = kf.frame_quality(0)
    fit, rmse = kfx.quality_figures(q)
    rec["frame_quality_level0"] = {"n": list(q.n[:]), "fitness": fit, "rmse_m": rmse}
    kf.close()
    rec["libkfx_sha256"] = hashlib.sha256(open(kfx.LIB_PATH, "rb").read()).hexdigest()
    with open(out_path, "w") as f:
        json.dump(rec, f)


def read_trace(d, launches):
    """us per (level, kernel) of the level section's dispatches: k_icp_acc's last, k_quality's first (the section
    is the first user of k_quality and the last of k_icp_acc), matched to the child's launch list in order."""
    paths = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    assert paths, "no kernel trace in " + d
    rows = {"k_icp_acc": [], "k_quality<false>": [], "k_quality<true>": []}
    for path in paths:
        for r in csv.DictReader(open(path)):
            name = r["Kernel_Name"]
            if "k_icp_acc" in name:
                kind = "k_icp_acc"
            elif "k_quality<false>" in name or "k_qualityILb0E" in name:
                kind = "k_quality<false>"
            elif "k_quality" in name:
                kind = "k_quality<true>"
            else:
                continue
            rows[kind].append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    n = len(launches) // 3
    per = {}
    for kind, rs in rows.items():
        rs.sort()
        assert len(rs) >= n, (kind, len(rs), n)
        sect = rs[-n:] if kind == "k_icp_acc" else rs[:n]
        for (_, us), (l, _, rep) in zip(sect, [x for x in launches if x[1] == kind]):
            if rep:
                per.setdefault(str(l), {}).setdefault(kind, []).append(us)
    return {l: {k: stats(v) for k, v in d.items()} for l, d in per.items()}


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2])
    out_path = sys.argv[1]
    commit = sys.argv[2] if len(sys.argv) > 2 else ""
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                    text=True).stdout.strip()
        except OSError:
            pass
    with tempfile.TemporaryDirectory() as tmp:
        cj = os.path.join(tmp, "child.json")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", cj]
        traced = not os.environ.get("QUALITY_BENCH_NOTRACE")
        if traced:
            cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", os.path.join(tmp, "trace"), "-o", "run",
                   "--"] + cmd
        subprocess.run(cmd, check=True, timeout=420, cwd=tmp, stdout=subprocess.DEVNULL)
        rec = json.load(open(cj))
        trace = read_trace(os.path.join(tmp, "trace"), rec["launches"]) if traced else None
    del rec["launches"]
    out = {
        "workload": "C2 640x480, 512^3 @ 4 mm, %d frames of the bench sequence (ping-pong over 48)" % FRAMES,
        "commit_parent": commit,
        "libkfx_sha256": rec.pop("libkfx_sha256"),
        "repetitions": "%d after one warm-up" % REPS,
        "kernel_trace_us": trace,
        "kernel_trace_note": "k_icp_acc (kfx_stage_icp_accumulate) and both k_quality instantiations, identity pose, "
                             "same maps, one rocprofv3 --kernel-trace of one process",
    }
    if trace:
        y, s, w = (trace["0"][k] for k in ("k_icp_acc", "k_quality<false>", "k_quality<true>"))
        out["yardstick_spread_us_level0"] = y["max"] - y["min"]
        out["expectation"] = "level 0, stats only: median <= k_icp_acc median + k_icp_acc (max - min)"
        out["expectation_met"] = bool(s["median"] <= y["median"] + (y["max"] - y["min"]))
        out["stores_cost_us_level0_median"] = w["median"] - s["median"]
    out.update(rec)
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
