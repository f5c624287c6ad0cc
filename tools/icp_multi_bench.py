#!/usr/bin/env python3
"""Device time of the multi-start ICP on the bench's C2 workload
(640x480, 512^3 @ 4 mm, 20 frames of the bench's sequence), 5 repetitions after
a warm-up, min / median / max:
  - kfx_icp_multi at n = 1, 16, 256 starts of the tests' family
    (tests/multi_cases.py): kfx_get_icp_multi_ms' HIP-event span of the loop's
    launches, the chunk the rule gave at each level, and how many starts were lost
    (a lost start is stepped over from its failing solve on, so it costs less)
  - the yardstick: kfx_stage_icp from the same process on the same maps.  Both
    from ONE rocprofv3 kernel trace of the child (the same instrument): the
    persistent k_icp_track launch of kfx_stage_icp beside the k_icp_multi
    launches of a call, as the sum of their durations and as the span from the
    first start to the last end (the gaps between 19 launches are part of the
    call's cost)
  - the expectation: per-pose time at n = 256 (span / 256) below the single
    kfx_stage_icp time; the ratio is reported either way
  - kfx_track_view's view raycasts (three levels) beside kfx_score_view's, per
    level and summed, for the same camera
usage: python3 tools/icp_multi_bench.py out.json [parent commit]
(the measuring run is a child under `rocprofv3 --kernel-trace`, no counters;
with ICP_MULTI_BENCH_NOTRACE=1 it runs plainly and the trace figures are left out)"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

FRAMES, REPS = 20, 5
BATCH = (1, 16, 256)


def stats(xs):
    xs = sorted(float(x) for x in xs)
    return {"min": xs[0], "median": xs[len(xs) // 2], "max": xs[-1], "all": xs}


def child(out_path):
    import kfx
    import multi_cases as M
    from kfx import synth
    from kfx.abi import Intrinsics, default_params
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
    iters = sum(p.icp_iter_count[:p.pyramid_height])
    rec = {"plan": kf.debug_icp_plan(), "launches_per_call": iters, "batch": {}, "order": []}
    ev = {n: [] for n in BATCH}
    lost = {}
    for rep in range(REPS + 1):  # one launch order for the trace reader: stage_icp, then the three batches
        rc, _ = kf.stage_icp()
        assert rc == 0
        rec["order"].append(["stage_icp", rep])
        for n in BATCH:
            res = kf.icp_multi(M.starts(n))
            lost[n] = sum(r.status for r in res)
            rec["order"].append([n, rep])
            if rep:
                ev[n].append(kf.icp_multi_ms()["loop"])
    for n in BATCH:
        s = stats(ev[n])
        rec["batch"][str(n)] = {"chunk_per_level": [kfx.icp_multi_chunk(I.level(l).width, I.level(l).height, n)
                                                    for l in range(p.pyramid_height)],
                                "lost": lost[n], "events_ms": s, "events_ms_per_pose_median": s["median"] / n}
    tv, sv = [], {l: [] for l in range(p.pyramid_height)}
    for rep in range(REPS + 1):
        kf.track_view(last, M.starts(16))
        a = kf.icp_multi_ms()
        for l in range(p.pyramid_height):
            kf.score_view(l, last)
            if rep:
                sv[l].append(kf.quality_ms()["view"])
        if rep:
            tv.append(a)
    rec["track_view_16"] = {k: stats([a[k] for a in tv]) for k in ("view", "loop", "score")}
    rec["score_view_raycast_ms"] = {str(l): stats(v) for l, v in sv.items()}
    rec["score_view_raycast_ms_sum_of_medians"] = sum(stats(v)["median"] for v in sv.values())
    kf.close()
    rec["libkfx_sha256"] = hashlib.sha256(open(kfx.LIB_PATH, "rb").read()).hexdigest()
    with open(out_path, "w") as f:
        json.dump(rec, f)


def read_trace(d, order, per_call):
    """Per entry of the child's call order: us of kfx_stage_icp's ICP kernels (the last of them in the trace, one
    group per call) and of each kfx_icp_multi call's k_icp_multi launches (per_call of them, in order)."""
    paths = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    assert paths, "no kernel trace in " + d
    track, multi = [], []
    for path in paths:
        for r in csv.DictReader(open(path)):
            t = (int(r["Start_Timestamp"]), int(r["End_Timestamp"]))
            if "k_icp_multi" in r["Kernel_Name"]:
                multi.append(t)
            elif "k_icp_track" in r["Kernel_Name"]:
                track.append(t)
    track.sort()
    multi.sort()
    calls = [o for o in order if o[0] != "stage_icp"]
    singles = [o for o in order if o[0] == "stage_icp"]
    assert len(multi) >= per_call * len(calls), (len(multi), per_call, len(calls))
    if len(track) < len(singles):  # kfx_stage_icp launched per iteration: no single launch to read
        track = []
    multi = multi[:per_call * len(calls)]  # (kfx_track_view's launches follow)
    out = {"stage_icp": {"us": []}}
    for (s, e), (_, rep) in zip(track[-len(singles):] if track else [], singles):
        if rep:
            out["stage_icp"]["us"].append((e - s) / 1e3)
    for k, (n, rep) in enumerate(calls):
        if not rep:
            continue
        ks = multi[per_call * k:per_call * (k + 1)]
        o = out.setdefault(str(n), {"sum_us": [], "span_us": []})
        o["sum_us"].append(sum(e - s for s, e in ks) / 1e3)
        o["span_us"].append((ks[-1][1] - ks[0][0]) / 1e3)
    return {k: {m: stats(v) for m, v in d.items() if v} for k, d in out.items()}


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
        traced = not os.environ.get("ICP_MULTI_BENCH_NOTRACE")
        if traced:
            cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", os.path.join(tmp, "trace"), "-o", "run",
                   "--"] + cmd
        subprocess.run(cmd, check=True, timeout=420, cwd=tmp, stdout=subprocess.DEVNULL)
        rec = json.load(open(cj))
        trace = read_trace(os.path.join(tmp, "trace"), rec["order"], rec["launches_per_call"]) if traced else None
    del rec["order"]
    out = {
        "workload": "C2 640x480, 512^3 @ 4 mm, %d frames of the bench sequence (ping-pong over 48)" % FRAMES,
        "commit_parent": commit,
        "libkfx_sha256": rec.pop("libkfx_sha256"),
        "repetitions": "%d after one warm-up" % REPS,
        "kernel_trace_us": trace,
        "kernel_trace_note": "kfx_stage_icp's persistent k_icp_track launch (plan.launch 1 or 2; where the plan launches "
                             "per iteration the comparison is left out) and each kfx_icp_multi call's k_icp_multi "
                             "launches, same maps, one rocprofv3 --kernel-trace of one process",
    }
    if trace and trace["stage_icp"]:
        y, m = trace["stage_icp"]["us"], trace[str(BATCH[-1])]["span_us"]
        out["expectation"] = "n = 256: span / 256 below the single kfx_stage_icp launch (medians)"
        out["per_pose_us_at_256"] = m["median"] / BATCH[-1]
        out["stage_icp_us"] = y["median"]
        out["ratio_per_pose_over_single"] = (m["median"] / BATCH[-1]) / y["median"]
        out["expectation_met"] = bool(m["median"] / BATCH[-1] < y["median"])
    out.update(rec)
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
