#!/usr/bin/env python3
"""Device time of the fern keyframes on the bench's C2 workload
(640x480, 512^3 @ 4 mm, 20 frames of the bench's sequence), 5 repetitions after
a warm-up, min / median / max.  Nothing here is a pass or fail threshold; each
figure stands beside its yardstick.
  - encode: kfx_get_keyframe_ms' HIP-event span of k_fern_encode at m = 512
  - search at N = 1024 and 65536 random keyframes, q = 1 and 256, k = 4,
    m = 512: the event span, and from ONE rocprofv3 kernel trace of the child
    the durations of k_fern_search and k_fern_merge per call.
    Yardstick for q = 1: the time to read the code table once (N * 256 bytes)
    at the copy rate profiles/shift_bench.json records.
    Yardstick for q = 256: the per-query time against the q = 1 time.
  - kfx_pipeline_recover beside kfx_pipeline, host ms per frame over the same
    20 frames from host memory (the price of probing before committing)
usage: python3 tools/reloc_bench.py out.json [parent commit]
(the measuring run is a child under `rocprofv3 --kernel-trace`, no counters;
with RELOC_BENCH_NOTRACE=1 it runs plainly and the trace figures are left out)"""
import csv
import glob
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

FRAMES, REPS = 20, 5
SIZES, BATCH, K, M_FERNS = (1024, 65536), (1, 256), 4, 512


def stats(xs):
    xs = sorted(float(x) for x in xs)
    return {"min": xs[0], "median": xs[len(xs) // 2], "max": xs[-1], "all": xs}


def child(out_path):
    import kfx
    from kfx import synth
    from kfx.abi import Intrinsics, Pose, default_params
    intr = synth.Intrinsics.vga()
    I = Intrinsics.from_any(intr)
    p = default_params(dims=512, range_m=2.048)
    bgr, dep, _ = synth.sequence(48, intr, L=2.048, noise=True, traj_seed=7, dropout=0.005)
    dep = dep.astype(np.float32)
    order = synth.ping_pong(48, FRAMES)
    kf = kfx.KinectFusion(I, p)
    t0 = time.perf_counter()
    for i in order:
        assert kf.pipeline(bgr[int(i)], dep[int(i)]) == 0
    plain_ms = 1e3 * (time.perf_counter() - t0) / FRAMES
    rec = {"order": [], "search": {}}
    st = kfx.Keyframes(kf, m=M_FERNS)
    enc = []
    for rep in range(REPS + 1):
        st.encode()
        if rep:
            enc.append(1e3 * kf.keyframe_ms()["encode"])
    rec["encode_us"] = stats(enc)
    rng = np.random.default_rng(7)
    eye = Pose.identity()
    for N in SIZES:
        codes = rng.integers(0, 1 << 63, (N, M_FERNS // 16), dtype=np.uint64)
        while len(st) < N:
            st.put(eye, codes[len(st)])
        for q in BATCH:
            queries = rng.integers(0, 1 << 63, (q, M_FERNS // 16), dtype=np.uint64)
            ev = []
            for rep in range(REPS + 1):
                st.search(queries, K)
                rec["order"].append([N, q, rep])
                if rep:
                    ev.append(1e3 * kf.keyframe_ms()["search"])
            rec["search"]["N%d_q%d" % (N, q)] = {"chunk": kfx.keyframes_search_chunk(N, q), "events_us": stats(ev)}
    st.close()
    kf.close()
    kf = kfx.KinectFusion(I, p)
    st = kfx.Keyframes(kf, m=M_FERNS)
    events = []
    t0 = time.perf_counter()
    for i in order:
        rc, rep = kf.pipeline_recover(st, bgr[int(i)], dep[int(i)])
        assert rc == 0
        events.append(rep.event)
    rec["recover"] = {"pipeline_ms_per_frame": plain_ms, "pipeline_recover_ms_per_frame": 1e3 * (time.perf_counter() - t0) / FRAMES,
                      "events": events, "keyframes": len(st),
                      "note": "host wall time per frame from host memory, first frames and graph capture included"}
    st.close()
    kf.close()
    rec["libkfx_sha256"] = hashlib.sha256(open(kfx.LIB_PATH, "rb").read()).hexdigest()
    with open(out_path, "w") as f:
        json.dump(rec, f)


def read_trace(d, order):
    """us of k_fern_search and k_fern_merge per search call of the child's order (one launch of each per call)."""
    paths = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    assert paths, "no kernel trace in " + d
    search, merge = [], []
    for path in paths:
        for r in csv.DictReader(open(path)):
            t = (int(r["Start_Timestamp"]), int(r["End_Timestamp"]))
            if "k_fern_search" in r["Kernel_Name"]:
                search.append(t)
            elif "k_fern_merge" in r["Kernel_Name"]:
                merge.append(t)
    search.sort()
    merge.sort()
    assert len(search) >= len(order) and len(merge) >= len(order), (len(search), len(merge), len(order))
    out = {}
    for (N, q, rep), s, m in zip(order, search, merge):
        if rep:
            o = out.setdefault("N%d_q%d" % (N, q), {"search_us": [], "merge_us": []})
            o["search_us"].append((s[1] - s[0]) / 1e3)
            o["merge_us"].append((m[1] - m[0]) / 1e3)
    return {k: {n: stats(v) for n, v in d.items()} for k, d in out.items()}


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
        traced = not os.environ.get("RELOC_BENCH_NOTRACE")
        if traced:
            cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", os.path.join(tmp, "trace"), "-o", "run",
                   "--"] + cmd
        subprocess.run(cmd, check=True, timeout=420, cwd=tmp, stdout=subprocess.DEVNULL)
        rec = json.load(open(cj))
        trace = read_trace(os.path.join(tmp, "trace"), rec["order"]) if traced else None
    del rec["order"]
    rate = json.load(open(os.path.join(ROOT, "profiles", "shift_bench.json")))["copy_rate_TBps"]
    for N in SIZES:
        one, many = rec["search"]["N%d_q1" % N], rec["search"]["N%d_q%d" % (N, BATCH[-1])]
        if trace:
            for key, o in ((1, one), (BATCH[-1], many)):
                o["kernel_trace_us"] = trace["N%d_q%d" % (N, key)]
        t1 = (one["kernel_trace_us"]["search_us"] if trace else one["events_us"])["median"]
        tq = (many["kernel_trace_us"]["search_us"] if trace else many["events_us"])["median"]
        one["table_bytes"] = N * (M_FERNS // 16) * 8
        one["yardstick_table_read_us_at_copy_rate"] = one["table_bytes"] / (rate * 1e12) * 1e6
        one["search_us_over_yardstick"] = t1 / one["yardstick_table_read_us_at_copy_rate"]
        many["per_query_us"] = tq / BATCH[-1]
        many["yardstick_q1_us"] = t1
        many["per_query_over_q1"] = (tq / BATCH[-1]) / t1
    out = {
        "workload": "C2 640x480, 512^3 @ 4 mm, %d frames of the bench sequence (ping-pong over 48); random codes, "
                    "m = %d, k = %d" % (FRAMES, M_FERNS, K),
        "commit_parent": commit,
        "libkfx_sha256": rec.pop("libkfx_sha256"),
        "repetitions": "%d after one warm-up" % REPS,
        "copy_rate_TBps": rate,
        "kernel_trace": "one rocprofv3 --kernel-trace of one process, no counters" if trace else None,
    }
    out.update(rec)
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
