#!/usr/bin/env python3
"""Rows of an alternated A/B of tools/view_bench.py and tools/world_view_bench.py:
DIR holds <tool>_<lib>_<round>.json as the tools write them, lib = parent or LIB.
Per row: each run's median ms (parent | LIB), then the parent's median over its
runs, its spread (max - min), LIB's median, and whether LIB's median is within
parent median + parent spread.
usage: tools/view_ab_rows.py DIR LIB [view_bench] [world_view_bench]"""
import glob
import json
import sys

D = sys.argv[1]
LIB = sys.argv[2]
ONLY = sys.argv[3:] or ["view_bench", "world_view_bench"]


def rows(tool, d):
    out = {}
    if tool == "view_bench":
        for name, rec in d["views"].items():
            for k, v in rec.items():
                if isinstance(v, dict):
                    out[f"render_view {name} {k}"] = v["median"]
    else:
        for name, rec in d["window_box"]["views"].items():
            for k, v in rec.items():
                if isinstance(v, dict):
                    out[f"window_box {name} {k} world_view"] = v["world_view"]["median"]
                    out[f"window_box {name} {k} render_view"] = v["render_view"]["median"]
        for k, v in d["window_plus_store"]["tracked_pose_640x480"].items():
            if isinstance(v, dict):
                out[f"window_plus_store tracked_pose_640x480 {k} world_view"] = v["world_view"]["median"]
                out[f"window_plus_store tracked_pose_640x480 {k} render_view"] = v["render_view_window_only"]["median"]
    return out


bad = 0
sha = {}
for tool in ONLY:
    data = {}
    for lib in ("parent", LIB):
        runs = []
        for p in sorted(glob.glob(f"{D}/{tool}_{lib}_*.json")):
            d = json.load(open(p))
            sha[lib] = d["libkfx_sha256"]
            runs.append(rows(tool, d))
        data[lib] = runs
    print(f"# tools/{tool}.py: median ms of each run (5 repetitions), parent | tree; then parent median, parent spread, tree median, verdict")
    for row in data["parent"][0]:
        p = [r[row] for r in data["parent"]]
        t = [r[row] for r in data[LIB]]
        pm, tm = sorted(p)[len(p) // 2], sorted(t)[len(t) // 2]
        sp = max(p) - min(p)
        ok = tm <= pm + sp
        bad += not ok
        print(f"{row}: {' '.join('%.4f' % x for x in p)} | {' '.join('%.4f' % x for x in t)} ; "
              f"{pm:.4f} {sp:.4f} {tm:.4f} {'ok' if ok else 'OVER'} ({100 * (tm / pm - 1):+.2f} %)")
print("# libkfx.so sha256:", ", ".join(f"{k} {v}" for k, v in sha.items()))
print("# rows over the bound:", bad)
