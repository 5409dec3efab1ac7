#!/usr/bin/env python3
"""The table of measured.txt from a directory of alternating timing rounds: <script>_<side>_<round>.json (the measure scripts' and
host_calls.py's result lines) and optim_<side>_<round>.txt (optim_bench.py's output), side = parent or change.  Per figure (every
median_us / median_ms of the project's own code and optim_bench's two SparseAdam lines): the parent's round medians, their median
and spread (largest minus smallest), the change's round medians and their median, and whether the change's median stays within the
parent's median plus the parent's spread.  Then every run's raw line.

    python profiles/map_steps/table.py DIR > measured.txt
"""
import glob
import json
import os
import re
import statistics
import sys


def figures(path):
    """{figure name: value} of one result file"""
    text = open(path).read()
    if path.endswith(".txt"):
        return {"optim_bench: " + " ".join(m.group(1).split()): float(m.group(2)) * 1e3
                for m in re.finditer(r"^(dgr SparseAdam.*?)\s+([\d.]+) ms/step", text, re.M)}
    out = {}

    def walk(node, where):
        for k, v in node.items() if isinstance(node, dict) else ():
            if k in ("median_us", "median_ms") and "torch" not in where:
                out[where] = v * (1e3 if k == "median_ms" else 1.0)
            else:
                walk(v, f"{where}/{k}" if where else k)
    walk(json.loads(text), "")
    return out


def main():
    d = sys.argv[1]
    runs = {}  # script -> side -> round -> {figure: us}
    for f in sorted(glob.glob(os.path.join(d, "*_*_*.json")) + glob.glob(os.path.join(d, "optim_*_*.txt"))):
        m = re.match(r"(\w+?)_(parent|change)_(\d+)\.", os.path.basename(f))
        runs.setdefault(m.group(1), {}).setdefault(m.group(2), {})[int(m.group(3))] = figures(f)
    print("microseconds; p = parent, c = change; spread = the largest minus the smallest of the parent's round medians")
    for script, sides in sorted(runs.items()):
        ok = True
        print(f"\n== {script}: rounds {sorted(sides['parent'])}")
        for fig in next(iter(sides["parent"].values())):
            p = [sides["parent"][r][fig] for r in sorted(sides["parent"])]
            c = [sides["change"][r][fig] for r in sorted(sides["change"])]
            mp, mc, spread = statistics.median(p), statistics.median(c), max(p) - min(p)
            ok &= mc <= mp + spread
            fmt = lambda xs: " ".join(f"{x:.1f}" for x in xs)  # noqa: E731
            print(f"  {fig}\n      p [{fmt(p)}] median {mp:.2f} spread {spread:.2f} | c [{fmt(c)}] median {mc:.2f}"
                  f" | {'within' if mc <= mp + spread else 'ABOVE'} ({mc - mp:+.2f})")
        print(f"  -> {script}: {'every figure within the bar' if ok else 'a figure ABOVE the bar'}")
    print("\n== every run")
    for f in sorted(glob.glob(os.path.join(d, "*_*_*.json")) + glob.glob(os.path.join(d, "optim_*_*.txt"))):
        print(f"-- {os.path.basename(f)}\n{' '.join(open(f).read().split())}")


if __name__ == "__main__":
    main()
