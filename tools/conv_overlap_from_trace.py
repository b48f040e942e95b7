"""How much of a pipelined run has only ONE convolution kernel resident?  (dev tool; profiles/step_overlap.md)

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python bench.py --gpus 1 --steps 20 --warmup 5
    python tools/conv_overlap_from_trace.py DIR [--tail 0.5]

Reads every *kernel_trace.csv under DIR, keeps the kernels of the densest part of the run -- the last `--tail` fraction of the span between the
first and the last convolution kernel, i.e. the timed steps, not the set-up -- and sweeps their [start, end) intervals: the share of wall time with
0, 1, and 2 or more convolution kernels (names containing "conv") resident, and the same with any kernel counted.  A kernel trace only: no counters."""
import argparse
import csv
import glob
import os
import sys


def load(d):
    rows = []
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r.get("Kernel_Name") or r.get("kernel_name") or ""
                s = r.get("Start_Timestamp") or r.get("start_timestamp")
                e = r.get("End_Timestamp") or r.get("end_timestamp")
                if s and e:
                    rows.append((int(s), int(e), name))
    return rows


def shares(intervals, t0, t1):
    """-> {resident count (capped at 2): share of [t0, t1)}"""
    ev = []
    for s, e in intervals:
        s, e = max(s, t0), min(e, t1)
        if e > s:
            ev.append((s, 1)); ev.append((e, -1))
    ev.sort()
    acc = {0: 0, 1: 0, 2: 0}
    depth, last = 0, t0
    for t, d in ev:
        acc[min(depth, 2)] += t - last
        depth += d
        last = t
    acc[min(depth, 2)] += t1 - last
    span = float(t1 - t0) or 1.0
    return {k: v / span for k, v in acc.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--tail", type=float, default=0.5)
    a = ap.parse_args()
    rows = load(a.dir)
    conv = [(s, e) for s, e, n in rows if "conv" in n]
    if not conv:
        sys.exit("no convolution kernels in " + a.dir)
    first, last = min(s for s, _ in conv), max(e for _, e in conv)
    t0 = last - int((last - first) * a.tail)
    c = shares(conv, t0, last)
    k = shares([(s, e) for s, e, _ in rows], t0, last)
    n = sum(1 for s, e in conv if s >= t0)
    print("window %.2f ms, %d conv launches" % ((last - t0) / 1e6, n))
    print("conv kernels resident:  none %.3f   exactly one %.3f   two or more %.3f" % (c[0], c[1], c[2]))
    print("any kernel resident:    none %.3f   exactly one %.3f   two or more %.3f" % (k[0], k[1], k[2]))


if __name__ == "__main__":
    main()
