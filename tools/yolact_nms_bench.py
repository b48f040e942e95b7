"""Yolact Detect in its three suppression modes: 0 fast NMS, 1 cross-class fast NMS, 2 traditional per-class NMS.

  op      isegmi_op_yolact_detect alone on synthetic head outputs at P = 19 248 with a CONTROLLED number of candidates per class
          (about 10 / 100 / 1000 over a few / half / all of the 80 classes), N = 1 and 8, the three modes on the same inputs in one process.
  engine  the whole Yolact forward at 550 x 550, random weights, bs = 1 and 8, in the three modes.  Random weights at this size fill every image's 100 slots (about
          2100 survivors of the per-class greedy pass, `nms_total` in the record); the synthetic rows are the ones that control the crowding.

  ab      (--ab-tree DIR) the same box, alternating fresh processes of this tree and of another, built checkout of the project -- the parent commit's:
          Detect in mode 0 and the bench.py headline, each side with ITS OWN Python package and library (a library of another commit need not export
          what this commit's isegmi/_abi.py declares, so swapping the library alone under ISEGMI_LIB, as tools/ab_lib.sh does for two builds of one
          tree, does not carry across an ABI addition).  Each side's runs and their spread go into the record.  The other tree:
              git worktree add /tmp/isegmi_parent HEAD~1 && make -C /tmp/isegmi_parent/instancesegmentation-jittor_amd -j16 -s
              python tools/yolact_nms_bench.py --skip-op --skip-engine --ab-tree /tmp/isegmi_parent --out profiles/yolact_nms_bench.json

Every figure is the median of `--reps` timed windows of `--iters` back-to-back calls (tens of milliseconds per window) after `--warmup` calls, with
the windows' min and max next to it; the three modes' windows alternate, so a drift of the box falls on all of them.
    python tools/yolact_nms_bench.py [--out profiles/yolact_nms_bench.json] [--skip-op] [--skip-engine] [--ab-tree DIR]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_ROOT = os.environ.get("ISEGMI_BENCH_TREE", ROOT)   # (set by --ab-tree for the other side's child processes)
sys.path[:0] = [PKG_ROOT, os.path.join(PKG_ROOT, "instancesegmentation-jittor_amd")]
import numpy as np  # noqa: E402

P_FULL = 19248
NCLS = 81


def synthetic_heads(rng, N, per_class, classes):
    """conf logits with `per_class` priors of each of the first `classes` foreground classes far above the threshold (distinct scores), everything else
    far below; clustered priors so that the suppression has work to do"""
    conf = np.full((N, P_FULL, NCLS), -9.0, np.float32)
    conf[..., 0] = 0.0
    for n in range(N):
        pick = rng.permutation(P_FULL)[:per_class * classes].reshape(classes, per_class)
        for c in range(classes):
            conf[n, pick[c], 1 + c] = rng.uniform(0.0, 6.0, per_class).astype(np.float32)
    ctr = rng.uniform(0.1, 0.9, (64, 2))[rng.integers(0, 64, P_FULL)] + rng.uniform(-0.05, 0.05, (P_FULL, 2))
    priors = np.concatenate([ctr, rng.uniform(0.05, 0.3, (P_FULL, 2))], 1).astype(np.float32)
    loc = (rng.standard_normal((N, P_FULL, 4)) * 0.2).astype(np.float32)
    mask = np.tanh(rng.standard_normal((N, P_FULL, 32))).astype(np.float32)
    return conf, loc, mask, priors


def timed_alternating(runs, sync, warmup, iters, reps):
    """runs: {name: callable}.  One window of every name per repetition, in turn -> {name: dict(median_us, min_us, max_us)}"""
    for run in runs.values():
        for _ in range(warmup):
            run()
    sync()
    us = {k: [] for k in runs}
    for _ in range(reps):
        for k, run in runs.items():
            t0 = time.perf_counter()
            for _ in range(iters):
                run()
            sync()
            us[k].append((time.perf_counter() - t0) / iters * 1e6)
    out = {}
    for k, v in us.items():
        v.sort()
        out[k] = dict(median_us=round(v[len(v) // 2], 1), min_us=round(v[0], 1), max_us=round(v[-1], 1))
    return out


OP_CASES = ((10, 4), (10, 40), (10, 80), (100, 4), (100, 40), (100, 80), (1000, 4), (1000, 19))


def bench_op(args, cases=OP_CASES, modes=(0, 1, 2)):
    from isegmi import _ffi
    rows = []
    rng = np.random.default_rng(0)
    fn = _ffi.lib().isegmi_op_yolact_detect
    for N in (1, 8):
        for per_class, classes in cases:
            conf, loc, mask, priors = synthetic_heads(rng, N, per_class, classes)
            row = dict(N=N, per_class=per_class, classes=classes)
            # mode 0 with nothing but the fields that existed before the modes (what another build of the library understands as well)
            prep = {m: _ffi.yolact_detect_prepare(conf, loc, mask, priors, nms_mode=m, return_nms=m != 0) for m in modes}
            runs = {m: (lambda a=prep[m][0]: _ffi.check(fn(C.byref(a), None))) for m in modes}
            res = timed_alternating(runs, _ffi.sync, args.warmup, args.iters, args.reps)
            for m in modes:
                if m:
                    res[m]["nms_total"] = prep[m][1]["d_out_nms_total"].numpy().tolist()
                    res[m]["overflow"] = prep[m][1]["d_out_nms_overflow"].numpy().tolist()
                row["mode%d" % m] = res[m]
            del prep, runs
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def bench_engine(args):
    import dataclasses
    from isegmi.weights import yolact_state_dict
    from isegmi.yolact import Yolact, YolactConfig, fast_base_transform
    sd = yolact_state_dict(1234)
    rows = []
    rng = np.random.default_rng(1)
    for bs in (1, 8):
        x = fast_base_transform(rng.uniform(0, 255, (bs, 550, 550, 3)).astype(np.float32))
        row = dict(bs=bs)
        nets = {}
        for mode in (0, 1, 2):
            cfg = dataclasses.replace(YolactConfig(), use_fast_nms=mode != 2, use_cross_class_nms=mode == 1)
            nets[mode] = Yolact(sd, cfg, max_batch=bs)
            nets[mode].upload(x)
        runs = {m: (lambda net=nets[m]: net.forward_device(bs)) for m in nets}

        def sync():
            for net in nets.values():
                net.sync()
        res = timed_alternating(runs, sync, args.warmup, max(args.iters // 8, 10), args.reps)
        for m, net in nets.items():
            res[m]["detections"] = net.fetch("det.count", bs).tolist()
            if m:
                res[m]["nms_total"] = net.fetch("det.nms_total", bs).tolist()
            row["mode%d" % m] = res[m]
            net.close()
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


AB_CASES = ((10, 4), (100, 40))


def _spread(vals):
    return round((max(vals) - min(vals)) / (sum(vals) / len(vals)) * 100.0, 2)


def bench_mode0_portable(args):
    """Detect in the default mode on the A/B cases through nothing but what every commit's package has (DeviceBuffer, the argument struct's
    original fields, isegmi_op_yolact_detect): runs unchanged against the other tree's package and library"""
    from isegmi import _ffi
    from isegmi._abi import YolactDetectArgs
    rows = []
    rng = np.random.default_rng(0)
    fn = _ffi.lib().isegmi_op_yolact_detect
    top_k, max_det, nc = 200, 100, NCLS - 1
    for N in (1, 8):
        for per_class, classes in AB_CASES:
            conf, loc, mask, priors = synthetic_heads(rng, N, per_class, classes)
            D = _ffi.DeviceBuffer
            bufs = dict(d_conf=D.from_numpy(conf), d_loc=D.from_numpy(loc), d_mask=D.from_numpy(mask), d_priors=D.from_numpy(priors),
                        d_ws_scoresT=D((N, nc, P_FULL)), d_ws_boxes=D((N, P_FULL, 4)), d_ws_counts=D((2 * N,), np.int32),
                        d_ws_tk_vals=D((N, nc, top_k)), d_ws_tk_idx=D((N, nc, top_k), np.int32), d_ws_tk_cnt=D((N, nc), np.int32),
                        d_ws_cand=D((N, nc, top_k)), d_ws_fin_vals=D((N, max_det)), d_ws_fin_idx=D((N, max_det), np.int32),
                        d_ws_fin_cnt=D((N,), np.int32), d_out_count=D((N,), np.int32), d_out_boxes=D((N, max_det, 4)), d_out_scores=D((N, max_det)),
                        d_out_classes=D((N, max_det), np.int32), d_out_coeffs=D((N, max_det, 32)), d_out_prior=D((N, max_det), np.int32))
            a = YolactDetectArgs()
            a.N, a.P, a.ncls, a.mask_dim, a.top_k, a.max_det, a.conf_thresh, a.nms_thresh = N, P_FULL, NCLS, 32, top_k, max_det, 0.05, 0.5
            for name, buf in bufs.items():
                setattr(a, name, buf.ptr)
            res = timed_alternating({0: lambda: _ffi.check(fn(C.byref(a), None))}, _ffi.sync, args.warmup, args.iters, args.reps)
            rows.append(dict(N=N, per_class=per_class, classes=classes, mode0=res[0], detections=bufs["d_out_count"].numpy().tolist()))
            del a, bufs
    return rows


def bench_ab(args):
    """alternating fresh processes: OTHER, THIS, OTHER, THIS, ... for Detect mode 0 (this tool's --child-mode0) and for the bench.py headline"""
    import subprocess
    here = os.path.abspath(__file__)
    tree = os.path.abspath(args.ab_tree)
    base = {k: v for k, v in os.environ.items() if k not in ("ISEGMI_LIB", "ISEGMI_BENCH_TREE")}
    sides = (("other", dict(base, ISEGMI_BENCH_TREE=tree), tree), ("this", base, ROOT))
    detect = dict(other=[], this=[])
    headline = dict(other=[], this=[])
    child = [sys.executable, here, "--child-mode0", "--warmup", str(args.warmup), "--iters", str(args.iters), "--reps", str(args.reps)]
    flags = ["--gpus", "1", "--steps", "30", "--warmup", "5", "--no-cpu-baseline", "--no-latency", "--no-maskrcnn", "--no-r101f16", "--no-box", "--no-h2d",
             "--no-e2e"]
    for _ in range(args.ab_reps):
        for side, env, root in sides:
            r = subprocess.run(child, env=env, capture_output=True, text=True, timeout=200)
            if r.returncode:
                raise RuntimeError("%s side, Detect child: %s" % (side, r.stderr[-2000:]))
            detect[side].append(json.loads(r.stdout.strip().splitlines()[-1]))
            r = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + flags, env=env, capture_output=True, text=True, timeout=200, cwd=root)
            if r.returncode:
                raise RuntimeError("%s side, bench.py: %s" % (side, r.stderr[-2000:]))
            headline[side].append(json.loads(r.stdout.strip().splitlines()[-1])["value"])
    for rows in zip(*(detect["other"] + detect["this"])):   # both sides computed the same thing
        assert len({json.dumps(r["detections"]) for r in rows}) == 1, "the two sides' Detect results differ"
    res = dict(other_tree="the parent commit, built", runs_per_side=args.ab_reps,
               headline_img_s=dict(headline, spread_pct={k: _spread(v) for k, v in headline.items()}), detect_mode0_us=[])
    for i, row in enumerate(detect["this"][0]):
        key = dict(N=row["N"], per_class=row["per_class"], classes=row["classes"])
        runs = {s: [r[i]["mode0"]["median_us"] for r in detect[s]] for s in ("other", "this")}
        res["detect_mode0_us"].append(dict(key, **runs, spread_pct={k: _spread(v) for k, v in runs.items()}))
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-engine", action="store_true")
    ap.add_argument("--skip-op", action="store_true")
    ap.add_argument("--ab-tree", default=None, help="another built checkout of the project (the parent commit's) for the same-box A/B")
    ap.add_argument("--ab-reps", type=int, default=3)
    ap.add_argument("--child-mode0", action="store_true", help="(used by --ab-tree) Detect mode 0 on the A/B cases with the package and library of ISEGMI_BENCH_TREE")
    ap.add_argument("--trace-case", type=int, default=None, metavar="MODE", help="200 Detect calls of MODE at N = 8, 10 x 4 and nothing else (for a kernel trace)")
    args = ap.parse_args()
    from isegmi import _ffi
    _ffi.set_device(0)
    if args.child_mode0:
        print(json.dumps(bench_mode0_portable(args)))
        return
    if args.trace_case is not None:
        conf, loc, mask, priors = synthetic_heads(np.random.default_rng(0), 8, 10, 4)
        a, bufs = _ffi.yolact_detect_prepare(conf, loc, mask, priors, nms_mode=args.trace_case, return_nms=args.trace_case != 0)
        for _ in range(200):
            _ffi.check(_ffi.lib().isegmi_op_yolact_detect(C.byref(a), None))
        _ffi.sync()
        return
    res = dict(tool="tools/yolact_nms_bench.py", P=P_FULL, ncls=NCLS, warmup=args.warmup, iters=args.iters, reps=args.reps)
    if args.out and os.path.exists(args.out):   # a partial run (--skip-*) keeps the other sections of an existing record
        res = dict(json.load(open(args.out)), **res)
    if not args.skip_op:
        res["op"] = bench_op(args)
    if not args.skip_engine:
        res["engine_550"] = bench_engine(args)
    if args.ab_tree:
        res["ab_parent"] = bench_ab(args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
