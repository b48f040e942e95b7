"""ViT measurements: images/s and per-stage times of a named model at 224 x 224, the linear layers' share of the fp32 MFMA peak from
conv_stats, the non-convolution stages from op_stats, and the attention / LayerNorm / GELU kernels alone with achieved FLOP/s and bytes/s.  Medians
over --rounds rounds after --warmup forwards; the box calibration (bare MFMA and copy loops on this device) is printed next to the figures.  Where
torch sees the GPU, scaled_dot_product_attention in fp32 on the same shapes is timed as a same-box yardstick only.

    python tools/vit_bench.py [--model vit_b16] [--batches 1 8] [--rounds 20] [--warmup 5] [--out profiles/vit_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "instancesegmentation-jittor_amd")]


def op_stats(net):
    """{label: (us, bytes, launches)} accumulated since the last call (isegmi_engine_op_stats)."""
    from isegmi import _ffi
    cap = 64
    names = C.create_string_buffer(8192); us = (C.c_double * cap)(); by = (C.c_double * cap)(); ln = (C.c_int64 * cap)(); cnt = C.c_int()
    _ffi.check(_ffi.lib().isegmi_engine_op_stats(net._h, names, 8192, us, by, ln, cap, C.byref(cnt)))
    labels = names.value.decode().split("\n") if cnt.value else []
    return {labels[i]: (us[i], by[i], int(ln[i])) for i in range(cnt.value)}


def timed(fn, rounds, inner, sync):
    """median seconds per call of fn over `rounds` rounds of `inner` back-to-back calls, one sync per round"""
    fn(); sync()
    ts = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        sync()
        ts.append((time.perf_counter() - t0) / inner)
    return statistics.median(ts)


def bench_model(name, batch, rounds, warmup, calib):
    from isegmi.vit import ViT, ViTConfig
    from isegmi.weights import vit_random_state_dict
    cfg = ViTConfig.named(name)
    net = ViT(vit_random_state_dict(cfg, 1234), cfg, 224, 224, max_batch=batch)
    try:
        n = net.upload(np.random.default_rng(0).uniform(-1, 1, (batch, 224, 224, 3)).astype(np.float32))
        for _ in range(warmup):
            net.forward_device(n)
        net.sync()
        sec = timed(lambda: net.forward_device(n), rounds, 4, net.sync)
        out = {"model": name, "batch": batch, "forward_ms": sec * 1e3, "images_per_s": batch / sec}
        net.set_param("timing", 1.0)
        stages = {}
        for _ in range(rounds):
            net.forward_device(n); net.sync()
            for k, ms in net.timings():
                stages.setdefault(k, []).append(ms)
        net.set_param("timing", 0.0)
        out["stage_ms"] = {k: statistics.median(v) for k, v in stages.items()}
        net.set_param("conv_timing", 1.0); net.set_param("op_timing", 1.0)
        net.conv_stats(); op_stats(net)
        for _ in range(rounds):
            net.forward_device(n); net.sync()
        flops, ms, launches = net.conv_stats()
        ops = op_stats(net)
        net.set_param("conv_timing", 0.0); net.set_param("op_timing", 0.0)
        out["linear"] = {"gflop_per_forward": flops / rounds / 1e9, "ms_per_forward": ms / rounds, "launches_per_forward": launches // rounds,
                         "tflops": flops / ms / 1e9, "fraction_of_calibrated_fp32_mfma": flops / ms / 1e9 / calib["mfma_f32_tflops"]}
        out["other_ops"] = {k: {"us_per_forward": u / rounds, "gb_per_s": (b / u / 1e3) if u else 0.0, "launches_per_forward": l // rounds} for k, (u, b, l) in ops.items()}
        other_ms = sum(u for u, _, _ in ops.values()) / rounds / 1e3
        out["share_outside_linear_layers"] = other_ms / (other_ms + ms / rounds)
        return out
    finally:
        net.close()


def bench_ops(name, batch, rounds, calib):
    """the three new kernels alone on the model's shapes (device buffers, the null stream)"""
    from isegmi import _ffi
    from isegmi.vit import ViTConfig
    cfg = ViTConfig.named(name)
    T, D, M, heads = cfg.tokens(224, 224), cfg.dim, cfg.mlp_dim, cfg.heads
    rng = np.random.default_rng(1)
    L = _ffi.lib()
    qkv = _ffi.DeviceBuffer.from_numpy(rng.standard_normal((batch, T, 3 * D)).astype(np.float32)); att = _ffi.DeviceBuffer((batch, T, D))
    x = _ffi.DeviceBuffer.from_numpy(rng.standard_normal((batch * T, D)).astype(np.float32)); y = _ffi.DeviceBuffer((batch * T, D))
    ga = _ffi.DeviceBuffer.from_numpy(np.ones(D, np.float32)); be = _ffi.DeviceBuffer.from_numpy(np.zeros(D, np.float32))
    h = _ffi.DeviceBuffer.from_numpy(rng.standard_normal((batch * T, M)).astype(np.float32)); g = _ffi.DeviceBuffer((batch * T, M))
    res = {}
    s = timed(lambda: _ffi.check(L.isegmi_op_attention(qkv.ptr, batch, T, heads, att.ptr, None)), rounds, 20, _ffi.sync)
    fl = 4.0 * batch * heads * T * T * 64
    res["attention"] = {"us": s * 1e6, "tflops": fl / s / 1e12, "gb_per_s": 4.0 * batch * T * D * 4 / s / 1e9, "fraction_of_calibrated_fp32_mfma": fl / s / 1e12 / calib["mfma_f32_tflops"]}
    s = timed(lambda: _ffi.check(L.isegmi_op_layer_norm(x.ptr, batch * T, D, D, ga.ptr, be.ptr, 1e-6, y.ptr, D, None)), rounds, 20, _ffi.sync)
    res["layer_norm"] = {"us": s * 1e6, "gb_per_s": 2.0 * batch * T * D * 4 / s / 1e9, "fraction_of_calibrated_copy": 2.0 * batch * T * D * 4 / s / 1e9 / calib["hbm_copy_gbs"]}
    for tanh in (0, 1):
        s = timed(lambda: _ffi.check(L.isegmi_op_gelu(h.ptr, g.ptr, batch * T * M, tanh, None)), rounds, 20, _ffi.sync)
        res["gelu_tanh" if tanh else "gelu_erf"] = {"us": s * 1e6, "gb_per_s": 2.0 * batch * T * M * 4 / s / 1e9,
                                                     "fraction_of_calibrated_copy": 2.0 * batch * T * M * 4 / s / 1e9 / calib["hbm_copy_gbs"]}
    try:
        import torch
        if torch.cuda.is_available():
            q, k, v = (torch.randn(batch, heads, T, 64, device="cuda", dtype=torch.float32) for _ in range(3))
            s = timed(lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v), rounds, 20, torch.cuda.synchronize)
            res["torch_sdpa_fp32_yardstick"] = {"us": s * 1e6, "tflops": fl / s / 1e12}
    except Exception as ex:      # the yardstick is optional: say why it is missing
        res["torch_sdpa_fp32_yardstick"] = {"unavailable": repr(ex)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="vit_b16")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vit_bench.json"))
    a = ap.parse_args()
    from isegmi import _ffi
    _ffi.set_device(0)
    calib = _ffi.box_calibrate()
    report = {"box_calibration": calib, "runs": []}
    for b in a.batches:
        r = bench_model(a.model, b, a.rounds, a.warmup, calib)
        r["kernels_alone"] = bench_ops(a.model, b, a.rounds, calib)
        report["runs"].append(r)
        print(json.dumps(r))
    report["box_calibration_after"] = _ffi.box_calibrate()
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print("box calibration before / after:", calib, report["box_calibration_after"])


if __name__ == "__main__":
    main()
