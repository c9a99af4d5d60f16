"""Timing probe for the upsampling ops (profiles/upsampling.md).

1. Bare kernels: K_RESIZE nearest and bilinear on
   [8,56,56,64] -> [8,112,112,64], against the K_POOL kernel (2x2/s2 max
   on [8,112,112,64] -> [8,56,56,64]) which moves the same number of
   bytes with the same one-thread-per-8-channels design. Achieved GB/s
   is (input bytes + output bytes) / time.
2. Transposed conv [8,28,28,64] -> [8,56,56,64]: 2x2/s2 through the
   gemm+transpose lowering, the same through zero-insert+conv (forced),
   and 3x3/s2 SAME (zero-insert+conv). Whole-plan hipGraph replay.
3. build_unet(image_size=64), all three variants, batch 1 and 16: warm
   wall latency of GpuModel-backed predict (host staging + H2D + graph
   replay + D2H).

Kernel and plan figures are the wall time of N back-to-back replays
ending in one device synchronise, divided by N; cases that are compared
alternate, and the spread over the rounds is printed with the median.

    python scripts/upsampling_probe.py [--replays 200] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tfservingcache_amd.engine import _tfsc_engine as ext  # noqa: E402
from tfservingcache_amd.engine import planner  # noqa: E402
from tfservingcache_amd.engine.gpu import GpuModel  # noqa: E402
from tfservingcache_amd.engine.model import load_model_from_dir  # noqa: E402
from tfservingcache_amd.engine.savedmodel import (GraphBuilder,  # noqa: E402
                                                  write_saved_model)
from tfservingcache_amd.models import build_unet  # noqa: E402

DEV = "cuda:0"


def _time_replays(replay, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6      # us per replay


def _summary(samples):
    return {"median_us": round(statistics.median(samples), 2),
            "min_us": round(min(samples), 2),
            "max_us": round(max(samples), 2),
            "rounds": len(samples)}


def kernel_cases(replays, rounds):
    N, H, W, C = 8, 56, 56, 64
    small = (torch.randn(N, H, W, C, device=DEV)).to(torch.bfloat16)
    big = (torch.randn(N, 2 * H, 2 * W, C, device=DEV)).to(torch.bfloat16)
    out_big = torch.empty_like(big)
    out_small = torch.empty_like(small)
    nbytes = (small.numel() + big.numel()) * 2
    up = [small.data_ptr(), out_big.data_ptr()]
    plans = {
        "pool_max_2x2s2": ext.ExecPlan([(
            ext.K_POOL, [big.data_ptr(), out_small.data_ptr()],
            [1, N, 2 * H, 2 * W, C, H, W, 2, 2, 2, 2, 0, 0], [])]),
        "resize_nearest": ext.ExecPlan([(
            ext.K_RESIZE, up, [N, H, W, C, 2 * H, 2 * W, 0, 0, 1], [])]),
        "resize_bilinear": ext.ExecPlan([(
            ext.K_RESIZE, up, [N, H, W, C, 2 * H, 2 * W, 1, 0, 1], [])]),
    }
    stream = torch.cuda.Stream(device=DEV)
    samples = {n: [] for n in plans}
    with torch.cuda.stream(stream):
        for p in plans.values():
            p.run()
            stream.synchronize()
            p.capture()
        for _ in range(rounds):
            for n, p in plans.items():
                samples[n].append(_time_replays(p.run_graph, replays))
    out = {"case": f"kernels_{N}x{H}x{W}x{C}_x2", "replays": replays,
           "bytes_moved": nbytes}
    for n in plans:
        out[n] = _summary(samples[n])
        out[n]["GBps"] = round(nbytes / out[n]["median_us"] / 1e3, 1)
    for n in ("resize_nearest", "resize_bilinear"):
        out[n]["bandwidth_vs_pool"] = round(
            out[n]["GBps"] / out["pool_max_2x2s2"]["GBps"], 3)
    return out


def _deconv_model(tmp, name, R, padding, gemm_lowering, cin=64, cout=64,
                  h=28, H=56):
    rng = np.random.default_rng(0)
    gb = GraphBuilder()
    f32 = gb.a_type(1)
    x = gb.placeholder("input", np.float32, [-1, h, h, cin],
                       signature_name="input")
    w = (rng.standard_normal((R, R, cout, cin)) * 0.1).astype(np.float32)
    # the node name keeps the SavedModel bytes distinct per case: plans
    # are cached by content, and the forced lowering must not be served
    # the other case's plan
    y = gb.node("Conv2DBackpropInput", f"deconv_{name}",
                [gb.const("sizes", np.array([-1, H, H, cout], np.int32)),
                 gb.const("w", w), x], T=f32,
                strides=gb.a_ints([1, 2, 2, 1]), padding=gb.a_str(padding),
                data_format=gb.a_str("NHWC"))
    y = gb.node("Relu", "relu", [y], T=f32)
    gb.mark_output("y", y)
    d = os.path.join(tmp, name, "1")
    write_saved_model(gb.build(), d)
    planner._Lowerer.DECONV_GEMM_LOWERING = gemm_lowering
    try:
        lm = load_model_from_dir(d, name, 1)
    finally:
        planner._Lowerer.DECONV_GEMM_LOWERING = True
    return lm


def _captured_context(lm, feeds):
    """Run twice (eager warm-up + capture, then a replay) and return the
    context of this batch's bucket, whose hipGraph holds the whole plan."""
    lm.predict(feeds)
    lm.predict(feeds)
    batch = next(iter(feeds.values())).shape[0]
    ctxs = lm._gpu._contexts[lm._gpu._bucket(batch)]
    return next(c for c in ctxs if c.captured and c.exec_plan.has_graph())


def deconv_cases(replays, rounds, batch=8):
    x = (np.random.default_rng(1).standard_normal((batch, 28, 28, 64))
         * 0.5).astype(np.float32)
    with tempfile.TemporaryDirectory() as tmp:
        models = {
            "2x2s2_gemm_transpose": _deconv_model(tmp, "a", 2, "VALID", True),
            "2x2s2_zero_insert_conv": _deconv_model(tmp, "b", 2, "VALID",
                                                    False),
            "3x3s2_same_zero_insert_conv": _deconv_model(tmp, "c", 3, "SAME",
                                                         True),
        }
    out = {"case": f"conv_transpose_b{batch}_28x28x64_to_56x56x64",
           "replays": replays}
    ctxs, outs = {}, {}
    for name, lm in models.items():
        lm._gpu = GpuModel(lm.plan, device=DEV, max_batch=batch,
                           model_name=name, model_version=1)
        ctxs[name] = _captured_context(lm, {"input": x})
        outs[name] = lm.predict({"input": x})["y"]
        out[name] = {"ops": [op.kind for op in lm.plan.ops]}
    out["max_abs_diff_2x2_a_vs_b"] = float(np.abs(
        outs["2x2s2_gemm_transpose"] -
        outs["2x2s2_zero_insert_conv"]).max())
    samples = {n: [] for n in models}
    for _ in range(rounds):
        for name, ctx in ctxs.items():
            with torch.cuda.stream(ctx.stream):
                samples[name].append(
                    _time_replays(ctx.exec_plan.run_graph, replays))
    for name in models:
        out[name].update(_summary(samples[name]))
        out[name]["kernels"] = ctxs[name].exec_plan.n_calls()
    out["b_over_a_2x2"] = round(
        out["2x2s2_zero_insert_conv"]["median_us"] /
        out["2x2s2_gemm_transpose"]["median_us"], 3)
    for lm in models.values():
        lm._gpu.release()
    return out


def unet_cases(replays, rounds):
    results = []
    for upsample in ("deconv", "nearest", "bilinear"):
        with tempfile.TemporaryDirectory() as tmp:
            d = os.path.join(tmp, "unet", "1")
            write_saved_model(build_unet(image_size=64, upsample=upsample),
                              d)
            lm = load_model_from_dir(d, f"unet_{upsample}", 1)
        lm._gpu = GpuModel(lm.plan, device=DEV, max_batch=16,
                           model_name=f"unet_{upsample}", model_version=1)
        out = {"case": f"unet64_{upsample}", "predicts": replays,
               "ops": len(lm.plan.ops)}
        for batch in (1, 16):
            x = (np.random.default_rng(batch).standard_normal(
                (batch, 64, 64, 3)) * 0.5).astype(np.float32)
            ctx = _captured_context(lm, {"input": x})
            samples = []
            for _ in range(rounds):
                t0 = time.perf_counter()
                for _ in range(replays):
                    lm.predict({"input": x})
                samples.append((time.perf_counter() - t0) / replays * 1e6)
            out[f"b{batch}_predict"] = _summary(samples)
            with torch.cuda.stream(ctx.stream):
                out[f"b{batch}_graph_replay"] = _summary(
                    [_time_replays(ctx.exec_plan.run_graph, replays)
                     for _ in range(rounds)])
            out[f"b{batch}_kernels"] = ctx.exec_plan.n_calls()
        lm._gpu.release()
        results.append(out)
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write JSON lines here")
    args = ap.parse_args()
    if args.replays < 200:
        ap.error("--replays must be >= 200")
    results = [kernel_cases(10 * args.replays, args.rounds)]
    print(json.dumps(results[-1]), flush=True)
    results.append(deconv_cases(5 * args.replays, args.rounds))
    print(json.dumps(results[-1]), flush=True)
    for r in unet_cases(args.replays, args.rounds):
        results.append(r)
        print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in results:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
