"""Timing probe for dilated convolution (profiles/dilated_conv.md).

1. Dense kernels, one K_CONV call each on bf16 tensors, 3x3 SAME with a
   fused relu: conv_igemm_dilated_kernel with dead-tap skipping, the same
   kernel with the skip compiled out (set_conv_dilated_skip(0)), and
   the existing conv_igemm_kernel at dilation 1 on the same shape as the
   yardstick (the same issued MFMA work as skip-off).
   (a) no dead taps: [8,65,65,256] -> 256 at d = 2;
   (b) ASPP: [8,33,33,512] -> 256 at d = 6, 12, 18 and
       [8,65,65,512] -> 256 at d = 12, 24, 36,
   with the fraction of K tiles the skip leaves out, counted here by the
   kernel's own rule.
2. Depthwise 3x3 [8,33,33,512] at d = 2 and d = 12 (k_depthwise_dilated_v8)
   against k_depthwise_v4 at d = 1.
3. build_deeplab(65) at batch 1 and 16: hipGraph replay of the whole plan
   and warm GpuModel-backed predict.

One process. Figures are the wall time of N back-to-back graph replays
ending in one device synchronise, divided by N; the variants of a case
alternate, five samples each, reported as median (min - max).

    python scripts/dilated_conv_probe.py [--replays 2000] [--rounds 5]
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
from tfservingcache_amd.engine.gpu import GpuModel  # noqa: E402
from tfservingcache_amd.engine.model import load_model_from_dir  # noqa: E402
from tfservingcache_amd.engine.savedmodel import write_saved_model  # noqa: E402
from tfservingcache_amd.models import build_deeplab  # noqa: E402

DEV = "cuda:0"
BF = torch.bfloat16


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


def _captured(kind, ptrs, ints, stream):
    """One call, run eagerly once and captured into a hipGraph."""
    plan = ext.ExecPlan([(kind, ptrs, ints, [])])
    with torch.cuda.stream(stream):
        plan.run()
        torch.cuda.synchronize()
        plan.capture()
        for _ in range(20):
            plan.run_graph()
        torch.cuda.synchronize()
    return plan


def _alternate(plans, stream, replays, rounds):
    samples = {n: [] for n in plans}
    for _ in range(rounds):
        for name, plan in plans.items():
            with torch.cuda.stream(stream):
                samples[name].append(_time_replays(plan.run_graph, replays))
    return {n: _summary(s) for n, s in samples.items()}


def _skipped_fraction(N, H, C, R, d):
    """K tiles the dilated kernel leaves out, over all blocks of one
    column of N tiles: its rule (min/max of hi0, wi0 over the 128 rows of
    an M tile), 3x3-style SAME at stride 1 (pad = d)."""
    M = N * H * H
    m = np.arange(M)
    hi0 = (m // H) % H - d
    wi0 = m % H - d
    live = total = 0
    for m0 in range(0, M, 128):
        h, w = hi0[m0:m0 + 128], wi0[m0:m0 + 128]
        for r in range(R):
            for s in range(R):
                dead = h.max() + r * d < 0 or h.min() + r * d >= H or \
                    w.max() + s * d < 0 or w.min() + s * d >= H
                live += 0 if dead else C // 64
                total += C // 64
    return round(1.0 - live / total, 4)


def dense_case(N, H, C, K, d, stream, replays, rounds):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N, H, H, C, generator=g).to(BF).to(DEV)
    w = (torch.randn(K, 9 * C, generator=g) * 0.05).to(BF).to(DEV)
    b = torch.randn(K, generator=g).to(BF).to(DEV)
    zeros = torch.zeros(64, dtype=BF, device=DEV)
    ys = {n: torch.empty(N * H * H * K, dtype=BF, device=DEV)
          for n in ("skip_on", "skip_off", "dense_d1")}

    def ints(pad, tail):
        return [N, H, H, C, K, 3, 3, 1, 1, pad, pad, H, H, 9 * C, 1] + tail

    def ptrs(name):
        return [x.data_ptr(), w.data_ptr(), b.data_ptr(), 0,
                zeros.data_ptr(), ys[name].data_ptr()]

    plans = {}
    for name, mode in (("skip_on", 2), ("skip_off", 0)):
        ext.set_conv_dilated_skip(mode)         # read at launch = capture
        plans[name] = _captured(ext.K_CONV, ptrs(name), ints(d, [1, d, d]),
                                stream)
    ext.set_conv_dilated_skip(1)
    plans["dense_d1"] = _captured(ext.K_CONV, ptrs("dense_d1"), ints(1, []),
                                  stream)
    out = {"case": f"conv3x3_b{N}_{H}x{H}x{C}_k{K}_d{d}", "replays": replays,
           "blocks": -(-N * H * H // 128) * -(-K // 128),
           "k_tiles": 9 * C // 64,
           "k_tiles_skipped": _skipped_fraction(N, H, C, 3, d),
           "default_skips": -(-N * H * H // 128) * -(-K // 128) > 256
           and 2 * d * 8 >= H,
           "skip_on_equals_skip_off": bool(torch.equal(ys["skip_on"],
                                                       ys["skip_off"]))}
    out.update(_alternate(plans, stream, replays, rounds))
    for n in ("skip_off", "dense_d1"):
        out[f"skip_on_over_{n}"] = round(
            out["skip_on"]["median_us"] / out[n]["median_us"], 3)
    return out


def depthwise_case(N, H, C, rates, stream, replays, rounds):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N, H, H, C, generator=g).to(BF).to(DEV)
    w = (torch.randn(9 * C, generator=g) * 0.2).to(BF).to(DEV)
    b = torch.randn(C, generator=g).to(BF).to(DEV)
    plans, keep = {}, []
    for d in (1,) + tuple(rates):
        y = torch.empty(N * H * H * C, dtype=BF, device=DEV)
        keep.append(y)
        ints = [N, H, H, C, 3, 3, 1, 1, d, d, H, H, 1] + \
            ([1, d, d] if d > 1 else [])
        plans[f"d{d}"] = _captured(
            ext.K_DEPTHWISE,
            [x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr()], ints,
            stream)
    out = {"case": f"depthwise3x3_b{N}_{H}x{H}x{C}", "replays": replays}
    out.update(_alternate(plans, stream, replays, rounds))
    for d in rates:
        out[f"d{d}_over_d1"] = round(
            out[f"d{d}"]["median_us"] / out["d1"]["median_us"], 3)
    return out


def model_case(replays, rounds):
    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, "deeplab", "1")
        write_saved_model(build_deeplab(image_size=65), d)
        lm = load_model_from_dir(d, "deeplab", 1)
    lm._gpu = GpuModel(lm.plan, device=DEV, max_batch=16,
                       model_name="deeplab", model_version=1)
    out = {"case": "deeplab_65", "predicts": replays,
           "dilated_ops": sum("dilation" in op.params for op in lm.plan.ops)}
    for batch in (1, 16):
        x = (np.random.default_rng(batch).standard_normal(
            (batch, 65, 65, 3)) * 0.5).astype(np.float32)
        lm.predict({"input": x})
        lm.predict({"input": x})
        ctxs = lm._gpu._contexts[lm._gpu._bucket(batch)]
        ctx = next(c for c in ctxs if c.captured and c.exec_plan.has_graph())
        replay, predict = [], []
        for _ in range(rounds):
            with torch.cuda.stream(ctx.stream):
                replay.append(_time_replays(ctx.exec_plan.run_graph, replays))
            t0 = time.perf_counter()
            for _ in range(replays):
                lm.predict({"input": x})
            predict.append((time.perf_counter() - t0) / replays * 1e6)
        out[f"b{batch}_graph_replay"] = _summary(replay)
        out[f"b{batch}_predict"] = _summary(predict)
        out[f"b{batch}_kernels"] = ctx.exec_plan.n_calls()
    lm._gpu.release()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write JSON lines here")
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dilated_conv_probe needs a GPU")
    stream = torch.cuda.Stream(device=DEV)
    results = []

    def emit(r):
        results.append(r)
        print(json.dumps(r), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(r) + "\n")

    emit(dense_case(8, 65, 256, 256, 2, stream, args.replays, args.rounds))
    for H, rates in ((33, (6, 12, 18)), (65, (12, 24, 36))):
        for d in rates:
            emit(dense_case(8, H, 512, 256, d, stream, args.replays,
                            args.rounds))
    emit(depthwise_case(8, 33, 512, (2, 12), stream, args.replays,
                        args.rounds))
    if not args.skip_model:
        emit(model_case(args.replays // 4, args.rounds))


if __name__ == "__main__":
    main()
