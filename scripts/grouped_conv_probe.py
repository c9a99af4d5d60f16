"""Timing probe for grouped convolution (profiles/grouped_conv.md).

1. The four grouped 3x3 layers of ResNeXt-50 32x4d at batch 8, each with
   BN and Relu folded, compiled twice: with the grouped lowering (merged
   super-groups on conv_igemm_grouped_kernel) and with
   GROUPED_CONV_DENSE (block-diagonal weight on the dense
   conv_igemm_kernel). One extra case, Cg = Ng = 1 at [8,56,56,128],
   compares the dense lowering the planner picks there with a merge of
   16 (GROUPED_CONV_MAX_MERGE raised), which is what the cap rules out.
2. build_resnext(224) under both lowerings at batch 1 and 16: hipGraph
   replay of the whole plan and warm GpuModel-backed predict.

One process. Figures are the wall time of N back-to-back graph replays
ending in one device synchronise, divided by N; the two lowerings of a
case alternate, five samples each, reported as median (min - max).

    python scripts/grouped_conv_probe.py [--replays 200] [--rounds 5]
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

from tfservingcache_amd.engine import planner  # noqa: E402
from tfservingcache_amd.engine.gpu import GpuModel  # noqa: E402
from tfservingcache_amd.engine.model import LoadedModel  # noqa: E402
from tfservingcache_amd.engine.savedmodel import (GraphBuilder,  # noqa: E402
                                                  read_saved_model,
                                                  write_saved_model)
from tfservingcache_amd.models import build_resnext  # noqa: E402

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


def _pad(v, m):
    return (v + m - 1) // m * m


def _compile(sm, name, dense, max_merge=None):
    """Compiled directly, not through the plan cache: it is keyed by the
    SavedModel's bytes, which both lowerings share."""
    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, name, "1")
        write_saved_model(sm, d)
        graph_def, sigs = read_saved_model(d)
    low = planner._Lowerer
    saved = (low.GROUPED_CONV_DENSE, low.GROUPED_CONV_MAX_MERGE)
    low.GROUPED_CONV_DENSE = dense
    if max_merge is not None:
        low.GROUPED_CONV_MAX_MERGE = max_merge
    try:
        plan = planner.compile_graph(graph_def, next(iter(sigs.values())))
    finally:
        low.GROUPED_CONV_DENSE, low.GROUPED_CONV_MAX_MERGE = saved
    return LoadedModel(name, 1, plan)


def _layer_graph(H, C, G):
    rng = np.random.default_rng(0)
    gb = GraphBuilder()
    f32 = gb.a_type(1)
    x = gb.placeholder("input", np.float32, [-1, H, H, C],
                       signature_name="input")
    w = (rng.standard_normal((3, 3, C // G, C)) * 0.1).astype(np.float32)
    y = gb.node("Conv2D", "conv", [x, gb.const("w", w)], T=f32,
                strides=gb.a_ints([1, 1, 1, 1]), padding=gb.a_str("SAME"),
                data_format=gb.a_str("NHWC"))
    consts = [gb.const(n, (np.abs(rng.standard_normal(C)) * 0.5 + 0.5
                           ).astype(np.float32))
              for n in ("gamma", "beta", "mean", "var")]
    y = gb.node("FusedBatchNormV3", "bn", [y] + consts, T=f32, U=f32,
                epsilon=gb.a_float(1e-5), is_training=gb.a_bool(False),
                data_format=gb.a_str("NHWC"))
    y = gb.node("Relu", "relu", [y], T=f32)
    gb.mark_output("y", y)
    return gb.build()


def _captured_context(lm, feeds):
    """Run twice (eager warm-up + capture, then a replay) and return the
    context of this batch's bucket, whose hipGraph holds the whole plan."""
    lm.predict(feeds)
    lm.predict(feeds)
    batch = next(iter(feeds.values())).shape[0]
    ctxs = lm._gpu._contexts[lm._gpu._bucket(batch)]
    return next(c for c in ctxs if c.captured and c.exec_plan.has_graph())


def _mfma_flops(op, M):
    """(issued MFMA FLOPs of the conv call, tile description)."""
    R, S, Cg, K = op.params["rsck"]
    G = op.params.get("groups", 1)
    if G == 1:
        return 2 * _pad(M, 128) * _pad(R * S * Cg, 64) * _pad(K, 128), \
            "128x128"
    Ng = K // G
    bn = 16 if Ng <= 16 else 32 if Ng <= 32 else 64
    return 2 * _pad(M, 128) * _pad(R * S * Cg, 64) * _pad(Ng, bn) * G, \
        f"128x{bn} x{G} groups"


def layer_case(H, C, G, batch, replays, rounds, max_merge=None):
    sm = _layer_graph(H, C, G)
    tag = f"{H}x{H}x{C}_g{G}"
    models = {
        "grouped": _compile(sm, f"g_{tag}", False, max_merge),
        "dense": _compile(sm, f"d_{tag}", True),
    }
    default_plan = _compile(sm, f"p_{tag}", False).plan
    x = (np.random.default_rng(1).standard_normal((batch, H, H, C)) * 0.5
         ).astype(np.float32)
    M = batch * H * H
    useful = 2 * M * 9 * (C // G) * C
    out = {"case": f"conv3x3_b{batch}_{tag}", "replays": replays,
           "useful_flops": useful,
           "planner_default": "grouped" if any(
               "groups" in op.params for op in default_plan.ops)
           else "dense"}
    ctxs, outs = {}, {}
    for name, lm in models.items():
        lm._gpu = GpuModel(lm.plan, device=DEV, max_batch=batch,
                           model_name=f"{name}_{tag}", model_version=1)
        ctxs[name] = _captured_context(lm, {"input": x})
        outs[name] = lm.predict({"input": x})["y"]
        op = next(op for op in lm.plan.ops if op.kind == "conv2d")
        issued, tile = _mfma_flops(op, M)
        out[name] = {"rsck": list(op.params["rsck"]),
                     "groups": op.params.get("groups", 1), "tile": tile,
                     "issued_flops": issued,
                     "useful_over_issued": round(useful / issued, 4),
                     "kernels": ctxs[name].exec_plan.n_calls()}
    out["max_abs_diff"] = float(np.abs(outs["grouped"] -
                                       outs["dense"]).max())
    samples = {n: [] for n in models}
    for _ in range(rounds):
        for name, ctx in ctxs.items():
            with torch.cuda.stream(ctx.stream):
                samples[name].append(
                    _time_replays(ctx.exec_plan.run_graph, replays))
    for name in models:
        out[name].update(_summary(samples[name]))
    out["dense_over_grouped"] = round(
        out["dense"]["median_us"] / out["grouped"]["median_us"], 3)
    for lm in models.values():
        lm._gpu.release()
    return out


def model_case(replays, rounds):
    sm = build_resnext(image_size=224)
    models = {"grouped": _compile(sm, "rx_grouped", False),
              "dense": _compile(sm, "rx_dense", True)}
    out = {"case": "resnext50_32x4d_224", "predicts": replays}
    for name, lm in models.items():
        lm._gpu = GpuModel(lm.plan, device=DEV, max_batch=16,
                           model_name=f"rx_{name}", model_version=1)
        out[name] = {"grouped_convs": sum(
            1 for op in lm.plan.ops if "groups" in op.params)}
    for batch in (1, 16):
        x = (np.random.default_rng(batch).standard_normal(
            (batch, 224, 224, 3)) * 0.5).astype(np.float32)
        ctxs = {n: _captured_context(lm, {"input": x})
                for n, lm in models.items()}
        replay = {n: [] for n in models}
        predict = {n: [] for n in models}
        for _ in range(rounds):
            for name, lm in models.items():
                ctx = ctxs[name]
                with torch.cuda.stream(ctx.stream):
                    replay[name].append(
                        _time_replays(ctx.exec_plan.run_graph, replays))
                t0 = time.perf_counter()
                for _ in range(replays):
                    lm.predict({"input": x})
                predict[name].append(
                    (time.perf_counter() - t0) / replays * 1e6)
        for name in models:
            out[name][f"b{batch}_graph_replay"] = _summary(replay[name])
            out[name][f"b{batch}_predict"] = _summary(predict[name])
            out[name][f"b{batch}_kernels"] = ctxs[name].exec_plan.n_calls()
    for lm in models.values():
        lm._gpu.release()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write JSON lines here")
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    results = []
    for H, C in ((56, 128), (28, 256), (14, 512), (7, 1024)):
        results.append(layer_case(H, C, 32, 8, 5 * args.replays,
                                  args.rounds))
        print(json.dumps(results[-1]), flush=True)
    # what the merge cap rules out: Cg = Ng = 1 needs m = 16
    results.append(layer_case(56, 128, 128, 8, 5 * args.replays,
                              args.rounds, max_merge=16))
    print(json.dumps(results[-1]), flush=True)
    if not args.skip_model:
        results.append(model_case(args.replays // 4, args.rounds))
        print(json.dumps(results[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in results:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
