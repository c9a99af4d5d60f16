"""Timing probe for depthwise convolution with a depth multiplier
(profiles/depthwise_multiplier.md).

1. Single layers at batch 8, DepthwiseConv2dNative [R,S,C,M] + BN +
   Relu6, compiled twice: as written (the depthwise kernels of
   csrc/ops/ops_memory.hip) and with the node respelled as a grouped
   Conv2D, filter [R,S,1,C*M], which is the only way the planner could
   run this maths before DepthwiseConv2dNative took a multiplier
   (lower_conv: merged groups on the grouped implicit-GEMM kernel or a
   dense conv on a block-diagonal weight).
2. build_separable_cnn(224) under both spellings at batch 1 and 16:
   hipGraph replay of the whole plan.

The two outputs are compared first, on the same seeded input, within
2^-8 * max|y| (each is one bf16 rounding of an f32 sum). One process.
Figures are the wall time of N back-to-back graph replays ending in one
device synchronise, divided by N; the two lowerings of a case alternate,
five samples each, reported as median (min - max). `bytes` is what the
conv has to move, from shapes: x once, y once, w and bias, all bf16;
`gbps` is bytes over the median replay time (a whole-replay figure: it
includes the graph launch) and `of_hbm_peak` is that over 8 TB/s.

    python scripts/depthwise_multiplier_probe.py [--replays 200] [--rounds 5]
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
from tfservingcache_amd.models import build_separable_cnn  # noqa: E402
from tfservingcache_amd.wire.tensor import (numpy_to_tensorproto,  # noqa: E402
                                            tensorproto_to_numpy)

DEV = "cuda:0"
HBM_PEAK = 8.0e12           # bytes/s, MI355X HBM3E spec peak


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


def _as_conv2d(sm):
    """Respell every DepthwiseConv2dNative [R,S,C,M] of a SavedModel, in
    place, as Conv2D [R,S,1,C*M]: the same maths through lower_conv."""
    nodes = sm.meta_graphs[0].graph_def.node
    by_name = {nd.name: nd for nd in nodes}
    for nd in nodes:
        if nd.op != "DepthwiseConv2dNative":
            continue
        nd.op = "Conv2D"
        wn = by_name[nd.input[1].split(":")[0]]
        w = tensorproto_to_numpy(wn.attr["value"].tensor)
        R, S, C, M = w.shape
        wn.attr["value"].tensor = numpy_to_tensorproto(
            np.ascontiguousarray(w.reshape(R, S, 1, C * M)))
    return sm


def _compile(sm, name):
    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, name, "1")
        write_saved_model(sm, d)
        graph_def, sigs = read_saved_model(d)
    plan = planner.compile_graph(graph_def, next(iter(sigs.values())))
    return LoadedModel(name, 1, plan)


def _layer_graph(H, C, M, k, stride):
    rng = np.random.default_rng(0)
    K = C * M
    gb = GraphBuilder()
    f32 = gb.a_type(1)
    x = gb.placeholder("input", np.float32, [-1, H, H, C],
                       signature_name="input")
    w = (rng.standard_normal((k, k, C, M)) * 0.3).astype(np.float32)
    y = gb.node("DepthwiseConv2dNative", "dw", [x, gb.const("w", w)], T=f32,
                strides=gb.a_ints([1, stride, stride, 1]),
                padding=gb.a_str("SAME"), data_format=gb.a_str("NHWC"))
    consts = [gb.const(n, (np.abs(rng.standard_normal(K)) * 0.5 + 0.5
                           ).astype(np.float32))
              for n in ("gamma", "beta", "mean", "var")]
    y = gb.node("FusedBatchNormV3", "bn", [y] + consts, T=f32, U=f32,
                epsilon=gb.a_float(1e-5), is_training=gb.a_bool(False),
                data_format=gb.a_str("NHWC"))
    y = gb.node("Relu6", "relu6", [y], T=f32)
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


def _describe(lm):
    """How the conv lowered: kinds of the plan's ops and, for conv2d,
    rsck / groups."""
    out = []
    for op in lm.plan.ops:
        if op.kind == "depthwise_conv":
            out.append({"kind": op.kind, "rsc": list(op.params["rsc"]),
                        "mult": op.params.get("mult", 1)})
        elif op.kind == "conv2d":
            out.append({"kind": op.kind, "rsck": list(op.params["rsck"]),
                        "groups": op.params.get("groups", 1)})
        else:
            out.append({"kind": op.kind})
    return out


def _kernel_variant(C, M):
    if M == 1:
        return "k_depthwise_v4" if C % 4 == 0 else "k_depthwise_scalar"
    if (C * M) % 8 == 0 and (M in (2, 4) or M % 8 == 0):
        return f"k_depthwise_mult_v8<{8 // M if M < 8 else 1}>"
    return "k_depthwise_mult_scalar"


def layer_case(H, C, M, k, stride, batch, replays, rounds):
    tag = f"{H}x{H}x{C}_m{M}_k{k}s{stride}"
    models = {
        "depthwise": _compile(_layer_graph(H, C, M, k, stride), f"dw_{tag}"),
        "conv2d": _compile(_as_conv2d(_layer_graph(H, C, M, k, stride)),
                           f"cv_{tag}"),
    }
    x = (np.random.default_rng(1).standard_normal((batch, H, H, C)) * 0.5
         ).astype(np.float32)
    Ho = -(-H // stride)
    K = C * M
    nbytes = 2 * (batch * H * H * C + batch * Ho * Ho * K + k * k * K + K)
    out = {"case": f"dw_b{batch}_{tag}", "replays": replays,
           "bytes": nbytes, "kernel": _kernel_variant(C, M)}
    ctxs, outs = {}, {}
    for name, lm in models.items():
        lm._gpu = GpuModel(lm.plan, device=DEV, max_batch=batch,
                           model_name=f"{name}_{tag}", model_version=1)
        ctxs[name] = _captured_context(lm, {"input": x})
        outs[name] = lm.predict({"input": x})["y"]
        out[name] = {"ops": _describe(lm),
                     "kernels": ctxs[name].exec_plan.n_calls()}
    diff = float(np.abs(outs["depthwise"] - outs["conv2d"]).max())
    bound = 2.0 ** -8 * float(np.abs(outs["conv2d"]).max())
    out["max_abs_diff"], out["diff_bound"] = diff, bound
    if not diff <= bound:
        raise SystemExit(f"{tag}: lowerings disagree, {diff} > {bound}")
    samples = {n: [] for n in models}
    for _ in range(rounds):
        for name, ctx in ctxs.items():
            with torch.cuda.stream(ctx.stream):
                samples[name].append(
                    _time_replays(ctx.exec_plan.run_graph, replays))
    for name in models:
        out[name].update(_summary(samples[name]))
        gbps = nbytes / (out[name]["median_us"] * 1e-6) / 1e9
        out[name]["gbps"] = round(gbps, 1)
        out[name]["of_hbm_peak"] = round(gbps * 1e9 / HBM_PEAK, 4)
    out["conv2d_over_depthwise"] = round(
        out["conv2d"]["median_us"] / out["depthwise"]["median_us"], 3)
    for lm in models.values():
        lm._gpu.release()
    return out


def model_case(replays, rounds):
    models = {
        "depthwise": _compile(build_separable_cnn(image_size=224),
                              "sep_dw"),
        "conv2d": _compile(_as_conv2d(build_separable_cnn(image_size=224)),
                           "sep_cv"),
    }
    out = {"case": "separable_cnn_224", "replays": replays}
    for name, lm in models.items():
        lm._gpu = GpuModel(lm.plan, device=DEV, max_batch=16,
                           model_name=f"sep_{name}", model_version=1)
        out[name] = {"ops": [d for d in _describe(lm)
                             if d["kind"] == "depthwise_conv" or
                             d.get("groups", 1) > 1]}
    for batch in (1, 16):
        x = (np.random.default_rng(batch).standard_normal(
            (batch, 224, 224, 3)) * 0.5).astype(np.float32)
        ctxs = {n: _captured_context(lm, {"input": x})
                for n, lm in models.items()}
        probs = {n: lm.predict({"input": x})["probs"]
                 for n, lm in models.items()}
        out[f"b{batch}_max_abs_diff_probs"] = float(
            np.abs(probs["depthwise"] - probs["conv2d"]).max())
        replay = {n: [] for n in models}
        for _ in range(rounds):
            for name in models:
                ctx = ctxs[name]
                with torch.cuda.stream(ctx.stream):
                    replay[name].append(
                        _time_replays(ctx.exec_plan.run_graph, replays))
        for name in models:
            out[name][f"b{batch}_graph_replay"] = _summary(replay[name])
            out[name][f"b{batch}_kernels"] = ctxs[name].exec_plan.n_calls()
    for lm in models.values():
        lm._gpu.release()
    return out


# (H, C, M, k, stride) at batch 8
LAYERS = [(56, 128, 2, 3, 1), (28, 256, 2, 3, 2), (112, 32, 4, 3, 1),
          (14, 512, 3, 3, 1), (28, 64, 8, 3, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write JSON lines here")
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    results = []

    def done(r):
        results.append(r)
        print(json.dumps(r), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(r) + "\n")

    for H, C, M, k, stride in LAYERS:
        done(layer_case(H, C, M, k, stride, 8, args.replays, args.rounds))
    if not args.skip_model:
        done(model_case(args.replays, args.rounds))


if __name__ == "__main__":
    main()
