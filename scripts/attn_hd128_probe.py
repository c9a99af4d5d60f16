"""Timing probe for the head_dim 128 attention geometry
(profiles/attention_hd128.md).

1. The bare kernel at B=16, S=128 and S=512: H=8, D=128 (null bias and
   [B,1,1,S] key-padding bias) next to H=16, D=64 (null bias), the same
   H*D and therefore the same FLOPs and bytes, in one process.
2. A 12-layer build_bert(hidden=1024, heads=8, intermediate=4096,
   with_mask=True) at b=8, S=128 and S=384: hipGraph replay time of the
   fused plan vs the unfused plan (_Lowerer(...).run(), what the engine
   ran for 128-wide heads before the kernel had this geometry).

Method of scripts/attn_mask_probe.py: captured graphs, N back-to-back
replays ending in one device synchronise divided by N (N >= 200 for the
models, 10x that for the bare kernel), the candidates alternating over
several rounds; median with min - max.

    python scripts/attn_hd128_probe.py [--replays 200] [--rounds 5]
                                       [--kernel-only]
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
from tfservingcache_amd.engine.model import (LoadedModel,  # noqa: E402
                                             load_model_from_dir)
from tfservingcache_amd.engine.planner import _Lowerer  # noqa: E402
from tfservingcache_amd.engine.savedmodel import (read_saved_model,  # noqa: E402
                                                  write_saved_model)
from tfservingcache_amd.models import build_bert  # noqa: E402

BERT = dict(hidden=1024, heads=8, intermediate=4096, with_mask=True)


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


def _captured_context(lm, feeds):
    lm.predict(feeds)
    lm.predict(feeds)
    ctxs = [c for lst in lm._gpu._contexts.values() for c in lst]
    return next(c for c in ctxs if c.captured and c.exec_plan.has_graph())


def bert_case(seq_len, batch, replays, rounds, layers):
    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, "mb", "1")
        write_saved_model(build_bert(seq_len=seq_len, layers=layers,
                                     **BERT), d)
        fused = load_model_from_dir(d, "mb", 1)
        gd, sigs = read_saved_model(d)
        unfused = LoadedModel(
            "mb_unfused", 1, _Lowerer(gd, next(iter(sigs.values()))).run())
    att = [op for op in fused.plan.ops if op.kind == "attention"]
    assert len(att) == layers and all(
        op.params["head_dim"] == 128 and len(op.inputs) == 4 for op in att)
    assert not any(op.kind == "attention" for op in unfused.plan.ops)
    rng = np.random.default_rng(0)
    lens = rng.integers(seq_len // 4, seq_len + 1, batch)
    feeds = {"input_ids": rng.integers(0, 30522, (batch, seq_len)).astype(
                 np.int32),
             "input_mask": (np.arange(seq_len)[None, :] < lens[:, None]
                            ).astype(np.int32)}
    samples = {"fused": [], "unfused": []}
    ctxs = {}
    for name, lm in (("fused", fused), ("unfused", unfused)):
        lm._gpu = GpuModel(lm.plan, device="cuda:0", max_batch=batch,
                           model_name=name, model_version=1)
        ctxs[name] = _captured_context(lm, feeds)
    for _ in range(rounds):
        for name in ("fused", "unfused"):
            ctx = ctxs[name]
            with torch.cuda.stream(ctx.stream):
                samples[name].append(
                    _time_replays(ctx.exec_plan.run_graph, replays))
    out = {"case": f"bert_h1024_hd128_masked_b{batch}_s{seq_len}",
           "layers": layers, "replays": replays,
           "kernels_fused": ctxs["fused"].exec_plan.n_calls(),
           "kernels_unfused": ctxs["unfused"].exec_plan.n_calls(),
           "fused": _summary(samples["fused"]),
           "unfused": _summary(samples["unfused"])}
    out["speedup_median"] = round(out["unfused"]["median_us"] /
                                  out["fused"]["median_us"], 3)
    for lm in (fused, unfused):
        lm._gpu.release()
    return out


def kernel_case(S, replays, rounds, B=16):
    dev = "cuda:0"
    keep = []

    def plan(H, D, with_bias):
        q, k, v = ((torch.randn(B, S, H, D, device=dev) * 0.5)
                   .to(torch.bfloat16).contiguous() for _ in range(3))
        o = torch.empty_like(q)
        keep.extend([q, k, v, o])
        ptrs = [q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr()]
        ints = [B, S, H, D]
        if with_bias:
            lens = torch.randint(S // 4, S + 1, (B,), device=dev)
            bias = torch.where(
                torch.arange(S, device=dev)[None, :] < lens[:, None],
                0.0, -10000.0).to(torch.bfloat16).contiguous()
            keep.append(bias)
            ptrs.append(bias.data_ptr())
            ints += [S, 0, 0]
        return ext.ExecPlan([(ext.K_ATTENTION, ptrs, ints, [D ** -0.5])])

    plans = {"hd128_null_bias": plan(8, 128, False),
             "hd128_key_padding_bias": plan(8, 128, True),
             "hd64_h16_null_bias": plan(16, 64, False)}
    stream = torch.cuda.Stream(device=dev)
    samples = {n: [] for n in plans}
    with torch.cuda.stream(stream):
        for p in plans.values():
            p.run()
            stream.synchronize()
            p.capture()
        for _ in range(rounds):
            for n, p in plans.items():
                samples[n].append(_time_replays(p.run_graph, replays))
    # QK^T and PV: 2 * 2 * B * H * S * S * D, the same for both geometries
    flops = 4.0 * B * 8 * S * S * 128
    out = {"case": f"attention_kernel_B{B}_HD1024_S{S}", "replays": replays}
    for n in plans:
        out[n] = _summary(samples[n])
        out[n]["tflops"] = round(flops / out[n]["median_us"] * 1e-6, 1)
    out["bias_cost_median"] = round(
        out["hd128_key_padding_bias"]["median_us"] /
        out["hd128_null_bias"]["median_us"], 3)
    out["hd128_over_hd64_time"] = round(
        out["hd128_null_bias"]["median_us"] /
        out["hd64_h16_null_bias"]["median_us"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--kernel-only", action="store_true",
                    help="skip the BERT cases")
    ap.add_argument("--out", default=None, help="also write JSON lines here")
    args = ap.parse_args()
    if args.replays < 200:
        ap.error("--replays must be >= 200")
    results = []
    for S in (128, 512):
        results.append(kernel_case(S, 10 * args.replays, args.rounds))
        print(json.dumps(results[-1]), flush=True)
    if not args.kernel_only:
        for S in (128, 384):
            results.append(bert_case(S, args.batch, args.replays,
                                     args.rounds, args.layers))
            print(json.dumps(results[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in results:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
