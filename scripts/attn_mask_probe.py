"""Timing probe for additive attention masks (profiles/attention_mask.md).

1. Masked BERT-base (build_bert(with_mask=True), default sizes) at b=8,
   S=128 and S=384: hipGraph replay time of the fused plan vs the
   unfused plan (_Lowerer(...).run(), what the engine ran for this
   graph before the mask was fusable). The two plans alternate, several
   rounds each, so drift hits both alike.
2. The bare attention kernel at the profiles/attention_r02.md shapes
   (B=16, H=12, S=128 and S=512): null bias vs [B,1,1,S] key-padding
   bias.

Every figure is the wall time of N back-to-back replays ending in one
device synchronise, divided by N (N >= 200 for the models, 10x that for
the bare kernel so the window is tens of milliseconds); the spread over
the rounds is printed next to the median.

    python scripts/attn_mask_probe.py [--replays 200] [--rounds 5]
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
    """Run twice (eager warm-up + capture, then a replay) and return the
    context whose hipGraph now holds the whole plan."""
    lm.predict(feeds)
    lm.predict(feeds)
    ctxs = [c for lst in lm._gpu._contexts.values() for c in lst]
    return next(c for c in ctxs if c.captured and c.exec_plan.has_graph())


def bert_case(seq_len, batch, replays, rounds, layers):
    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, "mb", "1")
        write_saved_model(build_bert(seq_len=seq_len, layers=layers,
                                     with_mask=True), d)
        fused = load_model_from_dir(d, "mb", 1)
        gd, sigs = read_saved_model(d)
        unfused = LoadedModel(
            "mb_unfused", 1, _Lowerer(gd, next(iter(sigs.values()))).run())
    kinds = [op.kind for op in fused.plan.ops]
    assert kinds.count("attention") == layers and "softmax" not in kinds
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
    out = {"case": f"bert_base_masked_b{batch}_s{seq_len}",
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


def kernel_case(S, replays, rounds, B=16, H=12, D=64):
    dev = "cuda:0"
    q, k, v = ((torch.randn(B, S, H, D, device=dev) * 0.5)
               .to(torch.bfloat16).contiguous() for _ in range(3))
    o = torch.empty_like(q)
    lens = torch.randint(S // 4, S + 1, (B,), device=dev)
    bias = torch.where(torch.arange(S, device=dev)[None, :] < lens[:, None],
                       0.0, -10000.0).to(torch.bfloat16).contiguous()
    base = [q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr()]
    scale = [1.0 / D ** 0.5]
    plans = {
        "null_bias": ext.ExecPlan([(ext.K_ATTENTION, base, [B, S, H, D],
                                    scale)]),
        "key_padding_bias": ext.ExecPlan(
            [(ext.K_ATTENTION, base + [bias.data_ptr()],
              [B, S, H, D, S, 0, 0], scale)]),
    }
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
    out = {"case": f"attention_kernel_B{B}_H{H}_S{S}", "replays": replays}
    for n in plans:
        out[n] = _summary(samples[n])
    out["bias_cost_median"] = round(
        out["key_padding_bias"]["median_us"] /
        out["null_bias"]["median_us"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=None, help="also write JSON lines here")
    args = ap.parse_args()
    if args.replays < 200:
        ap.error("--replays must be >= 200")
    results = []
    for S in (128, 512):
        results.append(kernel_case(S, 10 * args.replays, args.rounds))
        print(json.dumps(results[-1]), flush=True)
    for S in (128, 384):
        results.append(bert_case(S, args.batch, args.replays, args.rounds,
                                 args.layers))
        print(json.dumps(results[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in results:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
