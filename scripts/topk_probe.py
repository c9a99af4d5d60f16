"""Timing probe for the top-k kernels (profiles/topk.md).

Each variant is one ExecPlan of CALLS identical ARGMAX_LAST top-k calls
on fixed device buffers, captured into a hipGraph. A sample is the wall
time of N back-to-back replays ending in one device synchronise, over
N * CALLS: time per launch, graph-launch cost amortised over CALLS. The
variants of a shape alternate, `--rounds` samples each, reported as
median (min - max); N is sized so a sample lasts about `--sample-ms`.

Variants per shape [rows, cols] and k:
  sort      k_topk_sort (bound moved up to cols; cols <= 2048 only)
  select    k_topk_select, P = 1 (bound moved down to 0)
  split_P   k_topk_select on P segments + the merge launch
and the yardsticks on the same rows: `argmax` (k_argmax_last, reads the
row once) and `unary` (ELT_UNARY relu, reads and writes it once).
Before timing, every variant's indices are compared with `select`'s.

    python scripts/topk_probe.py [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch  # noqa: E402

from tfservingcache_amd.engine import _tfsc_engine as ext  # noqa: E402

CALLS = 20
SORT_COLS = 2048            # k_topk_sort's LDS row


def _graph(call, stream):
    plan = ext.ExecPlan([call] * CALLS)
    with torch.cuda.stream(stream):
        plan.run()
        stream.synchronize()
        plan.capture()
        stream.synchronize()
    if not plan.has_graph():
        raise SystemExit("capture failed")
    return plan


def _sample(plan, stream, n):
    with torch.cuda.stream(stream):
        stream.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            plan.run_graph()
        stream.synchronize()
        return (time.perf_counter() - t0) / (n * CALLS) * 1e6


def shape_case(rows, cols, k, splits, rounds, sample_ms, stream):
    g = torch.Generator().manual_seed(rows * 31 + cols)
    x = torch.randn(rows, cols, generator=g).to(torch.bfloat16).cuda()
    y = torch.empty_like(x)
    idx1 = torch.empty(rows, dtype=torch.int32, device="cuda")
    default_bound = ext.topk_sort_max_cols()
    plans, outs = {}, {}

    def topk(name, bound, P):
        idx = torch.zeros(rows * k, dtype=torch.int32, device="cuda")
        vals = torch.zeros(rows * k, dtype=torch.bfloat16, device="cuda")
        scr = torch.zeros(max(rows * P * k, 1), dtype=torch.int64,
                          device="cuda")
        ext.set_topk_sort_max_cols(bound)
        plans[name] = _graph(
            (ext.K_ARGMAX_LAST,
             [x.data_ptr(), idx.data_ptr(), vals.data_ptr(),
              scr.data_ptr() if P > 1 else 0], [rows, cols, k, P], []),
            stream)
        ext.set_topk_sort_max_cols(default_bound)
        outs[name] = (idx, vals, scr)

    topk("select", 0, 1)
    if cols <= SORT_COLS:
        topk("sort", cols, 1)
    for P in splits:
        if P <= cols:
            topk(f"split_{P}", 0, P)
    plans["argmax"] = _graph((ext.K_ARGMAX_LAST,
                              [x.data_ptr(), idx1.data_ptr()],
                              [rows, cols], []), stream)
    plans["unary"] = _graph((ext.K_ELT_UNARY, [x.data_ptr(), y.data_ptr()],
                             [rows * cols, ext.ELT_RELU], []), stream)
    torch.cuda.synchronize()
    for name, (idx, _v, _s) in outs.items():
        if not torch.equal(idx, outs["select"][0]):
            raise SystemExit(f"[{rows},{cols}] k={k}: {name} disagrees")

    out = {"rows": rows, "cols": cols, "k": k, "calls_per_graph": CALLS,
           "row_bytes": rows * cols * 2}
    samples = {n: [] for n in plans}
    reps = {}
    for name, plan in plans.items():          # warm up + size the window
        t = _sample(plan, stream, 20)
        reps[name] = max(20, int(sample_ms * 1e3 / (t * CALLS)))
    for _ in range(rounds):
        for name, plan in plans.items():
            samples[name].append(_sample(plan, stream, reps[name]))
    for name, s in samples.items():
        out[name] = {"median_us": round(statistics.median(s), 2),
                     "min_us": round(min(s), 2), "max_us": round(max(s), 2),
                     "replays": reps[name]}
    return out


SHAPES = [
    # rows, cols, splits tried
    (1, 128, ()), (64, 128, ()), (1, 256, ()), (64, 256, ()),
    (1, 512, ()), (64, 512, ()), (1, 1000, ()), (8, 1000, ()),
    (64, 1000, ()), (1, 2048, ()), (64, 2048, ()),
    (1, 16384, (2, 4, 8)), (1, 32768, (2, 4, 8, 16)),
    (1, 100000, (2, 4, 8, 16, 32, 64)), (8, 100000, (2, 4, 8, 16, 32)),
    (64, 100000, (2, 4)), (256, 100000, (2,)),
    (1, 1000000, (8, 16, 32, 64, 128, 256)),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sample-ms", type=float, default=30.0)
    ap.add_argument("--out", default=None, help="also write JSON lines here")
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    for rows, cols, splits in SHAPES:
        for k in (10, 100):
            if k > cols:
                continue
            r = shape_case(rows, cols, k, splits, args.rounds,
                           args.sample_ms, stream)
            print(json.dumps(r), flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
