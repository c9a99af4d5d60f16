"""Timing probe for the reduce kernels (profiles/reductions.md).

Method as in topk_probe.py: each variant is one ExecPlan of CALLS
identical calls on fixed device buffers, captured into a hipGraph. A
sample is the wall time of N back-to-back replays ending in one device
synchronise, over N * CALLS. The variants of a shape alternate,
`--rounds` samples each, reported as median (min - max); N is sized so a
sample lasts about `--sample-ms`. Every variant reads the same input
buffer, and its result is compared with the first variant's before
timing.

Variants per view [outer, red, inner], all with fn = mean:
  old        the yardstick: k_mean_last (inner == 1) or k_mean_mid
  new        launch_reduce as the engine calls it (P from
             emit.reduce_segments, thresholds as shipped)
  wave/block inner == 1: the row form forced by moving the handover
  tx_N       inner > 1: tile width N lanes (the cap moved, the
             narrowing rule switched off)
  split_P    P segments + the second launch

    python scripts/reduce_probe.py [--rounds 7] [--out FILE]
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
from tfservingcache_amd.engine import emit  # noqa: E402

CALLS = 20
MEAN = 0


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


def view_case(outer, red, inner, splits, rounds, sample_ms, stream):
    g = torch.Generator().manual_seed(outer * 31 + red)
    x = torch.randn(outer * red * inner, generator=g).to(
        torch.bfloat16).cuda()
    wave0, tx0, wgs0 = (ext.reduce_wave_max_cols(), ext.reduce_cols_tx_max(),
                        ext.reduce_cols_wg_target())
    plans, outs = {}, {}

    def reduce(name, P, wave=wave0, tx=tx0, wgs=wgs0):
        y = torch.zeros(outer * inner, dtype=torch.bfloat16, device="cuda")
        scr = torch.zeros(max(outer * inner * P, 1), dtype=torch.float32,
                          device="cuda")
        ptrs = [x.data_ptr(), y.data_ptr(), scr.data_ptr() if P > 1 else 0]
        ext.set_reduce_thresholds(wave, tx, wgs)
        plans[name] = _graph(
            (ext.K_MEAN_LAST, ptrs, [outer, red, MEAN, P], []) if inner == 1
            else (ext.K_MEAN_MID, ptrs, [outer, red, inner, MEAN, P], []),
            stream)
        ext.set_reduce_thresholds(wave0, tx0, wgs0)
        outs[name] = (y, scr)

    y_old = torch.zeros(outer * inner, dtype=torch.bfloat16, device="cuda")
    outs["old"] = (y_old, None)
    plans["old"] = _graph(
        (ext.K_MEAN_LAST, [x.data_ptr(), y_old.data_ptr()], [outer, red], [])
        if inner == 1 else
        (ext.K_MEAN_MID, [x.data_ptr(), y_old.data_ptr()],
         [outer, red, inner], []), stream)
    P_new = emit.reduce_segments(outer, red, inner)
    reduce("new", P_new)
    if inner == 1:
        if red <= 16384:
            reduce("wave", 1, wave=1 << 30)
        reduce("block", 1, wave=0)
    else:
        for tx in (4, 8, 16, 32, 64):
            if tx * 8 <= inner:
                reduce(f"tx_{tx}", 1, tx=tx, wgs=0)
    for P in splits:
        reduce(f"split_{P}", P)
    torch.cuda.synchronize()
    # reordered f32 sums: the results agree to one bf16 step
    ref = outs["old"][0].float()
    for name, (y, _s) in outs.items():
        if not torch.allclose(y.float(), ref, rtol=2 ** -7, atol=1e-3):
            raise SystemExit(f"[{outer},{red},{inner}]: {name} disagrees")

    out = {"outer": outer, "red": red, "inner": inner, "P_new": P_new,
           "bytes": outer * red * inner * 2}
    samples = {n: [] for n in plans}
    reps = {}
    for name, plan in plans.items():          # warm up + size the window
        t = _sample(plan, stream, 3)
        reps[name] = max(3, int(sample_ms * 1e3 / (t * CALLS)))
    for _ in range(rounds):
        for name, plan in plans.items():
            samples[name].append(_sample(plan, stream, reps[name]))
    for name, s in samples.items():
        out[name] = {"median_us": round(statistics.median(s), 2),
                     "min_us": round(min(s), 2), "max_us": round(max(s), 2)}
    return out


VIEWS = [
    # outer, red, inner, splits tried
    # short rows (softmax-sized and hidden-sized), the handover sweep
    (65536, 128, 1, ()), (8192, 512, 1, ()), (8192, 768, 1, ()),
    (4096, 1024, 1, ()), (4096, 2048, 1, ()), (2048, 4096, 1, ()),
    (64, 1024, 1, ()), (64, 2048, 1, ()), (64, 4096, 1, ()),
    (1024, 8192, 1, ()), (8, 768, 1, ()),
    # long rows: where a split starts to pay, and how far it goes
    (1, 16384, 1, (2, 4)), (1, 32768, 1, (2, 4, 8)),
    (1, 65536, 1, (2, 4, 8, 16)), (64, 32768, 1, (2, 4, 8)),
    (64, 100000, 1, (2, 4, 8, 16, 32)), (8, 100000, 1, (8, 16, 32, 64)),
    (1, 100000, 1, (4, 8, 16, 32)), (1, 1000000, 1, (64, 128, 256)),
    (1, 4000000, 1, (128, 256, 512, 1024)),
    # NHWC global pools
    (64, 49, 2048, ()), (8, 49, 2048, ()), (1, 49, 2048, ()),
    (64, 196, 512, ()), (256, 49, 2048, ()),
    (1, 3136, 256, (4, 8, 16, 32)), (8, 16384, 64, (16, 32, 64)),
    (1, 65536, 64, (64, 256, 512)),
    # narrow inner
    (64, 4096, 8, (2, 4, 8)), (8, 16384, 16, (16, 32, 64)),
    (256, 512, 12, ()), (64, 128, 768, ()),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sample-ms", type=float, default=20.0)
    ap.add_argument("--out", default=None, help="also write JSON lines here")
    args = ap.parse_args()
    stream = torch.cuda.Stream()
    for outer, red, inner, splits in VIEWS:
        r = view_case(outer, red, inner, splits, args.rounds,
                      args.sample_ms, stream)
        print(json.dumps(r), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
