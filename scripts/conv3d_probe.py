"""Timing probe for 3-D convolution (profiles/conv3d.md).

1. Cost of the 3-D gather: CONV's 23-int form with T = D = 1 against the
   15-int 2-D kernel on the identical problem (3x3 SAME, fused relu). The
   MFMA work is the same, so the ratio is what the three-axis gather and
   the f32-staged epilogue cost (or save). The two outputs are compared:
   they may differ by the 2-D epilogue's extra rounding only.
2. Per-layer time and TFLOP/s of build_video_resnet's conv shapes at
   I3D-like sizes (16 frames of 112x112 after the stem's spatial stride),
   batch 1 and 8, one K_CONV call each.

One process. A figure is the wall time of n back-to-back hipGraph replays
ending in one device synchronise, divided by n, with n sized so a sample
lasts about 0.2 s; the variants of a case alternate, five samples each,
reported as median (min - max).

    python scripts/conv3d_probe.py [--rounds 5] [--out FILE]
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

DEV = "cuda:0"
BF = torch.bfloat16


def _pad64(k):
    return (k + 63) // 64 * 64


def _same(size, k, s):
    out = -(-size // s)
    return out, max((out - 1) * s + k - size, 0) // 2


def _time_replays(replay, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6      # us per replay


def _captured(ptrs, ints, stream):
    """One K_CONV call, run eagerly once and captured into a hipGraph."""
    plan = ext.ExecPlan([(ext.K_CONV, ptrs, ints, [])])
    with torch.cuda.stream(stream):
        plan.run()
        torch.cuda.synchronize()
        plan.capture()
        for _ in range(20):
            plan.run_graph()
        torch.cuda.synchronize()
    return plan


def _alternate(plans, stream, rounds):
    samples = {n: [] for n in plans}
    with torch.cuda.stream(stream):
        n_rep = {n: max(20, min(20000, int(2e5 / _time_replays(p.run_graph,
                                                                20))))
                 for n, p in plans.items()}
        for _ in range(rounds):
            for name, plan in plans.items():
                samples[name].append(_time_replays(plan.run_graph,
                                                   n_rep[name]))
    return {n: {"median_us": round(statistics.median(s), 2),
                "min_us": round(min(s), 2), "max_us": round(max(s), 2),
                "replays": n_rep[n], "rounds": len(s)}
            for n, s in samples.items()}


def _problem(N, dhw, C, K, trs, stride):
    """Device tensors and the 23-int form of one SAME conv with relu."""
    g = torch.Generator().manual_seed(0)
    trsc = trs[0] * trs[1] * trs[2] * C
    x = torch.randn(N, *dhw, C, generator=g).to(BF).to(DEV)
    w = torch.zeros(K, _pad64(trsc), dtype=BF)
    w[:, :trsc] = (torch.randn(K, trsc, generator=g) * 0.05).to(BF)
    w = w.to(DEV)
    b = torch.zeros(_pad64(K) * 2, dtype=BF, device=DEV)
    zeros = torch.zeros(64, dtype=BF, device=DEV)
    (Do, pf), (Ho, pt), (Wo, pl) = (_same(n, k, s) for n, k, s in
                                    zip(dhw, trs, stride))
    ints = [N, dhw[1], dhw[2], C, K, trs[1], trs[2], stride[1], stride[2],
            pt, pl, Ho, Wo, _pad64(trsc), 1, 1, 1, 1, dhw[0], trs[0],
            stride[0], pf, Do]
    M = N * Do * Ho * Wo

    def ptrs(y):
        return [x.data_ptr(), w.data_ptr(), b.data_ptr(), 0,
                zeros.data_ptr(), y.data_ptr()]

    keep = (x, w, b, zeros)
    return ptrs, ints, M, 2.0 * M * K * trsc, keep


def gather_cost(N, H, C, K, stream, rounds):
    ptrs, ints, M, flop, keep = _problem(N, (1, H, H), C, K, (1, 3, 3),
                                         (1, 1, 1))
    ys = {n: torch.empty(M * K, dtype=BF, device=DEV)
          for n in ("conv3d_T1", "conv2d")}
    plans = {"conv3d_T1": _captured(ptrs(ys["conv3d_T1"]), ints, stream),
             "conv2d": _captured(ptrs(ys["conv2d"]), ints[:15], stream)}
    res = _alternate(plans, stream, rounds)
    torch.cuda.synchronize()
    a, b = ys["conv3d_T1"].float(), ys["conv2d"].float()
    return {"case": f"[{N},{H},{H},{C}]->{K} 3x3", **res,
            "ratio_3d_over_2d": round(res["conv3d_T1"]["median_us"] /
                                      res["conv2d"]["median_us"], 4),
            "max_abs_diff": float((a - b).abs().max()),
            "max_abs_out": float(b.abs().max()),
            "tflops_2d": round(flop / res["conv2d"]["median_us"] / 1e6, 1)}


# build_video_resnet's conv shapes at I3D-like sizes:
# (name, (D,H,W), C, K, (T,R,S), strides); the stem's C is the widened 8
_LAYERS = [
    ("stem 3x7x7/(1,2,2)", (16, 112, 112), 8, 64, (3, 7, 7), (1, 2, 2)),
    ("3x3x3", (16, 28, 28), 64, 64, (3, 3, 3), (1, 1, 1)),
    ("(2+1)D 1x3x3", (16, 28, 28), 64, 64, (1, 3, 3), (1, 1, 1)),
    ("(2+1)D 3x1x1", (16, 28, 28), 64, 64, (3, 1, 1), (1, 1, 1)),
    ("3x3x3/2", (16, 28, 28), 64, 128, (3, 3, 3), (2, 2, 2)),
    ("1x1x1/2 shortcut", (16, 28, 28), 64, 128, (1, 1, 1), (2, 2, 2)),
    ("3x3x3 mid", (8, 14, 14), 128, 128, (3, 3, 3), (1, 1, 1)),
    ("3x3x3 late", (2, 7, 7), 512, 512, (3, 3, 3), (1, 1, 1)),
]


def layer(name, dhw, C, K, trs, stride, N, stream, rounds):
    ptrs, ints, M, flop, keep = _problem(N, dhw, C, K, trs, stride)
    y = torch.empty(M * K, dtype=BF, device=DEV)
    res = _alternate({"t": _captured(ptrs(y), ints, stream)}, stream,
                     rounds)["t"]
    return {"layer": name, "batch": N, "in": [N, *dhw, C], "K": K, "M": M,
            "blocks": -(-M // 128) * -(-K // 128), **res,
            "tflops": round(flop / res["median_us"] / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv3d_probe needs a GPU")
    stream = torch.cuda.Stream()
    out = {"gather_cost": [], "layers": []}
    for N, H, C, K in ((8, 56, 64, 64), (8, 28, 128, 128), (8, 14, 256, 256),
                       (8, 56, 24, 64)):
        out["gather_cost"].append(gather_cost(N, H, C, K, stream,
                                              args.rounds))
        print(json.dumps(out["gather_cost"][-1]), flush=True)
    for N in (1, 8):
        for spec in _LAYERS:
            out["layers"].append(layer(*spec, N, stream, args.rounds))
            print(json.dumps(out["layers"][-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
