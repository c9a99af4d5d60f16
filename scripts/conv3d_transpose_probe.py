"""Timing probe for the 3-D transposed conv (profiles/conv3d_transpose.md).

The phase-split kernel (CONV's 24-int form) against the zero-insert
recipe's conv step: conv3d_igemm_kernel (23-int form, stride 1) with the
flipped, in/out-swapped filter on an input whose zeros were inserted
OUTSIDE the timed region. The project has no 3-D zero-insert pass, so the
baseline gets it for free. The two outputs are compared on the same bf16
values: they differ by accumulation order only.

Shapes: build_unet3d's up-steps at V-Net-like sizes, 3x3x3/2 SAME and
2x2x2/2 each, batch 1 and 8, fused relu.

One process. A figure is the wall time of n back-to-back hipGraph replays
ending in one device synchronise, divided by n, with n sized so a sample
lasts about 0.2 s; the two variants alternate, five samples each, reported
as median (min - max).

    python scripts/conv3d_transpose_probe.py [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch  # noqa: E402

from conv3d_probe import BF, DEV, _alternate, _captured, _pad64  # noqa: E402
from tfservingcache_amd.engine.planner import (  # noqa: E402
    conv3d_transpose_phases, conv3d_transpose_taps)


def case(N, dhw, C, K, k, stream, rounds):
    """One k x k x k / 2 up-step [N,*dhw,C] -> [N,*2*dhw,K], both ways."""
    g = torch.Generator().manual_seed(0)
    trs, stride = (k, k, k), (2, 2, 2)
    out = tuple(2 * n for n in dhw)
    pad = max((dhw[0] - 1) * 2 + k - out[0], 0) // 2       # SAME, low side
    x = torch.randn(N, *dhw, C, generator=g).to(BF)
    w = (torch.randn(k, k, k, K, C, generator=g) * 0.05).to(BF)
    b = torch.zeros(_pad64(K) * 2, dtype=BF, device=DEV)
    zeros = torch.zeros(64, dtype=BF, device=DEV)

    # phase-split: taps in the kernel's order
    kp = _pad64(conv3d_transpose_taps(trs, stride, C) * C)
    wt = torch.zeros(K, kp, dtype=BF)
    for _phase, taps, first in conv3d_transpose_phases(trs, stride):
        for i, (t, r, s) in enumerate(taps):
            wt[:, (first + i) * C:(first + i + 1) * C] = w[t, r, s]
    # baseline: zero-inserted x, flipped filter [K][(t,r,s,c)], stride 1;
    # low pad k-1-pad, the high pad is whatever yields `out`
    z = torch.zeros(N, *(2 * n - 1 for n in dhw), C, dtype=BF)
    z[:, ::2, ::2, ::2] = x
    kz = _pad64(k ** 3 * C)
    wz = torch.zeros(K, kz, dtype=BF)
    wz[:, :k ** 3 * C] = w.flip(0, 1, 2).permute(3, 0, 1, 2, 4).reshape(K, -1)

    M = N * out[0] * out[1] * out[2]
    dev = [t.to(DEV) for t in (x, wt, z, wz)]
    ys = {n: torch.empty(M * K, dtype=BF, device=DEV)
          for n in ("phase_split", "zero_insert_conv")}

    def ptrs(xin, win, y):
        return [xin.data_ptr(), win.data_ptr(), b.data_ptr(), 0,
                zeros.data_ptr(), y.data_ptr()]

    ints_t = [N, dhw[1], dhw[2], C, K, k, k, 2, 2, pad, pad, out[1], out[2],
              kp, 1, 1, 1, 1, dhw[0], k, 2, pad, out[0], 1]
    lo = k - 1 - pad
    ints_z = [N, 2 * dhw[1] - 1, 2 * dhw[2] - 1, C, K, k, k, 1, 1, lo, lo,
              out[1], out[2], kz, 1, 1, 1, 1, 2 * dhw[0] - 1, k, 1, lo,
              out[0]]
    plans = {
        "phase_split": _captured(ptrs(dev[0], dev[1], ys["phase_split"]),
                                 ints_t, stream),
        "zero_insert_conv": _captured(
            ptrs(dev[2], dev[3], ys["zero_insert_conv"]), ints_z, stream)}
    res = _alternate(plans, stream, rounds)
    torch.cuda.synchronize()
    a, c = (ys[n].float() for n in ("phase_split", "zero_insert_conv"))
    # the multiply-adds no zero takes part in: every x voxel meets every tap
    flop = 2.0 * N * dhw[0] * dhw[1] * dhw[2] * k ** 3 * C * K
    return {"case": f"[{N},{dhw[0]},{dhw[1]},{dhw[2]},{C}]->{K} {k}x{k}x{k}/2",
            **res,
            "ratio_split_over_baseline": round(
                res["phase_split"]["median_us"] /
                res["zero_insert_conv"]["median_us"], 4),
            "blocks_split": 8 * -(-(N * (out[0] // 2) * (out[1] // 2) *
                                    (out[2] // 2)) // 128) * -(-K // 128),
            "blocks_baseline": -(-M // 128) * -(-K // 128),
            "useful_tflops_split": round(
                flop / res["phase_split"]["median_us"] / 1e6, 1),
            "max_abs_diff": float((a - c).abs().max()),
            "max_abs_out": float(c.abs().max())}


# build_unet3d's up-steps at V-Net-like sizes: ((D,H,W), C, K)
_SHAPES = [((8, 8, 8), 256, 128), ((16, 16, 16), 128, 64)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv3d_transpose_probe needs a GPU")
    stream = torch.cuda.Stream()
    out = []
    for N in (1, 8):
        for dhw, C, K in _SHAPES:
            for k in (3, 2):
                out.append(case(N, dhw, C, K, k, stream, args.rounds))
                print(json.dumps(out[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
