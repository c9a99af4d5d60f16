"""Timing probe for the NMS select kernel (profiles/nms.md).

Each variant is one ExecPlan of CALLS identical K_NMS select calls on
fixed device buffers, captured into a hipGraph. A sample is the wall time
of n back-to-back replays ending in one device synchronise, over
n * CALLS: time per launch, graph-launch cost amortised over CALLS. The
variants of a shape alternate, `--rounds` samples each, reported as median
(min - max); n is sized so a sample lasts about `--sample-ms`.

Part 1, detector shapes (N boxes, C classes, q = 1, P = 100 per class) at
B = 1 and 8: `few` is a score threshold of 0.3 over detector-like scores
(sigmoid of N(-4, 1.5): about 1 % of the boxes are candidates), `all` a
threshold of -inf (every box is one). The default cap decides the
geometry; the candidate count of the fullest class is reported. Each is
also timed with the cap at 8192, the largest the LDS allows.

Part 2, the cap: B = 8, C = 80, N = 25200 with exactly `cand` candidates in
every class, timed with the cap at 8192 (resident) and at 1 (streamed) on
the same input; the two results are compared before timing.

Boxes: 40 objects per image, each box a jittered copy of one of them, so
suppression does what it does on a detector's output.

    python scripts/nms_probe.py [--rounds 5] [--out FILE]
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

CALLS = 10
P = 100
IOU_THR = 0.5


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


def _boxes(B, N, g):
    obj = torch.rand(B, 40, 2, generator=g) * 0.8 + 0.1
    pick = torch.randint(0, 40, (B, N), generator=g)
    centre = torch.gather(obj, 1, pick[..., None].expand(B, N, 2))
    centre = centre + torch.randn(B, N, 2, generator=g) * 0.03
    half = 0.08 + torch.rand(B, N, 2, generator=g) * 0.06
    return torch.cat([centre - half, centre + half], -1).reshape(B, N, 1, 4)


def _select(scores_cm, boxes, cap, thr, stream):
    """(plan, cls_score, cls_idx) of one select call under LDS cap `cap`;
    the cap is read at launch, so it is set around run and capture."""
    B, C, N = scores_cm.shape
    cls_score = torch.zeros(B * C * P, dtype=torch.bfloat16, device="cuda")
    cls_idx = torch.zeros(B * C * P, dtype=torch.int32, device="cuda")
    default = ext.nms_lds_candidates()
    ext.set_nms_lds_candidates(cap)
    try:
        plan = _graph((ext.K_NMS, [scores_cm.data_ptr(), boxes.data_ptr(),
                                   cls_score.data_ptr(), cls_idx.data_ptr()],
                       [B, N, C, 1, min(P, N)], [IOU_THR, thr]), stream)
    finally:
        ext.set_nms_lds_candidates(default)
    return plan, cls_score, cls_idx


def _time(plans, rounds, sample_ms, stream):
    reps = {}
    for name, plan in plans.items():          # warm up + size the window
        t = _sample(plan, stream, 3)
        reps[name] = max(3, int(sample_ms * 1e3 / (t * CALLS)))
    samples = {n: [] for n in plans}
    for _ in range(rounds):
        for name, plan in plans.items():
            samples[name].append(_sample(plan, stream, reps[name]))
    return {name: {"median_us": round(statistics.median(s), 2),
                   "min_us": round(min(s), 2), "max_us": round(max(s), 2),
                   "replays": reps[name]} for name, s in samples.items()}


def detector_case(name, B, N, C, rounds, sample_ms, stream):
    g = torch.Generator().manual_seed(N + C + B)
    scores = torch.sigmoid(torch.randn(B, C, N, generator=g) * 1.5 - 4.0)
    scores = scores.to(torch.bfloat16)
    boxes = _boxes(B, N, g).to(torch.bfloat16).cuda()
    cap = ext.nms_lds_candidates()
    plans = {}
    out = {"part": "detector", "shape": name, "B": B, "N": N, "C": C, "P": P,
           "cap": cap, "calls_per_graph": CALLS}
    sd = scores.cuda()
    for tag, thr in (("few", 0.3), ("all", float("-inf"))):
        most = int((scores.float() > thr).sum(-1).max())
        out[f"{tag}_candidates"] = most
        out[f"{tag}_geometry"] = "resident" if most <= cap else "streamed"
        plans[tag] = _select(sd, boxes, cap, thr, stream)[0]
        # the largest cap: 128 KB of LDS when N >= 8192, one workgroup a CU
        plans[f"{tag}_cap8192"] = _select(sd, boxes, 8192, thr, stream)[0]
    out.update(_time(plans, rounds, sample_ms, stream))
    return out


def cap_case(cand, rounds, sample_ms, stream, B=8, C=80, N=25200):
    g = torch.Generator().manual_seed(cand)
    rank = torch.rand(B, C, N, generator=g).argsort(-1).argsort(-1)
    scores = torch.where(rank < cand,
                         0.5 + 0.5 * torch.rand(B, C, N, generator=g),
                         torch.tensor(0.01)).to(torch.bfloat16).cuda()
    boxes = _boxes(B, N, g).to(torch.bfloat16).cuda()
    res = _select(scores, boxes, 8192, 0.3, stream)
    stm = _select(scores, boxes, 1, 0.3, stream)
    torch.cuda.synchronize()
    if not (torch.equal(res[1], stm[1]) and torch.equal(res[2], stm[2])):
        raise SystemExit(f"cand={cand}: resident and streamed disagree")
    out = {"part": "cap", "B": B, "N": N, "C": C, "P": P, "candidates": cand,
           "calls_per_graph": CALLS}
    out.update(_time({"resident": res[0], "streamed": stm[0]}, rounds,
                     sample_ms, stream))
    return out


DETECTORS = [("ssd", 1917, 90), ("yolo", 25200, 80),
             ("efficientdet", 49104, 90)]
CAP_CANDIDATES = [256, 1024, 2048, 4096, 8192]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sample-ms", type=float, default=30.0)
    ap.add_argument("--out", default=None, help="also write JSON lines here")
    args = ap.parse_args()
    stream = torch.cuda.Stream()

    def report(r):
        print(json.dumps(r), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(r) + "\n")

    for name, N, C in DETECTORS:
        for B in (1, 8):
            report(detector_case(name, B, N, C, args.rounds, args.sample_ms,
                                 stream))
    for cand in CAP_CANDIDATES:
        report(cap_case(cand, args.rounds, args.sample_ms, stream))


if __name__ == "__main__":
    main()
