"""The NMS kernels of ops/nms.hip, called as the emitter calls them
(TRANSPOSE, K_NMS select, top-k, K_NMS gather in one ExecPlan), and
CombinedNonMaxSuppression through build_ssd_detector. Harness as in
test_gpu_topk.py: outputs and scratch pre-filled with a sentinel, 64 guard
elements behind. Reference: test_nms.reference_nms, a float64 loop, on the
bf16-rounded inputs; all four outputs exactly equal.

Cases: the product of N, (C, q) and P <= N; B, M below / above C*P,
pad_per_class and clip cycle through their 16 combinations along it. M
above C*P needs C*P <= 1024 (the top-k bound); pad_per_class caps M at
C*P. Every N >= 257 case runs again with the LDS cap at 64, below the
scene's candidate counts: the streamed geometry. Before any launch a case
asserts on the reference that no same-class candidate pair has an IoU
within 1e-6 of the threshold (the kernel's f32 quotient is off by ~3e-8)
and, for N >= 63, that some class loses a third of its candidates to
suppression; N = 1 has no pair to suppress.
"""
import functools
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

from test_nms import iou64, reference_nms  # noqa: E402
from tfservingcache_amd.engine import _tfsc_engine as ext  # noqa: E402
from tfservingcache_amd.engine import emit  # noqa: E402
from tfservingcache_amd.engine.executor_cpu import combined_nms  # noqa: E402
from tfservingcache_amd.engine.model import (  # noqa: E402
    load_model_from_dir)
from tfservingcache_amd.engine.savedmodel import (  # noqa: E402
    write_saved_model)
from tfservingcache_amd.models import build_ssd_detector  # noqa: E402

SENTINEL, SENTINEL_INT, TAIL = 1.0e30, 0x7F7F7F7F, 64
GRID_CAP = 2048                 # blocks per launch, both kernels
LDS_CAP = 4096                  # ext.nms_lds_candidates(), asserted below
IOU_THR, SCORE_THR = 0.45, 0.25


# Boxes live on a grid of 1/128, exact in bf16 up to 2.0, so an IoU is a
# ratio of integers, inter / union. 9/20 needs 29 | area_a + area_b; every
# size below has h * w % 29 == 5, so no pair has IoU 0.45, and the nearest
# ratio is 1 / (20 * union) > 2e-5 away.
GRID = 128.0
SIZES = np.array([(h, w) for h in range(20, 32) for w in range(20, 32)
                  if h * w % 29 == 5])


@functools.lru_cache(maxsize=None)
def _scene(B, N, C, q, jitter=6):
    """bf16 boxes jittered around five corners (a tenth with swapped
    corners, a few of zero area, a few pushed below 0 or past 1) and scores
    on a grid of sixteenths, so ties are everywhere (box 0 of class 0 is
    always a candidate); then _preconditions."""
    rng = np.random.default_rng(1000 * N + 10 * C + q + B)
    lo = rng.integers(10, 81, (5, 2))[rng.integers(0, 5, (B, N, q))]
    lo = lo + rng.integers(-jitter, jitter + 1, (B, N, q, 2))
    boxes = np.concatenate(
        [lo, lo + SIZES[rng.integers(0, len(SIZES), (B, N, q))]], -1) / GRID
    kind = rng.integers(0, 40, (B, N, q))
    boxes[kind < 4] = boxes[kind < 4][:, [2, 3, 0, 1]]
    boxes[kind == 4, 2] = boxes[kind == 4, 0]
    boxes[kind == 5] += 0.5
    boxes[kind == 6] -= 0.25
    scores = rng.integers(0, 17, (B, N, C)) / 16.0
    scores[:, 0, 0] = 1.0
    boxes = torch.tensor(boxes, dtype=torch.float32).to(torch.bfloat16)
    scores = torch.tensor(scores, dtype=torch.float32).to(torch.bfloat16)
    return (boxes, scores) + _preconditions(boxes, scores)


def _preconditions(boxes, scores):
    """Over all (image, class): a candidate pair's least |IoU - threshold|,
    the largest share of candidates suppressed, the most candidates."""
    b64, s64 = boxes.double().numpy(), scores.double().numpy()
    (B, N, C), q = s64.shape, b64.shape[2]
    margin, lost, most = 1.0, 0.0, 0
    for b, cl in itertools.product(range(B), range(C)):
        cand = np.flatnonzero(s64[b, :, cl] > SCORE_THR)
        if cand.size == 0:
            continue
        bx = b64[b, cand, 0 if q == 1 else cl]
        uniq = np.unique(bx, axis=0)         # the same set of pair IoUs
        margin = min(margin, np.abs(iou64(uniq[:, None], uniq[None]) -
                                    IOU_THR).min())
        kept = reference_nms(bx[None, :, None], s64[b, cand, cl][None, :, None],
                             N, N, IOU_THR, SCORE_THR, False)[3][0]
        lost = max(lost, 1 - kept / cand.size)
        most = max(most, cand.size)
    return margin, lost, most


def _filled(n, dtype):
    return torch.full((n + TAIL,), SENTINEL_INT if dtype in (
        torch.int32, torch.int64) else SENTINEL, dtype=dtype, device="cuda")


def _check_nms(boxes, scores, P, M, clip, what):
    (B, N, C), q = scores.shape, boxes.shape[2]
    slots, k = C * P, min(M, C * P)
    seg = emit.topk_segments(B, slots, k)
    bf, i32 = torch.bfloat16, torch.int32
    bufs = {"scm": _filled(B * C * N if C > 1 else 0, bf),
            "cls_score": _filled(B * slots, bf),
            "cls_idx": _filled(B * slots, i32),
            "slot": _filled(B * k, i32), "val": _filled(B * k, bf),
            "part": _filled(B * seg * k if seg > 1 else 0, torch.int64),
            "boxes": _filled(B * M * 4, bf), "scores": _filled(B * M, bf),
            "classes": _filled(B * M, bf), "valid": _filled(B, i32)}
    used = {n_: t.numel() - TAIL for n_, t in bufs.items()}
    ptr = {n_: t.data_ptr() for n_, t in bufs.items()}
    bd, sd = boxes.contiguous().cuda(), scores.contiguous().cuda()
    calls = []
    if C > 1:
        calls.append((ext.K_TRANSPOSE, [sd.data_ptr(), ptr["scm"]],
                      [3, B, C, N, N * C, 1, C, B * C * N], []))
    calls += [
        (ext.K_NMS, [ptr["scm"] if C > 1 else sd.data_ptr(), bd.data_ptr(),
                     ptr["cls_score"], ptr["cls_idx"]], [B, N, C, q, P],
         [IOU_THR, SCORE_THR]),
        (ext.K_ARGMAX_LAST, [ptr["cls_score"], ptr["slot"], ptr["val"],
                             ptr["part"] if seg > 1 else 0],
         [B, slots, k, seg], []),
        (ext.K_NMS, [ptr["slot"], ptr["val"], ptr["cls_idx"], bd.data_ptr(),
                     ptr["boxes"], ptr["scores"], ptr["classes"],
                     ptr["valid"]], [B, N, C, q, P, k, M, int(clip)], [])]
    ext.ExecPlan(calls).run()
    torch.cuda.synchronize()
    for name, buf in bufs.items():
        tail = buf[used[name]:].cpu()
        assert (tail == tail.new_tensor(
            SENTINEL if buf.dtype == bf else SENTINEL_INT)).all(), \
            f"wrote past the end of {name}, {what}"
    want = reference_nms(boxes.double().numpy(), scores.double().numpy(), P,
                         M, np.float32(IOU_THR), np.float32(SCORE_THR), clip)
    shapes = {"boxes": (B, M, 4), "scores": (B, M), "classes": (B, M),
              "valid": (B,)}
    for (name, shape), w in zip(shapes.items(), want):
        got = bufs[name][:used[name]].cpu().double().numpy().reshape(shape)
        bad = np.argwhere(got != w)
        print(f"{what}: {len(bad)} of {got.size} {name} differ")
        assert len(bad) == 0, (what, name, bad[:4].tolist(),
                               got[tuple(bad[0])], w[tuple(bad[0])])


def _cases():
    combos = list(itertools.product((1, 3), (False, True), (False, True),
                                    (True, False)))
    grid = itertools.product((1, 63, 257, 1000), ((1, 1), (3, 1), (3, 3)),
                             (1, 5, None))
    grid = [(N, cq, P) for N, cq, P in grid if N > 1 or P == 1]   # P <= N
    for i, (N, (C, q), P) in enumerate(grid):
        B, above, pad, clip = combos[i % len(combos)]
        P = min(P or N, N)
        slots = C * P
        M = slots + 3 if above and slots <= 1024 else \
            max(1, min(slots // 2, 1000))
        M = min(M, slots) if pad else M
        for cap in (LDS_CAP, 64) if N >= 257 else (LDS_CAP,):
            yield pytest.param(B, N, C, q, P, M, clip, cap,
                               id=f"B{B}-N{N}-C{C}-q{q}-P{P}-M{M}-"
                                  f"clip{int(clip)}-cap{cap}")


@pytest.mark.parametrize("B,N,C,q,P,M,clip,cap", list(_cases()))
def test_nms_against_the_float64_loop(B, N, C, q, P, M, clip, cap):
    boxes, scores, margin, lost, most = _scene(B, N, C, q)
    print(f"margin {margin:.3g}, suppressed {lost:.2f}, candidates {most}")
    assert margin > 1e-6
    assert N < 63 or lost >= 1 / 3
    assert cap == LDS_CAP or most > cap          # really streamed
    assert ext.nms_lds_candidates() == LDS_CAP
    try:
        ext.set_nms_lds_candidates(cap)
        _check_nms(boxes, scores, P, M, clip, f"nms cap={cap}")
    finally:
        ext.set_nms_lds_candidates(LDS_CAP)


@pytest.mark.parametrize("extra", [0, 1])
def test_nms_at_the_default_lds_cap(extra):
    # LDS_CAP candidates run resident in 64 KB of LDS, one more streams
    boxes, scores, *_ = _scene(1, LDS_CAP + 8, 1, 1, 2)
    scores = scores.clone()
    scores[0, :, 0] = torch.where(scores[0, :, 0] > SCORE_THR,
                                  scores[0, :, 0], 0.5)
    scores[0, 7:15 - extra, 0] = 0.0
    margin, lost, most = _preconditions(boxes, scores)
    assert most == LDS_CAP + extra and margin > 1e-6 and lost >= 1 / 3
    assert ext.nms_lds_candidates() == LDS_CAP
    _check_nms(boxes, scores, 5, 8, True, f"nms {LDS_CAP + extra} candidates")


@pytest.mark.parametrize("B,C", [(GRID_CAP // 3 + 18, 3), (GRID_CAP + 3, 1)])
def test_nms_rows_past_the_grid_cap(B, C):
    # B * C past the cap loops k_nms_select's rows, B past it k_nms_gather's
    boxes, scores, margin, _lost, _most = _scene(B, 8, C, 1)
    assert B * C > GRID_CAP and margin > 1e-6
    _check_nms(boxes, scores, 3, 5, True, f"nms [{B},8,{C}]")


def test_nms_special_images():
    # image 0: all scores equal, boxes apart; image 1: all scores at or
    # below the threshold; image 2: all boxes identical
    N, C = 63, 3
    boxes, scores, *_ = _scene(3, N, C, 1)
    boxes, scores = boxes.clone(), scores.clone()
    grid = torch.arange(N, dtype=torch.float32)
    y, x = (grid // 8) / 8, (grid % 8) / 8
    boxes[0, :, 0] = torch.stack([y, x, y + 0.1, x + 0.1], -1).to(
        torch.bfloat16)
    scores[0] = 0.75
    scores[1, :, 0], scores[1, :, 1:] = SCORE_THR, 0.125
    boxes[2] = boxes[2, 0]
    for P, M in ((5, 20), (N, 200)):
        _check_nms(boxes, scores, P, M, True, f"nms special P={P} M={M}")


def test_launcher_refuses_before_any_launch():
    buf = torch.zeros(4096, dtype=torch.int64, device="cuda")
    p = buf.data_ptr()
    sel, gat = [p] * 4, [p] * 8
    for ints, floats, ptrs in (
            ([2, 0, 3, 1, 1], [0.5, 0.0], sel),               # N < 1
            ([2, 2 ** 19 + 1, 3, 1, 1], [0.5, 0.0], sel),     # N > 2^19
            ([2, 16, 3, 2, 4], [0.5, 0.0], sel),              # q not 1 or C
            ([2, 16, 3, 1, 17], [0.5, 0.0], sel),             # P > N
            ([2, 16, 3, 1, 0], [0.5, 0.0], sel),              # P < 1
            ([2, 16, 3, 1, 4], [1.5, 0.0], sel),              # iou > 1
            ([2, 16, 3, 1, 4], [0.5, 0.0], [p, p + 2, p, p]),  # alignment
            ([2, 16, 3, 1, 4], [0.5, 0.0], [p, p, 0, p]),     # null pointer
            ([2, 16, 3, 1, 4, 13, 20, 1], [], gat),           # k > C * P
            ([2, 16, 3, 1, 4, 5, 4, 1], [], gat),             # k > M
            ([2, 16, 3, 1, 4, 5, 8, 2], [], gat),             # clip
            ([2, 16, 3, 1, 4, 5, 8], [], gat)):               # form
        with pytest.raises(RuntimeError, match="nms"):
            ext.ExecPlan([(ext.K_NMS, ptrs, ints, floats)]).run()
    torch.cuda.synchronize()
    assert int(buf.abs().sum()) == 0


GEMM_RTOL, GEMM_ATOL = 0.05, 0.02       # test_mlp_gpu_vs_cpu


def test_ssd_detector_predict_and_fast_path(tmp_path):
    # eager, hipGraph replay, C++ fast path; the expectation is the CPU
    # definition applied to the GPU's own boxes and scores
    from tfservingcache_amd.engine.gpu import GpuModel
    from tfservingcache_amd.wire import messages as m
    from tfservingcache_amd.wire.tensor import (numpy_to_tensorproto,
                                                tensorproto_to_numpy)
    P, M = 10, 20
    sm = build_ssd_detector(max_per_class=P, max_total=M, seed=3)
    d = str(tmp_path / "ssd" / "1")
    write_saved_model(sm, d)
    cm = load_model_from_dir(d, "ssd", 1)
    gm = load_model_from_dir(d, "ssd", 1)
    gm._gpu = GpuModel(gm.plan, device="cuda:0", max_batch=8,
                       model_name="ssd", model_version=1)
    try:
        par = gm.plan.ops[-1].params
        assert gm.plan.ops[-1].kind == "combined_nms"
        x = np.random.default_rng(5).standard_normal(
            (5, 64, 64, 3)).astype(np.float32) * 0.5
        for batch in (1, 5):                        # 5 -> bucket 8
            feeds = {"input": x[:batch]}
            want = cm.predict(feeds)
            outs = {"predict": gm.predict(feeds),
                    "replay": gm.predict(feeds)}
            req = m.PredictRequest(
                model_spec=m.ModelSpec(name="ssd",
                                       version=m.Int64Value(value=1)),
                inputs={"input": numpy_to_tensorproto(x[:batch])}).encode()
            resp = m.PredictResponse.decode(gm._gpu.fast_predict(req))
            outs["fast"] = {a: tensorproto_to_numpy(t)
                            for a, t in resp.outputs.items()}
            for path, got in outs.items():
                what = f"{path} batch {batch}"
                exp = combined_nms(got["boxes"], got["scores"], P, M,
                                   par["iou_thr"], par["score_thr"], True)
                assert got["valid_detections"].dtype == np.int32, what
                assert got["nmsed_boxes"].shape == (batch, M, 4), what
                assert exp[3].min() > 0, what
                for alias, e in zip(("nmsed_boxes", "nmsed_scores",
                                     "nmsed_classes", "valid_detections"),
                                    exp):
                    assert got[alias].shape == e.shape, (what, alias)
                    np.testing.assert_array_equal(got[alias], e,
                                                  f"{what} {alias}")
                for alias in ("boxes", "scores"):
                    np.testing.assert_allclose(
                        got[alias], want[alias], rtol=GEMM_RTOL,
                        atol=GEMM_ATOL, err_msg=f"{what} {alias}")
    finally:
        gm._gpu.release()
