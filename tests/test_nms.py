"""CombinedNonMaxSuppression on the CPU side: planner lowering, the CPU
executor's definition against a plain float64 loop, and the calls the
emitter makes (TRANSPOSE, NMS select, top-k, NMS gather). The kernels are
pinned in test_gpu_nms.py, which shares reference_nms."""
import numpy as np
import pytest

from tfservingcache_amd.engine import emit
from tfservingcache_amd.engine.executor_cpu import combined_nms
from tfservingcache_amd.engine.planner import PlanError, compile_graph
from tfservingcache_amd.engine.savedmodel import GraphBuilder
from tfservingcache_amd.models import build_ssd_detector


def iou64(a, b):
    """IoU of boxes [..., 4] in float64, broadcast; area <= 0 gives 0."""
    lo_a, hi_a = np.minimum(a[..., :2], a[..., 2:]), np.maximum(a[..., :2],
                                                                a[..., 2:])
    lo_b, hi_b = np.minimum(b[..., :2], b[..., 2:]), np.maximum(b[..., :2],
                                                                b[..., 2:])
    area_a, area_b = np.prod(hi_a - lo_a, -1), np.prod(hi_b - lo_b, -1)
    inter = np.prod(np.clip(np.minimum(hi_a, hi_b) - np.maximum(lo_a, lo_b),
                            0, None), -1)
    ok = (area_a > 0) & (area_b > 0)
    return np.where(ok, inter / np.where(ok, area_a + area_b - inter, 1), 0)


def reference_nms(boxes, scores, P, M, iou_thr, score_thr, clip):
    """The issue's semantics as a float64 loop. Returns the four outputs."""
    boxes, scores = np.asarray(boxes, np.float64), np.asarray(scores,
                                                              np.float64)
    (nb, n, c), q = scores.shape, boxes.shape[2]
    out_b, out_s = np.zeros((nb, M, 4)), np.zeros((nb, M))
    out_c, valid = np.zeros((nb, M)), np.zeros(nb, np.int32)
    for b in range(nb):
        kept = []
        for cl in range(c):
            bx, s = boxes[b, :, 0 if q == 1 else cl], scores[b, :, cl]
            mine = []
            for i in sorted(np.flatnonzero(s > score_thr),
                            key=lambda i: (-s[i], i)):
                if len(mine) < P and not (iou64(bx[i], bx[mine])
                                          > iou_thr).any():
                    mine.append(i)
            kept += [(-s[i], cl, r, bx[i]) for r, i in enumerate(mine)]
        kept = sorted(kept, key=lambda e: e[:3])[:M]
        valid[b] = len(kept)
        for m, (ns, cl, _r, box) in enumerate(kept):
            out_b[b, m], out_s[b, m], out_c[b, m] = box, -ns, cl
    return (np.clip(out_b, 0, 1) if clip else out_b), out_s, out_c, valid


def _plan(boxes=(-1, 6, 1, 4), scores=(-1, 6, 3), per_class=2, total=4,
          iou=0.45, thr=0.25, dtype=np.float32, dynamic=None, **attrs):
    gb = GraphBuilder()
    consts = {"per_class": np.int32(per_class), "total": np.int32(total),
              "iou": np.float32(iou), "thr": np.float32(thr)}
    ins = [gb.placeholder("boxes", dtype, list(boxes)),
           gb.placeholder("scores", np.float32, list(scores))]
    ins += [gb.placeholder(k, v.dtype, []) if k == dynamic else
            gb.const(k, v) for k, v in consts.items()]
    nms = gb.node("CombinedNonMaxSuppression", "the_nms", ins, **attrs)
    for i in range(4):
        gb.mark_output(f"out{i}", f"{nms}:{i}")
    mg = gb.build().meta_graphs[0]
    return compile_graph(mg.graph_def,
                         next(iter(mg.signature_def.values())))


def test_fixture_plans_and_emits_the_four_calls():
    mg = build_ssd_detector(num_classes=3, max_per_class=10,
                            max_total=20).meta_graphs[0]
    plan = compile_graph(mg.graph_def,
                         next(iter(mg.signature_def.values())))
    op = plan.ops[-1]
    assert op.kind == "combined_nms" and len(op.outputs) == 4
    assert op.params == {"n": 160, "c": 3, "q": 1, "per_class": 10,
                         "max_total": 20, "iou_thr": float(np.float32(0.45)),
                         "score_thr": 0.5, "clip": True}
    outs = [plan.tensors[i] for i in op.outputs]
    assert [(t.shape, t.dtype) for t in outs] == [
        ((-1, 20, 4), "f32"), ((-1, 20), "f32"), ((-1, 20), "f32"),
        ((-1,), "i32")]
    assert "NMS" in emit.KINDS_NO_GOLDEN and "NMS" not in emit.KINDS
    tmpl = emit.build_template(plan, 8, "bf16")
    tr, sel, top, gat = tmpl.calls[-4:]
    assert [c[0] for c in (tr, sel, top, gat)] == [
        "TRANSPOSE", "NMS", "ARGMAX_LAST", "NMS"]
    assert tr[2] == [3, 8, 3, 160, 480, 1, 3, 8 * 3 * 160]
    assert sel[1][0] == tr[1][1] and sel[2] == [8, 160, 3, 1, 10]
    assert sel[3] == [float(np.float32(0.45)), 0.5]
    assert top[1][0] == sel[1][2] and top[2] == [8, 30, 20, 1]
    assert gat[1][:4] == [top[1][1], top[1][2], sel[1][3], sel[1][1]]
    assert gat[2] == [8, 160, 3, 1, 10, 20, 20, 1]
    # the scratch pieces are disjoint, 256-byte aligned and inside the arena
    offs = sorted([tr[1][1][1], sel[1][2][1], sel[1][3][1], top[1][1][1],
                   top[1][2][1]])
    assert all(o % 256 == 0 for o in offs) and len(set(offs)) == 5
    assert offs[-1] + 8 * 20 * 2 <= tmpl.total_bytes
    # one class: the scores are class-major as they are, no transpose
    one = emit.build_template(_plan(scores=(-1, 6, 1)), 2, "bf16").calls
    assert [c[0] for c in one] == ["NMS", "ARGMAX_LAST", "NMS"]


def test_pad_per_class_and_small_n_shape_the_outputs():
    plan = _plan(per_class=9, total=40, pad_per_class=GraphBuilder.a_bool(True),
                 clip_boxes=GraphBuilder.a_bool(False))
    p = plan.ops[-1].params
    assert (p["per_class"], p["max_total"], p["clip"]) == (6, 27, False)


@pytest.mark.parametrize("kwargs", [
    dict(dynamic="per_class"), dict(dynamic="total"), dict(dynamic="iou"),
    dict(dynamic="thr"), dict(scores=(-1, -1, 3)), dict(scores=(-1, 6, -1)),
    dict(boxes=(-1, 6, 1, 4), scores=(-1, 6, 257)), dict(thr=np.nan),
    dict(per_class=0), dict(total=0), dict(iou=1.5), dict(iou=-0.1),
    dict(boxes=(-1, 6, 2, 4)), dict(boxes=(-1, 6, 1, 5)), dict(dtype=np.int32),
    dict(boxes=(-1, 2 ** 19 + 1, 1, 4), scores=(-1, 2 ** 19 + 1, 3)),
    dict(boxes=(-1, 600, 1, 4), scores=(-1, 600, 3), per_class=400,
         total=2000)],
    ids=["dynamic-per-class", "dynamic-total", "dynamic-iou", "dynamic-thr",
         "symbolic-N", "symbolic-C", "C>256", "nan-thr", "per-class<1",
         "total<1", "iou>1", "iou<0", "q-not-1-or-C", "last-dim-5",
         "int-boxes", "N>2^19", "k>1024"])
def test_planner_refusals_name_the_node(kwargs):
    with pytest.raises(PlanError, match="the_nms"):
        _plan(**kwargs)


def test_cpu_executor_agrees_with_the_float64_loop():
    # class 0: a three-way score tie whose later members (a near copy and
    # the same box with swapped corners) are suppressed, cut at P = 2 with
    # candidates left; class 1: nothing above the threshold (0.25 is not
    # > 0.25); class 2: a zero-area box is kept and suppresses nothing, a
    # tie goes to the lower index, a kept box leaves [0, 1]
    boxes = np.array([[0.1, 0.1, 0.5, 0.5], [0.12, 0.1, 0.5, 0.52],
                      [0.5, 0.5, 0.1, 0.1], [0.6, 0.6, 0.9, 0.9],
                      [0.3, 0.3, 0.3, 0.7], [-0.2, 0.7, 0.2, 1.3],
                      [0.62, 0.6, 0.9, 0.9], [0.0, 0.0, 0.05, 0.05]],
                     np.float32).reshape(1, 8, 1, 4)
    scores = np.array([[0.9, 0.9, 0.9, 0.8, 0.8, 0.8, 0.7, 0.6],
                       [0.1, 0.25, 0.2, 0.0, 0.1, 0.25, 0.0, 0.2],
                       [0.3, 0.0, 0.0, 0.0, 0.9, 0.9, 0.0, 0.8]],
                      np.float32).T.reshape(1, 8, 3)
    for clip in (True, False):
        got = combined_nms(boxes, scores, 2, 5, 0.45, 0.25, clip)
        want = reference_nms(boxes, scores, 2, 5, 0.45, 0.25, clip)
        for g_, w_ in zip(got, want):
            np.testing.assert_array_equal(g_, w_.astype(g_.dtype))
        assert got[3].dtype == np.int32 and got[3].tolist() == [4]
        np.testing.assert_array_equal(got[2][0], [0, 2, 2, 0, 0])
        np.testing.assert_array_equal(
            got[0][0, 2], np.float32([0, 0.7, 0.2, 1] if clip
                                     else [-0.2, 0.7, 0.2, 1.3]))
