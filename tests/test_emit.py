"""Call emission (engine/emit.py) on CPU.

tests/golden/call_templates/<case>.json hold the call templates the
engine registered on an MI355X at commit db6ee08, when the template was
still recovered from emitted device addresses: the `tcalls` handed to
ext.CallTemplate (region indices resolved to keys, kinds by name), the
region keys, workspace size, scratch and buffer offsets, and the master
blob slots of `_upload_weights`, for buckets 1 and 4 of each case. The
symbolic emitter must reproduce them exactly.
"""
import functools
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tfservingcache_amd.engine import emit
from tfservingcache_amd.engine.planner import (Plan, PlanOp, PlanTensor,
                                               compile_graph)
from tfservingcache_amd.engine.savedmodel import GraphBuilder
from tfservingcache_amd.models import builders

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                          "golden", "call_templates")
BUCKETS = (1, 4)


def build_misc(seed=0):
    """The call kinds no model builder reaches: H/W pad, a batch norm
    with no conv to fold into, a unary eltwise, a mean over the last
    axis and an argmax."""
    rng = np.random.default_rng(seed)
    gb = GraphBuilder()
    f32, i32 = gb.a_type(1), gb.a_type(3)
    c = 8
    x = gb.placeholder("x", np.float32, [-1, 4, 4, c], signature_name="x")
    padded = gb.node(
        "Pad", "pad",
        [x, gb.const("pads", np.array([[0, 0], [1, 1], [1, 2], [0, 0]],
                                      np.int32))],
        T=f32, Tpaddings=i32)
    consts = [gb.const(n, (np.abs(rng.standard_normal(c)) * 0.5 + 0.5
                           ).astype(np.float32))
              for n in ("gamma", "beta", "mean", "var")]
    bn = gb.node("FusedBatchNormV3", "bn", [padded] + consts, T=f32, U=f32,
                 epsilon=gb.a_float(1e-3), is_training=gb.a_bool(False),
                 data_format=gb.a_str("NHWC"))
    th = gb.node("Tanh", "tanh", [bn], T=f32)
    mean = gb.node("Mean", "mean",
                   [th, gb.const("axes", np.array([-1], np.int32))],
                   T=f32, keep_dims=gb.a_bool(False))          # [B,6,7]
    am = gb.node("ArgMax", "am", [mean, gb.const("ax", np.int32(-1))],
                 T=f32, output_type=i32)                       # [B,6]
    gb.mark_output("mean", mean)
    gb.mark_output("idx", am)
    return gb.build()


_BERT_MASKED = dict(seq_len=16, hidden=128, layers=1, heads=2,
                    with_mask=True)
_UNET = dict(image_size=16, base=8)

# case -> (builder, kwargs, engine dtype); seed 0 everywhere
CASES = {
    "mlp_bf16": (builders.build_mlp, {}, "bf16"),
    "mlp_fp8": (builders.build_mlp, {}, "fp8"),
    "unet_deconv": (builders.build_unet,
                    dict(_UNET, upsample="deconv"), "bf16"),
    "unet_nearest": (builders.build_unet,
                     dict(_UNET, upsample="nearest"), "bf16"),
    "unet_bilinear": (builders.build_unet,
                      dict(_UNET, upsample="bilinear"), "bf16"),
    "mobilenet": (builders.build_mobilenet_v2,
                  dict(image_size=32, num_classes=10), "bf16"),
    "resnet": (builders.build_resnet50,
               dict(image_size=32, num_classes=10), "bf16"),
    "bert_masked_bf16": (builders.build_bert, _BERT_MASKED, "bf16"),
    "bert_masked_fp8": (builders.build_bert, _BERT_MASKED, "fp8"),
    "bert_unfused": (builders.build_bert,
                     dict(seq_len=16, hidden=64, layers=1, heads=2),
                     "bf16"),
    "misc": (build_misc, {}, "bf16"),
}


def compile_case(case):
    builder, kwargs, _dtype = CASES[case]
    sm = builder(seed=0, **kwargs)
    mg = sm.meta_graphs[0]
    sig = next(iter(mg.signature_def.values()))
    return compile_graph(mg.graph_def, sig)


@functools.lru_cache(maxsize=None)
def _case(case):
    """(golden record, plan, {bucket: template}), built once per case."""
    with open(os.path.join(GOLDEN_DIR, case + ".json")) as f:
        gold = json.load(f)
    plan = compile_case(case)
    tmpls = {b: emit.build_template(plan, b, CASES[case][2])
             for b in BUCKETS}
    return gold, plan, tmpls


def _jsonable(v):
    """Tuples -> lists, recursively (what json.load gives back)."""
    if isinstance(v, (tuple, list)):
        return [_jsonable(x) for x in v]
    return v


def _f32(xs):
    return [float(np.float32(x)) for x in xs]


def test_every_golden_file_has_a_case_and_back():
    files = sorted(os.path.splitext(os.path.basename(p))[0]
                   for p in glob.glob(os.path.join(GOLDEN_DIR, "*.json")))
    assert files == sorted(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_template_matches_golden(case):
    gold, _plan, tmpls = _case(case)
    assert gold["dtype"] == CASES[case][2]
    assert sorted(gold["buckets"]) == sorted(str(b) for b in BUCKETS)
    for b in BUCKETS:
        g, t = gold["buckets"][str(b)], tmpls[b]
        assert t.total_bytes == g["total_bytes"]
        assert {str(k): v for k, v in t.scratch_off.items()} == \
            g["scratch_off"]
        assert {str(k): [v.offset, v.nbytes]
                for k, v in t.bufs.items()} == g["bufs"]
        assert _jsonable(t.region_keys) == g["region_keys"]
        assert len(t.calls) == len(g["calls"])
        for (kind, descs, ints, floats), gc in zip(t.calls, g["calls"]):
            want_descs = [None if d is None else
                          ["ws", d[1]] if d[0] == emit.WS else
                          [_jsonable(d[0]), d[1]] for d in descs]
            assert [kind, want_descs, list(ints)] == gc[:3]
            assert all(isinstance(i, int) for i in ints)
            assert _f32(floats) == _f32(gc[3])


def test_golden_cases_reach_every_kind():
    seen = set()
    for case in CASES:
        gold = _case(case)[0]
        for rec in gold["buckets"].values():
            seen |= {c[0] for c in rec["calls"]}
    assert seen == set(emit.KINDS)


@pytest.mark.parametrize("case", sorted(CASES))
def test_template_invariants(case):
    gold, plan, tmpls = _case(case)
    layout = emit.blob_layout(plan)
    # the layout _upload_weights used on the parent
    assert {str(i): list(s) for i, s in layout.slots.items()} == \
        gold["blob_slots"]
    assert layout.total == gold["blob_elems"]
    for t in tmpls.values():
        assert t.total_bytes % emit.ALIGN == 0
        for info in t.bufs.values():
            assert info.offset % 256 == 0
            assert 0 <= info.offset and \
                info.offset + info.nbytes <= t.total_bytes
        for off in t.scratch_off.values():
            assert off % 256 == 0 and 0 <= off < t.total_bytes
        for _kind, descs, _ints, _floats in t.calls:
            for d in descs:
                if d is None:
                    continue
                key, off = d
                if key == emit.WS:
                    assert 0 <= off < t.total_bytes
                    continue
                assert key in t.region_keys
                if key == ("blob",):
                    assert 0 <= off < layout.total * 2
                else:
                    assert off == 0


def test_emit_imports_neither_torch_nor_the_extension():
    code = ("import sys; import tfservingcache_amd.engine.emit; "
            "bad = [m for m in sys.modules if m == 'torch' or "
            "m.endswith('_tfsc_engine')]; assert not bad, bad")
    root = os.path.dirname(GOLDEN_DIR.rsplit(os.sep, 2)[0])
    subprocess.run([sys.executable, "-c", code], check=True, cwd=root)


# -- error parity: same type and message as before the split ---------------

def _plan(tensors, ops, n_in=1):
    ts = [PlanTensor(i, shape, dtype, kind, weight=w)
          for i, (shape, dtype, kind, w) in enumerate(tensors)]
    return Plan(ts, ops, {f"in{i}": i for i in range(n_in)},
                {"out": len(ts) - 1}, {})


def _act(*shape):
    return (shape, "f32", "activation", None)


def _inp(*shape):
    return (shape, "f32", "input", None)


def _w(*shape):
    return (shape, "f32", "weight", np.zeros(shape, np.float32))


def test_gemm_trans_a_raises():
    plan = _plan([_inp(-1, 64), _w(64, 32), _act(-1, 32)],
                 [PlanOp("gemm", [0, 1], [2], {"trans_a": True})])
    for dtype in ("bf16", "fp8"):
        with pytest.raises(RuntimeError,
                           match="^gemm trans_a unsupported on GPU$"):
            emit.build_template(plan, 1, dtype)


def test_gemm_needs_a_constant_weight():
    plan = _plan([_inp(-1, 64), _inp(64, 32), _act(-1, 32)],
                 [PlanOp("gemm", [0, 1], [2], {})], n_in=2)
    with pytest.raises(RuntimeError,
                       match="^GPU gemm requires a constant weight "
                             "operand; activation x activation MatMul "
                             "must be BatchMatMul$"):
        emit.build_template(plan, 1, "bf16")
    with pytest.raises(RuntimeError,
                       match="^fp8 gemm requires a constant weight$"):
        emit.build_template(plan, 1, "fp8")


def test_rank7_eltwise_raises():
    big = (-1, 2, 2, 2, 2, 2, 2)
    plan = _plan([_inp(*big), _w(2), _act(*big)],
                 [PlanOp("eltwise", [0, 1], [2], {"fn": "add"})])
    with pytest.raises(RuntimeError, match="^eltwise rank > 6$"):
        emit.build_template(plan, 1, "bf16")


@pytest.mark.parametrize("pads", [
    [[1, 0], [0, 0], [0, 0], [0, 0]],       # N
    [[0, 0], [0, 0], [0, 0], [0, 3]],       # C
])
def test_pad_outside_hw_raises(pads):
    out = tuple(d + lo + hi for d, (lo, hi) in zip((1, 4, 4, 8), pads))
    plan = _plan([_inp(1, 4, 4, 8), _act(*out)],
                 [PlanOp("pad", [0], [1], {"pads": pads})])
    with pytest.raises(RuntimeError,
                       match="^GPU pad: only NHWC H/W pads$"):
        emit.build_template(plan, 1, "bf16")


def test_attention_bias_shape_contradicting_bias_dims_raises():
    qkv = (-1, 8, 2, 64)
    plan = _plan([_inp(*qkv), _inp(*qkv), _inp(*qkv), _inp(-1, 1, 1, 8),
                  _act(*qkv)],
                 [PlanOp("attention", [0, 1, 2, 3], [4],
                         {"scale": 0.125, "bias_dims": (True, 2, 1)})],
                 n_in=4)
    with pytest.raises(ValueError) as ei:
        emit.build_template(plan, 4, "bf16")
    assert str(ei.value) == ("attention bias shape (4, 1, 1, 8) does not "
                             "match plan (4, 2, 1, 8)")


def test_unsupported_op_raises():
    plan = _plan([_inp(-1, 8), _act(-1, 8)],
                 [PlanOp("frobnicate", [0], [1], {})])
    with pytest.raises(RuntimeError,
                       match="^GPU lowering: unsupported op frobnicate$"):
        emit.build_template(plan, 1, "bf16")
