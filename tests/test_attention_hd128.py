"""head_dim 128 attention: planner fusion and CPU numerics against the
unfused plan. Runs anywhere (CPU executor only).

Blocks are the graphs of test_attention_mask.py::_block at hidden=256,
heads=2, S=16. Fused and unfused plans are both f32 and differ only in
summation order; over a 128-long contraction the worst difference
measured on these graphs was 3.6e-6 (the [B,1,S,S] case), so the block
comparisons use atol=1e-5. The BERT comparison measured <= 7.2e-7 and
keeps the project's usual atol=1e-6.
"""
import numpy as np
import pytest

from tfservingcache_amd.engine.model import LoadedModel, load_model_from_dir
from tfservingcache_amd.engine.planner import _Lowerer
from tfservingcache_amd.engine.savedmodel import (GraphBuilder,
                                                  read_saved_model,
                                                  write_saved_model)
from tfservingcache_amd.models import build_bert

S = 16
RTOL, ATOL = 1e-5, 1e-5


def _block(scale_op="Mul", bias=None, hidden=256, heads=2, seed=0):
    """One attention block over x [B, S, hidden].

    bias: None     -> unmasked
          'pad'    -> input [B,1,1,S]
          'causal' -> constant [1,1,S,S]
          'bss'    -> activation [B,1,S,S] (an input scaled by a Mul)"""
    rng = np.random.default_rng(seed)
    dh = hidden // heads
    gb = GraphBuilder()
    f32 = gb.a_type(1)
    x = gb.placeholder("x", np.float32, [-1, S, hidden], signature_name="x")
    x2 = gb.node("Reshape", "x2", [x, gb.const(
        "to_2d", np.array([-1, hidden], dtype=np.int32))])
    to_heads = gb.const("to_heads",
                        np.array([-1, S, heads, dh], dtype=np.int32))
    perm = gb.const("perm0213", np.array([0, 2, 1, 3], dtype=np.int32))

    def head(name):
        w = gb.const(f"{name}/w", (rng.standard_normal((hidden, hidden))
                                   * 0.1).astype(np.float32))
        mm = gb.node("MatMul", f"{name}/mm", [x2, w], T=f32)
        r = gb.node("Reshape", f"{name}/r", [mm, to_heads])
        return gb.node("Transpose", f"{name}/t", [r, perm], T=f32)

    qh, kh, vh = head("q"), head("k"), head("v")
    scores = gb.node("BatchMatMulV2", "scores", [qh, kh], T=f32,
                     adj_x=gb.a_bool(False), adj_y=gb.a_bool(True))
    if scale_op == "Mul":
        c = gb.const("scale", np.float32(1.0 / np.sqrt(dh)))
        pre = gb.node("Mul", "scaled", [scores, c], T=f32)
    else:
        c = gb.const("scale", np.float32(np.sqrt(dh)))
        pre = gb.node("RealDiv", "scaled", [scores, c], T=f32)

    if bias is not None:
        if bias == "pad":
            b = gb.placeholder("bias", np.float32, [-1, 1, 1, S],
                               signature_name="bias")
        elif bias == "causal":
            tri = np.triu(np.full((S, S), -10000.0, np.float32), k=1)
            b = gb.const("bias", tri.reshape(1, 1, S, S))
        elif bias == "bss":
            raw = gb.placeholder("bias", np.float32, [-1, S, S],
                                 signature_name="bias")
            half = gb.node("Mul", "bias_half",
                           [raw, gb.const("half", np.float32(0.5))], T=f32)
            b = gb.node("Reshape", "bias4", [half, gb.const(
                "to_b4", np.array([-1, 1, S, S], dtype=np.int32))])
        else:
            raise ValueError(bias)
        pre = gb.node("AddV2", "masked", [pre, b], T=f32)
    probs = gb.node("Softmax", "probs", [pre], T=f32)
    ctx = gb.node("BatchMatMulV2", "ctx", [probs, vh], T=f32)
    ctx_t = gb.node("Transpose", "ctx_t", [ctx, perm], T=f32)
    y = gb.node("Reshape", "y", [ctx_t, gb.const(
        "to_out", np.array([-1, S, hidden], dtype=np.int32))])
    gb.mark_output("y", y)
    return gb.build()


def _load_pair(tmp_path, sm, name):
    """(model from the default path, unfused model of the same graph:
    the plan before fuse_attention)."""
    d = tmp_path / name / "1"
    write_saved_model(sm, str(d))
    fused = load_model_from_dir(str(d), name, 1)
    gd, sigs = read_saved_model(str(d))
    unfused = LoadedModel(name, 1,
                          _Lowerer(gd, next(iter(sigs.values()))).run())
    return fused, unfused


def _kinds(model):
    return [op.kind for op in model.plan.ops]


def _assert_fused_hd128(model, n_inputs):
    kinds = _kinds(model)
    att = [op for op in model.plan.ops if op.kind == "attention"]
    assert len(att) == 1, kinds
    assert len(att[0].inputs) == n_inputs
    assert att[0].params["head_dim"] == 128
    assert att[0].params["heads"] == 2 and att[0].params["seq"] == S
    assert att[0].params["scale"] == pytest.approx(128 ** -0.5)
    for k in ("softmax", "batched_gemm", "transpose"):
        assert k not in kinds, kinds
    return att[0]


def _assert_unfused(model):
    kinds = _kinds(model)
    assert "attention" not in kinds
    assert "softmax" in kinds and kinds.count("batched_gemm") == 2


def _same(a, b, atol=ATOL):
    assert a.keys() == b.keys()
    for k in a:
        err = float(np.abs(a[k] - b[k]).max())
        print(f"{k}: max|fused-unfused|={err:.3g}")
        np.testing.assert_allclose(a[k], b[k], rtol=RTOL, atol=atol,
                                   err_msg=k)


def _x(batch=2, hidden=256, seed=1):
    return np.random.default_rng(seed).standard_normal(
        (batch, S, hidden)).astype(np.float32)


def _feeds(bias, batch=2, hidden=256):
    feeds = {"x": _x(batch, hidden)}
    if bias == "pad":
        mask = np.array([[1] * 11 + [0] * 5, [0] * 6 + [1] * 10][:batch])
        feeds["bias"] = ((1.0 - mask.astype(np.float32)) * -10000.0
                         ).reshape(batch, 1, 1, S)
    elif bias == "bss":
        feeds["bias"] = np.random.default_rng(5).uniform(
            -4, 4, (batch, S, S)).astype(np.float32)
    return feeds


_BIAS_DIMS = {"pad": (True, 1, 1), "causal": (False, 1, S),
              "bss": (True, 1, S)}


@pytest.mark.parametrize("scale_op", ["Mul", "RealDiv"])
@pytest.mark.parametrize("bias", [None, "pad", "causal", "bss"],
                         ids=["unmasked", "pad", "causal", "bss"])
def test_hd128_block_fuses_and_matches_unfused(tmp_path, bias, scale_op):
    fused, unfused = _load_pair(
        tmp_path, _block(scale_op=scale_op, bias=bias), "blk")
    att = _assert_fused_hd128(fused, 3 if bias is None else 4)
    if bias is None:
        assert "bias_dims" not in att.params
    else:
        assert att.params["bias_dims"] == _BIAS_DIMS[bias]
    _assert_unfused(unfused)
    feeds = _feeds(bias)
    out = fused.predict(feeds)
    assert np.all(np.isfinite(out["y"]))
    _same(out, unfused.predict(feeds))


@pytest.mark.parametrize("hidden,heads", [(192, 2), (64, 2)],
                         ids=["head_dim96", "head_dim32"])
@pytest.mark.parametrize("bias", [None, "pad"], ids=["unmasked", "pad"])
def test_other_head_dims_stay_unfused(tmp_path, hidden, heads, bias):
    model, unfused = _load_pair(
        tmp_path, _block(bias=bias, hidden=hidden, heads=heads), "other")
    _assert_unfused(model)
    feeds = _feeds(bias, hidden=hidden)
    out = model.predict(feeds)
    assert np.all(np.isfinite(out["y"]))
    _same(out, unfused.predict(feeds))
    # and against softmax(QK^T/sqrt(d) + bias) V computed here, from
    # the weights _block draws (seed 0, in the order q, k, v)
    rng = np.random.default_rng(0)
    x = feeds["x"].reshape(-1, hidden)
    dh = hidden // heads
    q, k, v = (
        (x @ (rng.standard_normal((hidden, hidden)) * 0.1).astype(np.float32)
         ).reshape(-1, S, heads, dh).transpose(0, 2, 1, 3) for _ in range(3))
    sc = q @ k.transpose(0, 1, 3, 2) / np.sqrt(dh)
    if bias is not None:
        sc = sc + feeds["bias"]
    p = np.exp(sc - sc.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    want = (p @ v).transpose(0, 2, 1, 3).reshape(-1, S, hidden)
    np.testing.assert_allclose(out["y"], want, rtol=1e-4, atol=1e-5)


# -- build_bert at hidden=256, heads=2 ---------------------------------------
_BERT = dict(seq_len=S, hidden=256, layers=2, heads=2, intermediate=64,
             vocab=60, seed=13)


@pytest.mark.parametrize("with_mask", [False, True],
                         ids=["plain", "with_mask"])
def test_bert_hd128_one_attention_per_layer(tmp_path, with_mask):
    fused, unfused = _load_pair(
        tmp_path, build_bert(**_BERT, with_mask=with_mask), "b128")
    att = [op for op in fused.plan.ops if op.kind == "attention"]
    assert len(att) == 2
    assert all(op.params["head_dim"] == 128 for op in att)
    assert all(len(op.inputs) == (4 if with_mask else 3) for op in att)
    kinds = _kinds(fused)
    assert "softmax" not in kinds and "batched_gemm" not in kinds
    assert _kinds(unfused).count("softmax") == 2
    rng = np.random.default_rng(3)
    feeds = {"input_ids": rng.integers(0, 60, (2, S)).astype(np.int32)}
    if with_mask:
        mask = np.ones((2, S), np.int32)
        mask[0, 9:] = 0
        mask[1, :4] = 0
        feeds["input_mask"] = mask
    _same(fused.predict(feeds), unfused.predict(feeds), atol=1e-6)
