"""Additive attention masks: planner fusion (scale step, bias step,
eligibility), CPU numerics against the unfused plan, and the masked
BERT builder. Runs anywhere (CPU executor only)."""
import numpy as np
import pytest

from tfservingcache_amd.engine.model import LoadedModel, load_model_from_dir
from tfservingcache_amd.engine.planner import _Lowerer
from tfservingcache_amd.engine.savedmodel import (GraphBuilder,
                                                  read_saved_model,
                                                  write_saved_model)
from tfservingcache_amd.models import build_bert

S = 16
RTOL, ATOL = 1e-5, 1e-6          # the tolerances of test_attention_fusion


def _block(scale_op="Mul", bias_first=False, bias="pad", hidden=128,
           heads=2, scores_as_divisor=False, second_consumer=False,
           seed=0):
    """One attention block over x [B, S, hidden] with an additive bias
    on the scaled scores.

    bias: 'pad'    -> input [B,1,1,S]
          'causal' -> constant [1,1,S,S]
          'bss'    -> activation [B,1,S,S] (an input scaled by a Mul)
          'last1'  -> input [B,1,S,1] (not fusable: last dim 1)"""
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
        scaled = gb.node("Mul", "scaled", [scores, c], T=f32)
    else:
        c = gb.const("scale", np.float32(np.sqrt(dh)))
        ins = [c, scores] if scores_as_divisor else [scores, c]
        scaled = gb.node("RealDiv", "scaled", ins, T=f32)

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
    elif bias == "last1":
        b = gb.placeholder("bias", np.float32, [-1, 1, S, 1],
                           signature_name="bias")
    else:
        raise ValueError(bias)
    masked = gb.node("AddV2", "masked",
                     [b, scaled] if bias_first else [scaled, b], T=f32)
    probs = gb.node("Softmax", "probs", [masked], T=f32)
    ctx = gb.node("BatchMatMulV2", "ctx", [probs, vh], T=f32)
    ctx_t = gb.node("Transpose", "ctx_t", [ctx, perm], T=f32)
    y = gb.node("Reshape", "y", [ctx_t, gb.const(
        "to_out", np.array([-1, S, hidden], dtype=np.int32))])
    gb.mark_output("y", y)
    if second_consumer:
        gb.mark_output("peek", gb.node("Neg", "peek", [masked], T=f32))
    return gb.build()


def _load_pair(tmp_path, sm, name):
    """(fused model from the default path, unfused model of the same
    graph: the plan before fuse_attention)."""
    d = tmp_path / name / "1"
    write_saved_model(sm, str(d))
    fused = load_model_from_dir(str(d), name, 1)
    gd, sigs = read_saved_model(str(d))
    unfused = LoadedModel(name, 1, _Lowerer(gd, next(iter(sigs.values()))).run())
    return fused, unfused


def _kinds(model):
    return [op.kind for op in model.plan.ops]


def _assert_fused(model):
    kinds = _kinds(model)
    att = [op for op in model.plan.ops if op.kind == "attention"]
    assert len(att) == 1, kinds
    assert len(att[0].inputs) == 4
    for k in ("softmax", "batched_gemm", "transpose"):
        assert k not in kinds, kinds
    return att[0]


def _assert_unfused(model):
    kinds = _kinds(model)
    assert "attention" not in kinds
    assert "softmax" in kinds and kinds.count("batched_gemm") == 2


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_allclose(a[k], b[k], rtol=RTOL, atol=ATOL,
                                   err_msg=k)


def _x(batch=2, hidden=128, seed=1):
    return np.random.default_rng(seed).standard_normal(
        (batch, S, hidden)).astype(np.float32)


# right-padded, left-padded, one valid token (row 0 / row 1 of the batch)
_MASKS = {
    "right": np.array([[1] * 11 + [0] * 5, [1] * 3 + [0] * 13]),
    "left": np.array([[0] * 6 + [1] * 10, [0] * 15 + [1]]),
    "one": np.array([[1] + [0] * 15, [0] * 7 + [1] + [0] * 8]),
}


def _pad_bias(mask):
    return ((1.0 - mask.astype(np.float32)) * -10000.0).reshape(
        mask.shape[0], 1, 1, S)


@pytest.mark.parametrize("scale_op", ["Mul", "RealDiv"])
@pytest.mark.parametrize("bias_first", [False, True],
                         ids=["scores_first", "bias_first"])
def test_masked_attention_fuses(tmp_path, scale_op, bias_first):
    fused, unfused = _load_pair(
        tmp_path, _block(scale_op=scale_op, bias_first=bias_first), "blk")
    att = _assert_fused(fused)
    assert att.params["bias_dims"] == (True, 1, 1)
    assert att.params["scale"] == pytest.approx(0.125)
    assert fused.plan.tensors[att.inputs[3]].kind == "input"
    _assert_unfused(unfused)
    x = _x()
    for name, mask in _MASKS.items():
        feeds = {"x": x, "bias": _pad_bias(mask)}
        _same(fused.predict(feeds), unfused.predict(feeds))


def test_masked_keys_do_not_leak(tmp_path):
    """Changing x at masked positions leaves the valid rows' output
    unchanged (a sanity check of the reference itself)."""
    fused, _ = _load_pair(tmp_path, _block(), "leak")
    mask = _MASKS["right"]
    x = _x()
    x2 = x.copy()
    x2[0, 11:] += 3.0
    x2[1, 3:] -= 2.0
    a = fused.predict({"x": x, "bias": _pad_bias(mask)})["y"]
    b = fused.predict({"x": x2, "bias": _pad_bias(mask)})["y"]
    np.testing.assert_allclose(a[0, :11], b[0, :11], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(a[1, :3], b[1, :3], rtol=RTOL, atol=ATOL)


def test_neg_inf_bias_equals_dropping_keys(tmp_path):
    fused, _ = _load_pair(tmp_path, _block(), "ninf")
    mask = _MASKS["left"]
    x = _x()
    bias = np.where(mask.reshape(2, 1, 1, S) > 0, 0.0,
                    -np.inf).astype(np.float32)
    a = fused.predict({"x": x, "bias": bias})["y"]
    b = fused.predict({"x": x, "bias": _pad_bias(mask)})["y"]
    assert np.all(np.isfinite(a))
    np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL)
    # every key at -inf: zeros, not NaN
    allinf = np.full((2, 1, 1, S), -np.inf, np.float32)
    z = fused.predict({"x": x, "bias": allinf})["y"]
    np.testing.assert_array_equal(z, np.zeros_like(z))


def test_causal_constant_bias_fuses(tmp_path):
    fused, unfused = _load_pair(tmp_path, _block(bias="causal"), "causal")
    att = _assert_fused(fused)
    assert att.params["bias_dims"] == (False, 1, S)
    assert fused.plan.tensors[att.inputs[3]].kind == "weight"
    x = _x(batch=3)
    _same(fused.predict({"x": x}), unfused.predict({"x": x}))


def test_per_batch_query_activation_bias_fuses(tmp_path):
    fused, unfused = _load_pair(tmp_path, _block(bias="bss"), "bss")
    att = _assert_fused(fused)
    assert att.params["bias_dims"] == (True, 1, S)
    assert fused.plan.tensors[att.inputs[3]].kind == "activation"
    feeds = {"x": _x(), "bias": np.random.default_rng(5).uniform(
        -4, 4, (2, S, S)).astype(np.float32)}
    _same(fused.predict(feeds), unfused.predict(feeds))


@pytest.mark.parametrize("case", ["last1", "head_dim32", "second_consumer",
                                  "scores_as_divisor"])
def test_ineligible_chains_stay_unfused(tmp_path, case):
    hidden = 128
    if case == "last1":
        sm = _block(bias="last1")
        bias = np.random.default_rng(2).uniform(
            -2, 2, (2, 1, S, 1)).astype(np.float32)
    else:
        bias = _pad_bias(_MASKS["right"])
        if case == "head_dim32":
            hidden = 64
            sm = _block(hidden=64)
        elif case == "second_consumer":
            sm = _block(second_consumer=True)
        else:
            sm = _block(scale_op="RealDiv", scores_as_divisor=True)
    model, unfused = _load_pair(tmp_path, sm, case)
    _assert_unfused(model)
    feeds = {"x": _x(hidden=hidden), "bias": bias}
    out = model.predict(feeds)
    _same(out, unfused.predict(feeds))
    assert np.all(np.isfinite(out["y"]))


# -- build_bert(with_mask=True) ---------------------------------------------
_BERT = dict(seq_len=S, hidden=128, layers=1, heads=2, intermediate=64,
             vocab=60, seed=13)


def _bert(tmp_path, name, **kw):
    d = tmp_path / name / "1"
    write_saved_model(build_bert(**_BERT, **kw), str(d))
    return load_model_from_dir(str(d), name, 1)


def test_bert_with_mask_signature_and_all_ones(tmp_path):
    masked = _bert(tmp_path, "bm", with_mask=True)
    plain = _bert(tmp_path, "bp")
    assert set(masked.plan.sig_inputs) == {"input_ids", "input_mask"}
    assert set(plain.plan.sig_inputs) == {"input_ids"}
    att = _assert_fused(masked)
    assert att.params["bias_dims"] == (True, 1, 1)
    ids = np.random.default_rng(3).integers(0, 60, (2, S)).astype(np.int32)
    a = masked.predict({"input_ids": ids,
                        "input_mask": np.ones((2, S), np.int32)})
    b = plain.predict({"input_ids": ids})
    for k in ("sequence_output", "pooled_output"):
        np.testing.assert_allclose(a[k], b[k], rtol=1e-5, atol=ATOL)


def test_bert_with_mask_keeps_weights(tmp_path):
    """The mask nodes draw nothing from the rng: same seed, same
    weights."""
    wm = {t.name: t.weight for t in _bert(tmp_path, "wm",
                                          with_mask=True).plan.tensors
          if t.weight is not None}
    wp = {t.name: t.weight for t in _bert(tmp_path, "wp").plan.tensors
          if t.weight is not None}
    assert set(wp) <= set(wm)
    for k, w in wp.items():
        np.testing.assert_array_equal(w, wm[k], err_msg=k)


def test_bert_masked_positions_do_not_reach_valid_ones(tmp_path):
    masked = _bert(tmp_path, "bmm", with_mask=True)
    rng = np.random.default_rng(4)
    ids = rng.integers(0, 60, (2, S)).astype(np.int32)
    mask = np.ones((2, S), np.int32)
    mask[0, 9:] = 0
    mask[1, 4:] = 0
    ids2 = ids.copy()
    ids2[0, 9:] = (ids[0, 9:] + 17) % 60
    ids2[1, 4:] = (ids[1, 4:] + 23) % 60
    a = masked.predict({"input_ids": ids, "input_mask": mask})
    b = masked.predict({"input_ids": ids2, "input_mask": mask})
    sa, sb = a["sequence_output"], b["sequence_output"]
    np.testing.assert_allclose(sa[0, :9], sb[0, :9], rtol=1e-5, atol=ATOL)
    np.testing.assert_allclose(sa[1, :4], sb[1, :4], rtol=1e-5, atol=ATOL)
    # and the masked rows did change (the inputs differ there)
    assert np.abs(sa[0, 9:] - sb[0, 9:]).max() > 1e-3


def test_masked_and_unmasked_plans_do_not_collide(tmp_path):
    """The plan cache dedups by SavedModel content: a masked and an
    unmasked model of one seed must get different plans, and two copies
    of the masked model the same one."""
    m1 = _bert(tmp_path, "k1", with_mask=True)
    p1 = _bert(tmp_path, "k2")
    m2 = _bert(tmp_path, "k3", with_mask=True)
    assert m1.plan is not p1.plan
    assert m1.plan is m2.plan
    n_in = {len(op.inputs) for op in m1.plan.ops if op.kind == "attention"}
    assert n_in == {4}
    n_in = {len(op.inputs) for op in p1.plan.ops if op.kind == "attention"}
    assert n_in == {3}
    assert all("bias_dims" not in op.params for op in p1.plan.ops)
