"""Dilated (atrous) Conv2D and DepthwiseConv2dNative through the planner,
the CPU executor, call emission and the build_deeplab fixture.

A dilation reaches the planner in two spellings: the `dilations`
attribute, and SpaceToBatchND -> VALID conv -> BatchToSpaceND (TF1/slim,
tf.nn.atrous_conv2d, every dilated tf.nn.depthwise_conv2d). Both must
compile to the same single op. The numeric reference is a plain float64
numpy dilated conv written here.
"""
import numpy as np
import pytest

from tfservingcache_amd.engine import emit
from tfservingcache_amd.engine.model import LoadedModel
from tfservingcache_amd.engine.planner import PlanError, compile_graph
from tfservingcache_amd.engine.savedmodel import (GraphBuilder,
                                                  read_saved_model,
                                                  write_saved_model)
from tfservingcache_amd.models import build_deeplab

EPS = 1.001e-5
H, RATE = 7, 2      # padded 7 + 4 = 11 -> 12: extra padding and an end crop


def _compile(tmp_path, sm, name):
    d = str(tmp_path / name / "1")
    write_saved_model(sm, d)
    graph_def, sigs = read_saved_model(d)
    return LoadedModel(name, 1,
                       compile_graph(graph_def, next(iter(sigs.values()))))


def _params(op, C, K, seed=0):
    rng = np.random.default_rng(seed)
    shape = (3, 3, C, K) if op == "Conv2D" else (3, 3, C, 1)
    p = {"w": (rng.standard_normal(shape) * 0.3).astype(np.float32)}
    for n in ("gamma", "var"):
        p[n] = (np.abs(rng.standard_normal(K)) * 0.5 + 0.5).astype(np.float32)
    for n in ("beta", "mean"):
        p[n] = (rng.standard_normal(K) * 0.1).astype(np.float32)
    return p


def _graph(op, p, spelling, C=16, rate=(RATE, RATE), fused=True, tag="",
           dilations=None, block2=None, crop0=0, lone=False):
    """One 3x3 SAME-equivalent dilated conv on [-1,H,H,C], spelt by the
    `dilations` attribute or as the sandwich, optionally + BN + Relu."""
    gb = GraphBuilder()
    f32, i32 = gb.a_type(1), gb.a_type(3)
    x = gb.placeholder("input", np.float32, [-1, H, H, C],
                       signature_name="input")
    conv = dict(T=f32, strides=gb.a_ints([1, 1, 1, 1]),
                data_format=gb.a_str("NHWC"))
    w = gb.const("w", p["w"])
    if spelling == "attr":
        y = gb.node(op, f"conv{tag}", [x, w], padding=gb.a_str("SAME"),
                    dilations=gb.a_ints(dilations or [1, *rate, 1]), **conv)
    else:
        extra = [-(H + 2 * r) % r for r in rate]
        ints = lambda n, v: gb.const(n, np.asarray(v, np.int32))  # noqa: E731
        y = gb.node("SpaceToBatchND", f"s2b{tag}",
                    [x, ints("block", rate),
                     ints("paddings", [[r, r + e]
                                       for r, e in zip(rate, extra)])],
                    T=f32, Tblock_shape=i32, Tpaddings=i32)
        if not lone:
            y = gb.node(op, f"conv{tag}", [y, w], padding=gb.a_str("VALID"),
                        **conv)
            y = gb.node("BatchToSpaceND", f"b2s{tag}",
                        [y, ints("block2", block2 or rate),
                         ints("crops", [[crop0, e] for e in extra])],
                        T=f32, Tblock_shape=i32, Tcrops=i32)
    if fused:
        y = gb.node("FusedBatchNormV3", "bn",
                    [y] + [gb.const(n, p[n])
                           for n in ("gamma", "beta", "mean", "var")],
                    T=f32, U=f32, epsilon=gb.a_float(EPS),
                    is_training=gb.a_bool(False),
                    data_format=gb.a_str("NHWC"))
        y = gb.node("Relu", "relu", [y], T=f32)
    gb.mark_output("y", y)
    return gb.build()


def _numpy_ref(x, p, depthwise, rate):
    """float64 3x3 dilated SAME conv (stride 1, so SAME pads `rate` on
    both sides) + BN + Relu, tap by tap."""
    x = x.astype(np.float64)
    w = p["w"].astype(np.float64)
    xp = np.pad(x, ((0, 0), (rate, rate), (rate, rate), (0, 0)))
    K = p["gamma"].shape[0]
    y = np.zeros(x.shape[:3] + (K,))
    for r in range(3):
        for s in range(3):
            patch = xp[:, r * rate:r * rate + H, s * rate:s * rate + H, :]
            y += patch * w[r, s, :, 0] if depthwise else patch @ w[r, s]
    y = (y - p["mean"]) / np.sqrt(p["var"].astype(np.float64) + EPS) \
        * p["gamma"] + p["beta"]
    return np.maximum(y, 0.0)


@pytest.mark.parametrize("op", ["Conv2D", "DepthwiseConv2dNative"])
def test_both_spellings_compile_to_one_op(tmp_path, op):
    C = 16
    p = _params(op, C, 24 if op == "Conv2D" else C)
    a = _compile(tmp_path, _graph(op, p, "attr"), "attr")
    b = _compile(tmp_path, _graph(op, p, "sandwich"), "sandwich")
    assert len(a.plan.ops) == 1 and len(b.plan.ops) == 1
    oa, ob = a.plan.ops[0], b.plan.ops[0]
    assert oa.kind == ob.kind and oa.params == ob.params
    assert oa.params["dilation"] == (RATE, RATE)
    assert oa.params["pads"] == (RATE,) * 4
    assert oa.params["out_hw"] == (H, H) and oa.params["act"] == "relu"
    for i in (1, 2):                                # BN-folded w and bias
        np.testing.assert_array_equal(a.plan.tensors[oa.inputs[i]].weight,
                                      b.plan.tensors[ob.inputs[i]].weight)
    x = np.random.default_rng(1).standard_normal((2, H, H, C)).astype(
        np.float32)
    want = _numpy_ref(x, p, op != "Conv2D", RATE)
    for lm in (a, b):
        np.testing.assert_allclose(lm.predict({"input": x})["y"], want,
                                   rtol=1e-4, atol=1e-4)


def test_1x1_dilation_is_normalised_away(tmp_path):
    gb = GraphBuilder()
    x = gb.placeholder("input", np.float32, [-1, H, H, 64],
                       signature_name="input")
    y = gb.node("Conv2D", "conv",
                [x, gb.const("w", np.ones((1, 1, 64, 8), np.float32))],
                T=gb.a_type(1), strides=gb.a_ints([1, 1, 1, 1]),
                dilations=gb.a_ints([1, 2, 2, 1]), padding=gb.a_str("SAME"),
                data_format=gb.a_str("NHWC"))
    gb.mark_output("y", y)
    lm = _compile(tmp_path, gb.build(), "one")
    assert "dilation" not in lm.plan.ops[0].params
    assert [c[0] for c in emit.build_template(lm.plan, 4, "bf16").calls] \
        == ["GEMM"]


_PLAN_ERRORS = {
    # name: (graph kwargs, op, C, K, node the message must name)
    "start_crop": (dict(spelling="sandwich", crop0=1), "Conv2D", 16, 16,
                   "b2s_e"),
    "mismatched_blocks": (dict(spelling="sandwich", block2=(2, 3)),
                          "Conv2D", 16, 16, "b2s_e"),
    "lone_space_to_batch": (dict(spelling="sandwich", lone=True,
                                 fused=False), "Conv2D", 16, 16, "s2b_e"),
    "batch_axis": (dict(spelling="attr", dilations=[2, 2, 2, 1]), "Conv2D",
                   16, 16, "conv_e"),
    "grouped": (dict(spelling="attr", C=32), "Conv2D", 16, 16, "conv_e"),
    "c12": (dict(spelling="attr", C=12), "Conv2D", 12, 16, "conv_e"),
}


@pytest.mark.parametrize("name", list(_PLAN_ERRORS))
def test_plan_errors_name_the_node(tmp_path, name):
    kw, op, C, K, node = _PLAN_ERRORS[name]
    with pytest.raises(PlanError, match=node):
        _compile(tmp_path, _graph(op, _params(op, C, K), tag="_e", **kw),
                 name)


@pytest.mark.parametrize("op,kind,dilated,plain", [
    ("Conv2D", "CONV", 18, 15), ("DepthwiseConv2dNative", "DEPTHWISE", 16, 13)])
def test_emission(tmp_path, op, kind, dilated, plain):
    p = _params(op, 16, 16)
    for rate, n_ints in ((3, dilated), (1, plain)):
        lm = _compile(tmp_path, _graph(op, p, "attr", rate=(rate, 1)),
                      f"r{rate}")
        calls = emit.build_template(lm.plan, 4, "bf16").calls
        assert [c[0] for c in calls] == [kind]
        ints = calls[0][2]
        assert len(ints) == n_ints
        if rate > 1:
            assert list(ints[-3:]) == [1, 3, 1]     # groups | M, dh, dw


def test_deeplab_fixture_cpu(tmp_path):
    lm = _compile(tmp_path, build_deeplab(image_size=33), "dl")
    dil = [(op.kind, op.params["dilation"]) for op in lm.plan.ops
           if "dilation" in op.params]
    assert dil == [("conv2d", (2, 2)), ("depthwise_conv", (2, 2)),
                   ("conv2d", (6, 6)), ("conv2d", (12, 12)),
                   ("conv2d", (18, 18))]
    assert not any(t.name.endswith(("s2b:0", "b2s:0"))
                   for t in lm.plan.tensors)
    x = (np.random.default_rng(0).standard_normal((2, 33, 33, 3)) * 0.3
         ).astype(np.float32)
    probs = lm.predict({"input": x})["probs"]
    assert probs.shape == (2, 33, 33, 5)
    np.testing.assert_allclose(probs.sum(-1), 1.0, atol=1e-4)
