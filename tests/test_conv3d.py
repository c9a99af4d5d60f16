"""Conv3D / MaxPool3D / AvgPool3D through the planner, the CPU executor and
call emission. The reference is torch float64 on input padded explicitly by
TF's rules: conv3d, max over -inf padding, sum-pool(x) / sum-pool(ones).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tfservingcache_amd.engine import emit
from tfservingcache_amd.engine.model import LoadedModel
from tfservingcache_amd.engine.planner import PlanError, compile_graph
from tfservingcache_amd.engine.savedmodel import (GraphBuilder,
                                                  read_saved_model,
                                                  write_saved_model)
from tfservingcache_amd.models import build_video_resnet

EPS = 1.001e-5
DHW, C, K = (5, 6, 7), 4, 6


def _compile(tmp_path, sm, name="m"):
    d = str(tmp_path / name / "1")
    write_saved_model(sm, d)
    graph_def, sigs = read_saved_model(d)
    return LoadedModel(name, 1,
                       compile_graph(graph_def, next(iter(sigs.values()))))


def geometry(dims, window, stride, padding):
    # per axis (out, pad before, pad after), TF rules: low half first
    res = []
    for size, k, s in zip(dims, window, stride):
        out = -(-size // s) if padding == "SAME" else (size - k) // s + 1
        tot = max((out - 1) * s + k - size, 0) if padding == "SAME" else 0
        res.append((out, tot // 2, tot - tot // 2))
    return res


def padded(x, geom, value=0.0):
    pads = [p for (_, lo, hi) in reversed(geom) for p in (lo, hi)]
    return F.pad(x.double().permute(0, 4, 1, 2, 3), pads, value=value)


def _graph(op, name, in_shape=(-1, *DHW, C), w=None, const_w=True, bn=None,
           res_shape=None, **attrs):
    # one Conv3D (optionally + BN(NDHWC) + residual + Relu) or 3-D pool
    gb = GraphBuilder()
    f32 = gb.a_type(1)
    ins = [gb.placeholder("input", np.float32, list(in_shape),
                          signature_name="input")]
    if w is not None:
        ins.append(gb.const("w", w) if const_w else gb.placeholder(
            "w", np.float32, list(w.shape), signature_name="w"))
    if bn is not None:          # before the conv: lowered when it folds
        r = gb.placeholder("res", np.float32, [-1, *res_shape],
                           signature_name="res")
    attrs.setdefault("data_format", "NDHWC")
    y = gb.node(op, name, ins, T=f32, **{
        k: gb.a_str(v) if isinstance(v, str) else gb.a_ints(v)
        for k, v in attrs.items()})
    if bn is not None:
        y = gb.node("FusedBatchNormV3", "bn",
                    [y] + [gb.const(f"bn{i}", v) for i, v in enumerate(bn)],
                    T=f32, U=f32, epsilon=gb.a_float(EPS),
                    is_training=gb.a_bool(False),
                    data_format=gb.a_str("NDHWC"))
        y = gb.node("Relu", "relu",
                    [gb.node("AddV2", "add", [y, r], T=f32)], T=f32)
    gb.mark_output("y", y)
    return gb.build()


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("padding", ["SAME", "VALID"])
@pytest.mark.parametrize("stride", [(1, 1, 1), (2, 2, 2), (2, 1, 2)])
@pytest.mark.parametrize("trs", [(3, 3, 3), (1, 3, 3), (3, 1, 1), (2, 4, 3)])
def test_conv3d_cpu_vs_torch(tmp_path, trs, stride, padding, fused):
    rng = np.random.default_rng(sum(trs) + sum(stride))
    w = (rng.standard_normal((*trs, C, K)) * 0.3).astype(np.float32)
    x = rng.standard_normal((2, *DHW, C)).astype(np.float32)
    geom = geometry(DHW, trs, stride, padding)
    out_dhw = tuple(o for o, _, _ in geom)
    want = F.conv3d(padded(torch.from_numpy(x), geom),
                    torch.from_numpy(w).double().permute(4, 3, 0, 1, 2),
                    stride=stride).permute(0, 2, 3, 4, 1).numpy()
    feeds, bn = {"input": x}, None
    if fused:
        bn = [(np.abs(rng.standard_normal(K)) * 0.5 + 0.5 if i in (0, 3)
               else rng.standard_normal(K) * 0.1).astype(np.float32)
              for i in range(4)]                # gamma, beta, mean, var
        gamma, beta, mean, var = (v.astype(np.float64) for v in bn)
        feeds["res"] = rng.standard_normal((2, *out_dhw, K)).astype(
            np.float32)
        want = np.maximum((want - mean) / np.sqrt(var + EPS) * gamma + beta
                          + feeds["res"], 0.0)
    lm = _compile(tmp_path, _graph("Conv3D", "conv", w=w, bn=bn,
                                   res_shape=(*out_dhw, K), padding=padding,
                                   strides=[1, *stride, 1]))
    (op,) = lm.plan.ops                 # BN, add and relu folded
    assert op.kind == "conv3d" and op.params["out_dhw"] == out_dhw
    np.testing.assert_allclose(lm.predict(feeds)["y"], want, rtol=1e-4,
                               atol=1e-5)


def pool_reference(x, geom, is_max, window, stride):
    if is_max:
        y = F.max_pool3d(padded(x, geom, float("-inf")), window, stride)
    else:
        y = F.avg_pool3d(padded(x, geom), window, stride,
                         divisor_override=1) / \
            F.avg_pool3d(padded(torch.ones_like(x), geom), window, stride,
                         divisor_override=1)
    return y.permute(0, 2, 3, 4, 1).contiguous()


@pytest.mark.parametrize("padding", ["SAME", "VALID"])
@pytest.mark.parametrize("ksize,stride", [
    ((3, 3, 3), (2, 2, 2)), ((1, 3, 3), (1, 2, 2)), ((3, 1, 1), (1, 1, 1)),
    ((2, 2, 3), (2, 1, 2))])
@pytest.mark.parametrize("op", ["MaxPool3D", "AvgPool3D"])
def test_pool3d_cpu_vs_torch(tmp_path, op, ksize, stride, padding):
    x = torch.randn(2, *DHW, C, generator=torch.Generator().manual_seed(3))
    want = pool_reference(x, geometry(DHW, ksize, stride, padding),
                          op == "MaxPool3D", ksize, stride)
    lm = _compile(tmp_path, _graph(op, "pool", ksize=[1, *ksize, 1],
                                   strides=[1, *stride, 1], padding=padding))
    assert [o.kind for o in lm.plan.ops] == ["pool3d"]
    np.testing.assert_allclose(lm.predict({"input": x.numpy()})["y"],
                               want.numpy(), rtol=1e-4, atol=1e-5)


_W = np.ones((3, 3, 3, C, K), np.float32)
_POOL = dict(ksize=[1, 2, 2, 2, 1], strides=[1, 2, 2, 2, 1], padding="SAME")
_PLAN_ERRORS = {
    # name: (op, graph kwargs[, what the message must match: the node])
    "ncdhw": ("Conv3D", dict(w=_W, data_format="NCDHW")),
    "dilated": ("Conv3D", dict(w=_W, dilations=[1, 2, 2, 2, 1]),
                "dilated.*n_e"),
    "grouped": ("Conv3D", dict(w=_W, in_shape=(-1, *DHW, 2 * C))),
    "symbolic_dim": ("Conv3D", dict(w=_W, in_shape=(-1, -1, 6, 7, C))),
    "batch_stride": ("Conv3D", dict(w=_W, strides=[2, 1, 1, 1, 1])),
    "channel_stride": ("Conv3D", dict(w=_W, strides=[1, 1, 1, 1, 2])),
    "filter_not_const": ("Conv3D", dict(w=_W, const_w=False)),
    "pool_batch_ksize": ("MaxPool3D", {**_POOL, "ksize": [2, 2, 2, 2, 1]}),
    "pool_channel_stride": ("AvgPool3D",
                            {**_POOL, "strides": [1, 2, 2, 2, 2]}),
    "backprop_input": ("Conv3DBackpropInputV2", dict(w=_W),
                       "unsupported op Conv3DBackpropInputV2"),
}


@pytest.mark.parametrize("name", list(_PLAN_ERRORS))
def test_plan_errors_name_the_node(tmp_path, name):
    op, kw, *match = _PLAN_ERRORS[name]
    with pytest.raises(PlanError, match=(match or ["n_e"])[0]):
        _compile(tmp_path, _graph(op, "n_e", **kw))


def test_emission_beside_the_2d_forms(tmp_path):
    gb = GraphBuilder()
    f32 = gb.a_type(1)

    def branch(tag, shape, w_shape, fmt, conv, pool, c_st, p_ks, p_st):
        x = gb.placeholder(tag, np.float32, shape, signature_name=tag)
        kw = dict(T=f32, padding=gb.a_str("SAME"), data_format=gb.a_str(fmt))
        y = gb.node(conv, f"c{tag}",
                    [x, gb.const(f"w{tag}", np.ones(w_shape, np.float32))],
                    strides=gb.a_ints(c_st), **kw)
        y = gb.node(pool, f"p{tag}", [y], ksize=gb.a_ints(p_ks),
                    strides=gb.a_ints(p_st), **kw)
        gb.mark_output(f"y{tag}", y)

    branch("a", [-1, 4, 7, 6, 16], (3, 2, 3, 16, 24), "NDHWC", "Conv3D",
           "AvgPool3D", [1, 2, 1, 2, 1], [1, 3, 2, 2, 1], [1, 1, 2, 1, 1])
    branch("b", [-1, 7, 6, 16], (2, 3, 16, 24), "NHWC", "Conv2D", "AvgPool",
           [1, 1, 2, 1], [1, 2, 2, 1], [1, 2, 1, 1])
    lm = _compile(tmp_path, gb.build())
    for dtype in ("bf16", "fp8"):
        calls = {(kind, len(ints)): ints for kind, _p, ints, _f in
                 emit.build_template(lm.plan, 4, dtype).calls}
        assert len(calls) == 4
        assert calls["CONV", 23] == [4, 7, 6, 16, 24, 2, 3, 1, 2, 0, 0, 7, 3,
                                     320, 0, 1, 1, 1, 4, 3, 2, 0, 2]
        assert calls["POOL", 18] == [0, 4, 2, 7, 3, 24, 2, 4, 3, 3, 2, 2, 1,
                                     2, 1, 1, 0, 0]
        assert calls["CONV", 15] == [4, 7, 6, 16, 24, 2, 3, 1, 2, 0, 0, 7, 3,
                                     128, 0]
        assert calls["POOL", 13] == [0, 4, 7, 3, 24, 4, 3, 2, 2, 2, 1, 0, 0]


def test_gemm_shortcut_and_cpad_stem(tmp_path):
    one = _compile(tmp_path, _graph(
        "Conv3D", "c", (-1, *DHW, 64), np.ones((1, 1, 1, 64, 8), np.float32),
        padding="SAME", strides=[1] * 5), "a")
    (call,) = emit.build_template(one.plan, 4, "bf16").calls
    assert call[0] == "GEMM" and call[2] == [4 * 5 * 6 * 7, 8, 64, 0]
    rgb = _compile(tmp_path, _graph(
        "Conv3D", "c", (-1, *DHW, 3), np.ones((3, 7, 7, 3, 8), np.float32),
        padding="SAME", strides=[1, 1, 2, 2, 1]), "b")
    pad, conv = emit.build_template(rgb.plan, 4, "bf16").calls
    assert pad[0] == "PAD_LAST" and pad[2] == [4 * 5 * 6 * 7, 3, 8]
    assert conv[0] == "CONV" and conv[1][0] == pad[1][1]
    assert conv[1][1][0] == ("cw", rgb.plan.ops[0].inputs[1], "cpad", 8)
    assert conv[2][3] == 8 and conv[2][13] == 3 * 7 * 7 * 8 + 40  # pad64


def test_video_resnet_fixture_cpu(tmp_path):
    lm = _compile(tmp_path, build_video_resnet())
    assert [op.kind for op in lm.plan.ops] == \
        ["conv3d", "pool3d"] + ["conv3d"] * 8 + \
        ["pool3d", "reduce", "gemm", "softmax"]    # every BN folded
    names = [c[0] for c in emit.build_template(lm.plan, 2, "bf16").calls]
    assert names.count("CONV") == 8 and names.count("GEMM") == 2
    x = (np.random.default_rng(0).standard_normal((2, 8, 32, 32, 3)) * 0.3
         ).astype(np.float32)
    probs = lm.predict({"input": x})["probs"]
    assert probs.shape == (2, 10)
    np.testing.assert_allclose(probs.sum(-1), 1.0, atol=1e-4)
