"""DepthwiseConv2dNative with depth_multiplier M > 1 (filter [R,S,C,M])
through the planner, the CPU executor, call emission and the
build_separable_cnn fixture.

Output channel k = c*M + m reads input channel c = k // M. The reference
is torch.nn.functional.conv2d(groups=C) with the filter permuted to
[C*M,1,R,S] and TF's SAME pads applied by hand (PyTorch's CPU kernels:
independent of the planner and of the numpy executor). Tolerance is the
one test_grouped_conv.py uses for the same comparison: rtol 1e-4,
atol 1e-5.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tfservingcache_amd.engine import emit  # noqa: E402
from tfservingcache_amd.engine.model import LoadedModel  # noqa: E402
from tfservingcache_amd.engine.planner import (PlanError,  # noqa: E402
                                               compile_graph)
from tfservingcache_amd.engine.savedmodel import (GraphBuilder,  # noqa: E402
                                                  read_saved_model,
                                                  write_saved_model)
from tfservingcache_amd.models import build_separable_cnn  # noqa: E402

EPS = 1.001e-5
H, W = 6, 5                 # H != W; stride 2 SAME: pad 0 on top, 1 below
RTOL, ATOL = 1e-4, 1e-5


def _compile(tmp_path, sm, name="m"):
    d = str(tmp_path / name / "1")
    write_saved_model(sm, d)
    graph_def, sigs = read_saved_model(d)
    return LoadedModel(name, 1,
                       compile_graph(graph_def, next(iter(sigs.values()))))


def _weights(C, M, R, S, seed, fused):
    rng = np.random.default_rng(seed)
    K = C * M
    p = {"w": (rng.standard_normal((R, S, C, M)) * 0.3).astype(np.float32)}
    if fused:
        p["gamma"] = (np.abs(rng.standard_normal(K)) * 0.5 + 0.5
                      ).astype(np.float32)
        p["beta"] = (rng.standard_normal(K) * 0.1).astype(np.float32)
        p["mean"] = (rng.standard_normal(K) * 0.1).astype(np.float32)
        p["var"] = (np.abs(rng.standard_normal(K)) * 0.5 + 0.5
                    ).astype(np.float32)
    return p


def _graph(C, p, strides, padding, fused, explicit=None, residual=None,
           op="DepthwiseConv2dNative", data_format="NHWC",
           dilations=None):
    """One conv node on a [-1,H,W,C] input: DepthwiseConv2dNative with
    p['w'] [R,S,C,M], or Conv2D with the same weights spelled
    [R,S,1,C*M]. Optionally + BN + Relu6, or + a residual AddV2.
    residual = (Ho, Wo)."""
    w = p["w"]
    R, S, _, M = w.shape
    K = C * M
    gb = GraphBuilder()
    f32 = gb.a_type(1)
    x = gb.placeholder("input", np.float32, [-1, H, W, C],
                       signature_name="input")
    if residual is not None:
        res = gb.placeholder("res", np.float32, [-1, *residual, K],
                             signature_name="res")
    if op == "Conv2D":
        w = w.reshape(R, S, 1, K)
    attrs = dict(T=f32, strides=gb.a_ints([1, *strides, 1]),
                 padding=gb.a_str(padding),
                 data_format=gb.a_str(data_format))
    if explicit is not None:
        pt, pb, pl, pr = explicit
        attrs["explicit_paddings"] = gb.a_ints([0, 0, pt, pb, pl, pr, 0, 0])
    if dilations is not None:
        attrs["dilations"] = gb.a_ints(dilations)
    y = gb.node(op, "dw", [x, gb.const("w", w)], **attrs)
    if fused:
        y = gb.node("FusedBatchNormV3", "bn",
                    [y] + [gb.const(n, p[n])
                           for n in ("gamma", "beta", "mean", "var")],
                    T=f32, U=f32, epsilon=gb.a_float(EPS),
                    is_training=gb.a_bool(False),
                    data_format=gb.a_str("NHWC"))
        y = gb.node("Relu6", "relu6", [y], T=f32)
    if residual is not None:
        y = gb.node("AddV2", "add", [y, res], T=f32)
    gb.mark_output("y", y)
    return gb.build()


def _same(n, k, s):
    out = -(-n // s)
    tot = max((out - 1) * s + k - n, 0)
    return tot // 2, tot - tot // 2


def _torch_ref(x, p, strides, pads, fused, res=None):
    """conv2d(groups=C) on [C*M,1,R,S]; pads = (pt, pb, pl, pr)."""
    R, S, C, M = p["w"].shape
    pt, pb, pl, pr = pads
    xt = torch.nn.functional.pad(torch.from_numpy(x).permute(0, 3, 1, 2),
                                 (pl, pr, pt, pb))
    wt = torch.from_numpy(p["w"]).reshape(R, S, C * M).permute(2, 0, 1)
    y = torch.nn.functional.conv2d(xt, wt.unsqueeze(1).contiguous(),
                                   stride=strides, groups=C)
    if fused:
        y = torch.nn.functional.batch_norm(
            y, torch.from_numpy(p["mean"]), torch.from_numpy(p["var"]),
            torch.from_numpy(p["gamma"]), torch.from_numpy(p["beta"]),
            training=False, eps=EPS)
        y = torch.clamp(y, 0.0, 6.0)
    y = y.permute(0, 2, 3, 1)
    if res is not None:
        y = y + torch.from_numpy(res)
    return y.contiguous().numpy()


def _pads_for(padding, R, S, strides):
    if padding == "SAME":
        return _same(H, R, strides[0]) + _same(W, S, strides[1])
    return (0, 0, 0, 0)


_CM = [(8, 2), (4, 4), (3, 8), (6, 3), (3, 2)]


def _x(C, seed=7, n=2):
    return np.random.default_rng(seed).standard_normal(
        (n, H, W, C)).astype(np.float32)


# -- 1. numerics -------------------------------------------------------------

@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("stride,padding", [(1, "SAME"), (2, "SAME"),
                                            (1, "VALID"), (2, "VALID")])
@pytest.mark.parametrize("C,M", _CM)
def test_depthwise_multiplier_cpu_vs_torch(tmp_path, C, M, stride, padding,
                                           fused):
    p = _weights(C, M, 3, 3, seed=C + M + stride, fused=fused)
    lm = _compile(tmp_path, _graph(C, p, (stride, stride), padding, fused))
    if fused:
        assert [op.kind for op in lm.plan.ops] == ["depthwise_conv"]
    x = _x(C)
    got = lm.predict({"input": x})["y"]
    want = _torch_ref(x, p, (stride, stride),
                      _pads_for(padding, 3, 3, (stride, stride)), fused)
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)


def test_explicit_padding(tmp_path):
    C, M = 4, 4
    pads = (2, 0, 1, 3)                         # pt, pb, pl, pr
    p = _weights(C, M, 3, 3, seed=21, fused=True)
    lm = _compile(tmp_path, _graph(C, p, (1, 2), "EXPLICIT", True,
                                   explicit=pads))
    (op,) = lm.plan.ops
    assert op.kind == "depthwise_conv" and op.params["pads"] == pads
    assert op.params["out_hw"] == ((H + 2 - 3) // 1 + 1,
                                   (W + 4 - 3) // 2 + 1)
    x = _x(C)
    got = lm.predict({"input": x})["y"]
    want = _torch_ref(x, p, (1, 2), pads, True)
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)


def test_residual_add(tmp_path):
    C, M = 6, 3
    p = _weights(C, M, 3, 3, seed=22, fused=False)
    lm = _compile(tmp_path, _graph(C, p, (2, 2), "SAME", False,
                                   residual=(3, 3)))
    assert [op.kind for op in lm.plan.ops] == ["depthwise_conv", "eltwise"]
    assert lm.plan.tensors[lm.plan.ops[1].outputs[0]].shape[1:] == \
        (3, 3, C * M)
    rng = np.random.default_rng(3)
    x = _x(C)
    res = rng.standard_normal((2, 3, 3, C * M)).astype(np.float32)
    got = lm.predict({"input": x, "res": res})["y"]
    want = _torch_ref(x, p, (2, 2), _pads_for("SAME", 3, 3, (2, 2)),
                      False, res)
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)


# -- 2. cross-lowering -------------------------------------------------------

@pytest.mark.parametrize("C,M", [(16, 2), (8, 4), (6, 3)])
def test_same_output_as_conv2d_spelling(tmp_path, C, M):
    """[R,S,C,M] read as a grouped Conv2D filter [R,S,1,C*M] goes through
    lower_conv (grouped or block-diagonal dense) and must agree: an
    independent check of the c*M + m order."""
    p = _weights(C, M, 3, 3, seed=31 + C, fused=True)
    dw = _compile(tmp_path, _graph(C, p, (2, 1), "SAME", True), name="dw")
    cv = _compile(tmp_path, _graph(C, p, (2, 1), "SAME", True,
                                   op="Conv2D"), name="cv")
    assert [op.kind for op in dw.plan.ops] == ["depthwise_conv"]
    assert [op.kind for op in cv.plan.ops] == ["conv2d"]
    x = _x(C, seed=5, n=3)
    np.testing.assert_allclose(dw.predict({"input": x})["y"],
                               cv.predict({"input": x})["y"],
                               rtol=RTOL, atol=ATOL)


# -- 3. plan shape -----------------------------------------------------------

@pytest.mark.parametrize("C,M", [(8, 2), (6, 3), (3, 8)])
def test_plan_shape(tmp_path, C, M):
    p = _weights(C, M, 3, 5, seed=4, fused=True)
    lm = _compile(tmp_path, _graph(C, p, (2, 2), "SAME", True))
    (op,) = lm.plan.ops
    K = C * M
    assert op.params["mult"] == M
    assert op.params["rsc"] == (3, 5, C)
    assert list(op.params) == ["stride", "pads", "act", "rsc", "hw",
                               "out_hw", "mult"]
    t = lm.plan.tensors
    assert t[op.inputs[1]].weight.shape == (3, 5, K)
    assert t[op.inputs[2]].weight.shape == (K,)
    assert tuple(t[op.outputs[0]].shape[1:]) == (3, 3, K)
    # BN folded over K channels in k = c*M + m order
    g = p["gamma"] / np.sqrt(p["var"] + np.float32(EPS))
    np.testing.assert_allclose(t[op.inputs[1]].weight,
                               p["w"].reshape(3, 5, K) * g, rtol=1e-6)
    np.testing.assert_allclose(t[op.inputs[2]].weight,
                               p["beta"] - p["mean"] * g, rtol=1e-5,
                               atol=1e-7)


def test_multiplier_1_params_unchanged(tmp_path):
    p = _weights(8, 1, 3, 3, seed=2, fused=False)
    lm = _compile(tmp_path, _graph(8, p, (2, 2), "SAME", False))
    (op,) = lm.plan.ops
    assert op.params == {"stride": (2, 2), "pads": (0, 1, 1, 1),
                         "act": "none", "rsc": (3, 3, 8),
                         "hw": (H, W), "out_hw": (3, 3)}
    assert list(op.params) == ["stride", "pads", "act", "rsc", "hw",
                               "out_hw"]
    assert lm.plan.tensors[op.inputs[1]].weight.shape == (3, 3, 8)
    np.testing.assert_array_equal(lm.plan.tensors[op.inputs[1]].weight,
                                  p["w"].reshape(3, 3, 8))


# -- 4. emission -------------------------------------------------------------

@pytest.mark.parametrize("C,M", [(8, 1), (8, 2), (6, 3)])
def test_emission(tmp_path, C, M):
    p = _weights(C, M, 3, 3, seed=6, fused=True)
    lm = _compile(tmp_path, _graph(C, p, (2, 1), "SAME", True))
    (op,) = lm.plan.ops
    K, n = C * M, 4
    layout = emit.blob_layout(lm.plan)
    per_dtype = []
    for dtype in ("bf16", "fp8"):
        t = emit.build_template(lm.plan, n, dtype)
        calls = [c for c in t.calls if c[0] == "DEPTHWISE"]
        assert len(calls) == 1 and len(t.calls) == 1
        _, descs, ints, floats = calls[0]
        base = [n, H, W, C, 3, 3, 2, 1, 0, 1, 3, W, 5]    # act 5 = relu6
        assert ints == (base if M == 1 else base + [M])
        assert floats == []
        # [x, w, bias, y]: every byte the kernel touches is inside the
        # workspace / the blob
        (xk, xo), (wk, wo), (bk, bo), (yk, yo) = descs
        assert xk == emit.WS and yk == emit.WS
        assert 0 <= xo and xo + n * H * W * C * 2 <= t.total_bytes
        assert 0 <= yo and yo + n * 3 * W * K * 2 <= t.total_bytes
        assert wk == ("blob",) and bk == ("blob",)
        assert wo == layout.slots[op.inputs[1]][0] * 2
        assert bo == layout.slots[op.inputs[2]][0] * 2
        assert wo % 16 == 0 and bo % 16 == 0 and xo % 16 == 0 \
            and yo % 16 == 0
        assert wo + 9 * K * 2 <= layout.total * 2
        assert bo + K * 2 <= layout.total * 2
        per_dtype.append(t.calls)
    assert per_dtype[0] == per_dtype[1]


# -- 5. rejects --------------------------------------------------------------

def test_rejects(tmp_path):
    p = _weights(4, 2, 3, 3, seed=0, fused=False)
    with pytest.raises(PlanError, match="dilated"):
        _compile(tmp_path, _graph(4, p, (1, 1), "SAME", False,
                                  dilations=[1, 2, 2, 1]), name="dil")
    with pytest.raises(PlanError, match="NHWC"):
        _compile(tmp_path, _graph(4, p, (1, 1), "SAME", False,
                                  data_format="NCHW"), name="nchw")


# -- 6. fixture --------------------------------------------------------------

def test_separable_cnn_fixture_cpu(tmp_path):
    lm = _compile(tmp_path, build_separable_cnn(image_size=32), name="sep")
    dws = [op for op in lm.plan.ops if op.kind == "depthwise_conv"]
    # (R, S, C), M, stride per block; M = 3 lands on the scalar kernel
    assert [(op.params["rsc"], op.params.get("mult", 1),
             op.params["stride"]) for op in dws] == [
        ((3, 3, 16), 2, (1, 1)), ((3, 3, 16), 4, (2, 2)),
        ((5, 5, 24), 3, (1, 1)), ((3, 3, 24), 8, (2, 2))]
    assert all(op.params["act"] == "relu6" for op in dws)
    # both identity residuals fold into their 1x1 convs
    assert sum(1 for op in lm.plan.ops
               if op.kind == "conv2d" and op.params.get("residual")) == 2
    x = (np.random.default_rng(0).standard_normal((3, 32, 32, 3)) * 0.3
         ).astype(np.float32)
    out = lm.predict({"input": x})
    assert out["probs"].shape == (3, 10) and out["logits"].shape == (3, 10)
    assert np.all(np.isfinite(out["logits"]))
    np.testing.assert_allclose(out["probs"].sum(-1), 1.0, atol=1e-4)
