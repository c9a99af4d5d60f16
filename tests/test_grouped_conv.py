"""Grouped Conv2D (ResNeXt / RegNet class) through the planner, the CPU
executor, call emission and the build_resnext fixture.

TensorFlow has no `groups` attribute: a grouped Conv2D is a Conv2D node
whose filter is [R,S,C/G,K] on a C-channel input. The reference is
torch.nn.functional.conv2d(groups=G) on the original, un-merged weights
(PyTorch's CPU kernels: independent of the planner's weight rewrite and
of the numpy executor).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tfservingcache_amd.engine import emit, planner  # noqa: E402
from tfservingcache_amd.engine.model import LoadedModel  # noqa: E402
from tfservingcache_amd.engine.planner import (PlanError,  # noqa: E402
                                               compile_graph)
from tfservingcache_amd.engine.savedmodel import (GraphBuilder,  # noqa: E402
                                                  read_saved_model,
                                                  write_saved_model)
from tfservingcache_amd.models import build_resnext  # noqa: E402


def _compile(tmp_path, sm, name="m", dense=False):
    """Write + read the SavedModel and compile it (not through the
    content-keyed plan cache: the same bytes compile under both
    lowerings here)."""
    d = str(tmp_path / name / "1")
    write_saved_model(sm, d)
    graph_def, sigs = read_saved_model(d)
    planner._Lowerer.GROUPED_CONV_DENSE = dense
    try:
        plan = compile_graph(graph_def, next(iter(sigs.values())))
    finally:
        planner._Lowerer.GROUPED_CONV_DENSE = False
    return LoadedModel(name, 1, plan)


def _weights(C, K, G, R, seed, fused):
    rng = np.random.default_rng(seed)
    p = {"w": (rng.standard_normal((R, R, C // G, K)) * 0.3
               ).astype(np.float32)}
    if fused:
        p["gamma"] = (np.abs(rng.standard_normal(K)) * 0.5 + 0.5
                      ).astype(np.float32)
        p["beta"] = (rng.standard_normal(K) * 0.1).astype(np.float32)
        p["mean"] = (rng.standard_normal(K) * 0.1).astype(np.float32)
        p["var"] = (np.abs(rng.standard_normal(K)) * 0.5 + 0.5
                    ).astype(np.float32)
    return p


EPS = 1.001e-5


def _graph(C, H, p, stride, padding, fused, tag=""):
    """Conv2D (grouped when p['w'] has fewer input channels than C),
    optionally + BN + residual Add + Relu."""
    K = p["w"].shape[3]
    gb = GraphBuilder()
    f32 = gb.a_type(1)
    x = gb.placeholder("input", np.float32, [-1, H, H, C],
                       signature_name="input")
    if fused:
        # before the conv: the planner folds a residual that is already
        # lowered
        Ho = -(-H // stride) if padding == "SAME" else \
            (H - p["w"].shape[0]) // stride + 1
        res = gb.placeholder("res", np.float32, [-1, Ho, Ho, K],
                             signature_name="res")
    y = gb.node("Conv2D", f"conv{tag}", [x, gb.const("w", p["w"])], T=f32,
                strides=gb.a_ints([1, stride, stride, 1]),
                padding=gb.a_str(padding), data_format=gb.a_str("NHWC"))
    if fused:
        y = gb.node("FusedBatchNormV3", "bn",
                    [y] + [gb.const(n, p[n])
                           for n in ("gamma", "beta", "mean", "var")],
                    T=f32, U=f32, epsilon=gb.a_float(EPS),
                    is_training=gb.a_bool(False),
                    data_format=gb.a_str("NHWC"))
        y = gb.node("AddV2", "add", [y, res], T=f32)
        y = gb.node("Relu", "relu", [y], T=f32)
    gb.mark_output("y", y)
    return gb.build()


def _torch_ref(x, p, G, stride, padding, fused, res=None):
    """conv2d(groups=G) with TF's SAME padding (extra pixel at the
    bottom/right), on the original weights."""
    R = p["w"].shape[0]
    H = x.shape[1]
    xt = torch.from_numpy(x).permute(0, 3, 1, 2)
    if padding == "SAME":
        Ho = -(-H // stride)
        tot = max((Ho - 1) * stride + R - H, 0)
        lo, hi = tot // 2, tot - tot // 2
        xt = torch.nn.functional.pad(xt, (lo, hi, lo, hi))
    wt = torch.from_numpy(p["w"]).permute(3, 2, 0, 1).contiguous()
    y = torch.nn.functional.conv2d(xt, wt, stride=stride, groups=G)
    if fused:
        y = torch.nn.functional.batch_norm(
            y, torch.from_numpy(p["mean"]), torch.from_numpy(p["var"]),
            torch.from_numpy(p["gamma"]), torch.from_numpy(p["beta"]),
            training=False, eps=EPS)
        y = torch.relu(y + torch.from_numpy(res).permute(0, 3, 1, 2))
    return y.permute(0, 2, 3, 1).numpy()


_CKG = [(32, 32, 8), (16, 48, 2), (6, 6, 2), (64, 64, 64)]


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("stride,padding", [(1, "SAME"), (2, "SAME"),
                                            (1, "VALID"), (2, "VALID")])
@pytest.mark.parametrize("C,K,G", _CKG)
def test_grouped_conv_cpu_vs_torch(tmp_path, C, K, G, stride, padding,
                                   fused):
    H = 6                   # stride 2 SAME: pad 0 on top, 1 at the bottom
    p = _weights(C, K, G, 3, seed=C + K + G + stride, fused=fused)
    lm = _compile(tmp_path, _graph(C, H, p, stride, padding, fused))
    rng = np.random.default_rng(7)
    x = rng.standard_normal((2, H, H, C)).astype(np.float32)
    feeds = {"input": x}
    res = None
    if fused:
        Ho = lm.plan.ops[-1].params["out_hw"][0]
        res = rng.standard_normal((2, Ho, Ho, K)).astype(np.float32)
        feeds["res"] = res
        assert [op.kind for op in lm.plan.ops] == ["conv2d"]
    got = lm.predict(feeds)["y"]
    want = _torch_ref(x, p, G, stride, padding, fused, res)
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5)


def _conv_op(lm):
    ops = [op for op in lm.plan.ops if op.kind == "conv2d"]
    assert len(ops) == 1
    return ops[0]


def test_merge_rule(tmp_path):
    def op_for(C, K, G, dense=False):
        p = _weights(C, K, G, 3, seed=1, fused=False)
        return _conv_op(_compile(tmp_path, _graph(C, 6, p, 1, "SAME", False),
                                 name=f"m{C}_{K}_{G}_{dense}", dense=dense))

    op = op_for(32, 32, 8)                  # Cg = Ng = 4 -> m = 4
    assert op.params["groups"] == 2
    assert op.params["rsck"] == (3, 3, 16, 32)
    assert op_for(128, 128, 32).params["groups"] == 8
    assert op_for(128, 128, 32).params["rsck"] == (3, 3, 16, 128)
    op = op_for(16, 48, 2)                  # already aligned: m = 1
    assert op.params["groups"] == 2
    assert op.params["rsck"] == (3, 3, 8, 48)
    for C, K, G in [(6, 6, 2), (64, 64, 64)]:
        op = op_for(C, K, G)
        assert "groups" not in op.params
        assert op.params["rsck"] == (3, 3, C, K)
    # forced dense lowering
    op = op_for(32, 32, 8, dense=True)
    assert "groups" not in op.params
    assert op.params["rsck"] == (3, 3, 32, 32)


def test_merged_weight_is_block_diagonal(tmp_path):
    p = _weights(32, 32, 8, 3, seed=3, fused=False)
    lm = _compile(tmp_path, _graph(32, 6, p, 1, "SAME", False))
    w = lm.plan.tensors[_conv_op(lm).inputs[1]].weight   # [3,3,16,32]
    assert w.shape == (3, 3, 16, 32)
    for k in range(32):
        g = k // 4                          # original group
        i = g % 4                           # slot inside the super-group
        np.testing.assert_array_equal(w[:, :, i * 4:(i + 1) * 4, k],
                                      p["w"][:, :, :, k])
        rest = np.delete(w[:, :, :, k], np.s_[i * 4:(i + 1) * 4], axis=2)
        assert not rest.any()


def test_dense_conv_params_unchanged(tmp_path):
    """A genuinely dense conv lowers to exactly the parent's op."""
    p = _weights(16, 24, 1, 3, seed=2, fused=False)
    op = _conv_op(_compile(tmp_path, _graph(16, 6, p, 2, "SAME", False)))
    assert op.params == {"stride": (2, 2), "pads": (0, 1, 0, 1),
                         "act": "none", "rsck": (3, 3, 16, 24),
                         "hw": (6, 6), "out_hw": (3, 3)}
    assert list(op.params) == ["stride", "pads", "act", "rsck", "hw",
                               "out_hw"]
    np.testing.assert_array_equal(
        _compile(tmp_path, _graph(16, 6, p, 2, "SAME", False),
                 name="again").plan.tensors[op.inputs[1]].weight, p["w"])


def test_forced_dense_same_cpu_output(tmp_path):
    p = _weights(32, 32, 8, 3, seed=5, fused=True)
    sm = _graph(32, 6, p, 2, "SAME", True)
    a = _compile(tmp_path, sm, name="grouped")
    b = _compile(tmp_path, sm, name="dense", dense=True)
    assert _conv_op(a).params.get("groups") == 2
    assert "groups" not in _conv_op(b).params
    rng = np.random.default_rng(11)
    feeds = {"input": rng.standard_normal((3, 6, 6, 32)).astype(np.float32),
             "res": rng.standard_normal((3, 3, 3, 32)).astype(np.float32)}
    np.testing.assert_allclose(a.predict(feeds)["y"], b.predict(feeds)["y"],
                               rtol=1e-4, atol=1e-5)


def test_plan_errors(tmp_path):
    rng = np.random.default_rng(0)
    # C % Cg != 0: 12 input channels, filter takes 8
    p = {"w": rng.standard_normal((3, 3, 8, 16)).astype(np.float32)}
    with pytest.raises(PlanError, match="conv_bad_c"):
        _compile(tmp_path, _graph(12, 6, p, 1, "SAME", False, tag="_bad_c"),
                 name="e1")
    # K % G != 0: G = 4 groups, 18 filters
    p = {"w": rng.standard_normal((3, 3, 4, 18)).astype(np.float32)}
    with pytest.raises(PlanError, match="conv_bad_k"):
        _compile(tmp_path, _graph(16, 6, p, 1, "SAME", False, tag="_bad_k"),
                 name="e2")


def _two_conv_graph(w_grouped, w_dense, C, H):
    gb = GraphBuilder()
    f32 = gb.a_type(1)
    x = gb.placeholder("input", np.float32, [-1, H, H, C],
                       signature_name="input")
    k = w_grouped.shape[0]
    y = gb.node("Conv2D", "gconv", [x, gb.const("wg", w_grouped)], T=f32,
                strides=gb.a_ints([1, 1, 1, 1]),
                padding=gb.a_str("SAME" if k == 3 else "VALID"),
                data_format=gb.a_str("NHWC"))
    y = gb.node("Relu", "relu", [y], T=f32)
    y = gb.node("Conv2D", "dconv", [y, gb.const("wd", w_dense)], T=f32,
                strides=gb.a_ints([1, 1, 1, 1]), padding=gb.a_str("SAME"),
                data_format=gb.a_str("NHWC"))
    gb.mark_output("y", y)
    return gb.build()


@pytest.mark.parametrize("k", [3, 1])
def test_emission(tmp_path, k):
    """CONV with a 16th int for the grouped conv (3x3 and 1x1), 15 ints
    for the dense conv after it."""
    rng = np.random.default_rng(k)
    C, K, G = 128, 128, 32          # 1x1, C % 64 == 0: the GEMM shortcut's
    wg = rng.standard_normal((k, k, C // G, K)).astype(np.float32)  # shape
    wd = rng.standard_normal((3, 3, K, 32)).astype(np.float32)
    lm = _compile(tmp_path, _two_conv_graph(wg, wd, C, 5), name=f"e{k}")
    gop, dop = [op for op in lm.plan.ops if op.kind == "conv2d"]
    assert gop.params["groups"] == 8 and "groups" not in dop.params
    cg = gop.params["rsck"][2]
    assert cg == 16
    for dtype in ("bf16", "fp8"):
        t = emit.build_template(lm.plan, 4, dtype)
        kinds = [c[0] for c in t.calls]
        assert set(kinds) <= emit.KINDS
        assert "GEMM" not in kinds and "PAD_LAST" not in kinds
        convs = [c for c in t.calls if c[0] == "CONV"]
        assert len(convs) == 2
        gi, di = convs[0][2], convs[1][2]
        assert len(gi) == 16 and gi[15] == 8
        assert gi[3] == C                       # the input's channel count
        assert gi[4] == K
        assert gi[13] == (k * k * cg + 63) // 64 * 64
        assert convs[0][1][1] == (("cw", gop.inputs[1]), 0)
        assert len(di) == 15
        assert di[3] == K and di[13] == (9 * K + 63) // 64 * 64


def test_resnext_fixture_cpu(tmp_path):
    sm = build_resnext(image_size=32, num_classes=10,
                       stage_blocks=(1, 1, 1, 1))
    lm = _compile(tmp_path, sm, name="rx")
    grouped = [op for op in lm.plan.ops
               if op.kind == "conv2d" and "groups" in op.params]
    # 32x4d: widths 128..1024, Cg = Ng = 4..32 -> m = 4, 2, 1, 1
    assert [(op.params["groups"], op.params["rsck"][2]) for op in grouped] \
        == [(8, 16), (16, 16), (32, 16), (32, 32)]
    x = (np.random.default_rng(0).standard_normal((2, 32, 32, 3)) * 0.3
         ).astype(np.float32)
    probs = lm.predict({"input": x})["probs"]
    assert probs.shape == (2, 10)
    assert np.all(np.isfinite(probs))
    np.testing.assert_allclose(probs.sum(-1), 1.0, atol=1e-4)
