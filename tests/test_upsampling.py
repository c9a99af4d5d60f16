"""Upsampling decoders on the CPU path: ResizeNearestNeighbor,
ResizeBilinear and Conv2DBackpropInput through planner + CPU executor.

Numerics compare `predict` against naive loops written here (not the
executor's code) and, where torch has the mode, against
torch.nn.functional. Nearest is exact; everything else uses
rtol=1e-4, atol=1e-5 (the tolerance of tests/test_op_coverage.py).
"""
import math

import numpy as np
import pytest

from tfservingcache_amd.engine.model import load_model_from_dir
from tfservingcache_amd.engine.planner import PlanError
from tfservingcache_amd.engine.savedmodel import (GraphBuilder,
                                                  write_saved_model)
from tfservingcache_amd.models import build_unet

RTOL, ATOL = 1e-4, 1e-5


def _load(tmp_path, sm, name="m"):
    d = str(tmp_path / name / "1")
    write_saved_model(sm, d)
    return load_model_from_dir(d, name, 1)


# -- resize ------------------------------------------------------------------

_F = np.float32


def _scale(n_in, n_out, align):
    if align and n_out > 1:
        return _F(n_in - 1) / _F(n_out - 1)
    return _F(n_in) / _F(n_out)


def _naive_resize(x, out_hw, mode, align, half):
    """TF's resize kernels as direct loops, coordinates in f32."""
    N, H, W, C = x.shape
    Ho, Wo = out_hw
    hs, ws = _scale(H, Ho, align), _scale(W, Wo, align)

    def nearest(d, s, n):
        src = (_F(d) + _F(0.5)) * s if half else _F(d) * s
        # roundf = floor(src + 0.5) for src >= 0, exact in f64
        i = math.floor(float(src) + 0.5) if align else math.floor(float(src))
        return min(max(i, 0), n - 1)

    def bilinear(d, s, n):
        src = (_F(d) + _F(0.5)) * s - _F(0.5) if half else _F(d) * s
        fl = math.floor(float(src))
        return (max(fl, 0), min(math.ceil(float(src)), n - 1),
                _F(src - _F(fl)))

    y = np.zeros((N, Ho, Wo, C), np.float32)
    for ho in range(Ho):
        for wo in range(Wo):
            if mode == "nearest":
                y[:, ho, wo] = x[:, nearest(ho, hs, H), nearest(wo, ws, W)]
                continue
            y0, y1, ly = bilinear(ho, hs, H)
            x0, x1, lx = bilinear(wo, ws, W)
            top = x[:, y0, x0] + (x[:, y0, x1] - x[:, y0, x0]) * lx
            bot = x[:, y1, x0] + (x[:, y1, x1] - x[:, y1, x0]) * lx
            y[:, ho, wo] = top + (bot - top) * ly
    return y


def _resize_graph(in_hw, out_hw, mode, align, half, C=3):
    gb = GraphBuilder()
    f32 = gb.a_type(1)
    x = gb.placeholder("input", np.float32, [-1, in_hw[0], in_hw[1], C],
                       signature_name="input")
    size = gb.const("size", np.array(out_hw, np.int32))
    op = "ResizeNearestNeighbor" if mode == "nearest" else "ResizeBilinear"
    y = gb.node(op, "resize", [x, size], T=f32,
                align_corners=gb.a_bool(align),
                half_pixel_centers=gb.a_bool(half))
    gb.mark_output("y", y)
    return gb.build()


_SIZES = [((5, 7), (10, 14)), ((5, 7), (7, 9)), ((9, 6), (4, 3)),
          ((4, 4), (1, 1))]
_FLAGS = [(False, False), (True, False), (False, True)]  # (align, half)
# torch.nn.functional.interpolate equivalents, where they exist
_TORCH_MODE = {
    ("nearest", False, False): dict(mode="nearest"),
    ("nearest", False, True): dict(mode="nearest-exact"),
    ("bilinear", False, True): dict(mode="bilinear", align_corners=False),
    ("bilinear", True, False): dict(mode="bilinear", align_corners=True),
}


@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
@pytest.mark.parametrize("align,half", _FLAGS)
def test_resize_numerics_vs_naive_and_torch(tmp_path, mode, align, half):
    import torch
    rng = np.random.default_rng(7)
    for k, (in_hw, out_hw) in enumerate(_SIZES):
        model = _load(tmp_path, _resize_graph(in_hw, out_hw, mode, align,
                                              half), name=f"r{k}")
        assert [op.kind for op in model.plan.ops] == ["resize"]
        p = model.plan.ops[0].params
        assert (p["mode"], p["align_corners"], p["half_pixel_centers"],
                tuple(p["in_hw"]), tuple(p["out_hw"])) == \
            (mode, align, half, in_hw, out_hw)
        x = rng.standard_normal((2,) + in_hw + (3,)).astype(np.float32)
        got = model.predict({"input": x})["y"]
        assert got.shape == (2,) + out_hw + (3,)
        want = _naive_resize(x, out_hw, mode, align, half)
        kw = _TORCH_MODE.get((mode, align, half))
        refs = [want]
        if kw is not None:
            t = torch.nn.functional.interpolate(
                torch.from_numpy(x).permute(0, 3, 1, 2), size=out_hw, **kw)
            refs.append(t.permute(0, 2, 3, 1).numpy())
        for ref in refs:
            if mode == "nearest":
                np.testing.assert_array_equal(got, ref)
            else:
                np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL)


def test_resize_same_size_aliases_input(tmp_path):
    model = _load(tmp_path, _resize_graph((5, 7), (5, 7), "bilinear",
                                          False, True))
    assert model.plan.ops == []
    x = np.random.default_rng(1).standard_normal(
        (2, 5, 7, 3)).astype(np.float32)
    np.testing.assert_array_equal(model.predict({"input": x})["y"], x)


# -- Conv2DBackpropInput -----------------------------------------------------

def _fwd_pads(h, R, stride, padding, H):
    if padding == "SAME":
        return max((h - 1) * stride + R - H, 0) // 2
    return 0


def _naive_deconv(x, w, stride, padding, H):
    """The definition, as a scatter:
    y[n, i*s-pt+r, j*s-pl+q, co] += x[n,i,j,ci] * w[r,q,co,ci]."""
    N, h, _, Cin = x.shape
    R, S, Cout, _ = w.shape
    pt = _fwd_pads(h, R, stride, padding, H)
    y = np.zeros((N, H, H, Cout), np.float64)
    xd, wd = x.astype(np.float64), w.astype(np.float64)
    for i in range(h):
        for j in range(h):
            for r in range(R):
                for q in range(S):
                    oy, ox = i * stride - pt + r, j * stride - pt + q
                    if 0 <= oy < H and 0 <= ox < H:
                        y[:, oy, ox] += xd[:, i, j] @ wd[r, q].T
    return y.astype(np.float32)


def _deconv_graph(h, R, stride, padding, H, w, tail=(), sizes="const",
                  residual=False, **attrs):
    """x [B,h,h,Cin] -> Conv2DBackpropInput -> tail ops. sizes: "const"
    (a literal [-1,H,H,Cout]) or "shape" (Keras: Shape -> StridedSlice
    -> Pack)."""
    Cout, Cin = w.shape[2], w.shape[3]
    gb = GraphBuilder()
    f32, i32 = gb.a_type(1), gb.a_type(3)
    x = gb.placeholder("input", np.float32, [-1, h, h, Cin],
                       signature_name="input")
    skip = None
    if residual:
        skip = gb.placeholder("skip", np.float32, [-1, H, H, Cout],
                              signature_name="skip")
    if sizes == "const":
        sz = gb.const("sizes", np.array([-1, H, H, Cout], np.int32))
    else:
        shp = gb.node("Shape", "shape", [x], T=f32, out_type=i32)
        b = gb.node("StridedSlice", "batch",
                    [shp, gb.const("ss_b", np.array([0], np.int32)),
                     gb.const("ss_e", np.array([1], np.int32)),
                     gb.const("ss_s", np.array([1], np.int32))],
                    T=i32, Index=i32, shrink_axis_mask=gb.a_int(1))
        sz = gb.node("Pack", "sizes",
                     [b, gb.const("oh", np.int32(H)),
                      gb.const("ow", np.int32(H)),
                      gb.const("oc", np.int32(Cout))],
                     T=i32, N=gb.a_int(4), axis=gb.a_int(0))
    kw = dict(strides=gb.a_ints([1, stride, stride, 1]),
              padding=gb.a_str(padding), data_format=gb.a_str("NHWC"))
    kw.update(attrs)
    y = gb.node("Conv2DBackpropInput", "deconv", [sz, gb.const("w", w), x],
                T=f32, **kw)
    if residual:
        y = gb.node("AddV2", "add", [y, skip], T=f32)
    for op in tail:
        if op == "BiasAdd":
            y = gb.node("BiasAdd", "bias", [y, gb.const(
                "b", np.linspace(-0.5, 0.5, Cout).astype(np.float32))],
                T=f32)
        else:
            y = gb.node(op, op.lower(), [y], T=f32)
    gb.mark_output("y", y)
    return gb.build()


# (h, R, stride, padding, H)
_DECONV_CASES = [(5, 3, 2, "SAME", 10), (5, 3, 2, "SAME", 9),
                 (4, 2, 2, "VALID", 8), (4, 3, 2, "VALID", 9),
                 (4, 3, 2, "VALID", 10), (3, 4, 2, "SAME", 6),
                 (5, 3, 1, "SAME", 5), (3, 5, 3, "SAME", 9)]
CIN, COUT = 3, 4


def _deconv_data(h, R, seed=0):
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((R, R, COUT, CIN)) * 0.3).astype(np.float32)
    x = rng.standard_normal((2, h, h, CIN)).astype(np.float32)
    return w, x


@pytest.mark.parametrize("h,R,stride,padding,H", _DECONV_CASES)
def test_conv_transpose_numerics_vs_scatter(tmp_path, h, R, stride,
                                            padding, H):
    w, x = _deconv_data(h, R, seed=h * 10 + R)
    model = _load(tmp_path, _deconv_graph(h, R, stride, padding, H, w))
    got = model.predict({"input": x})["y"]
    assert got.shape == (2, H, H, COUT)
    np.testing.assert_allclose(got, _naive_deconv(x, w, stride, padding, H),
                               rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("h,R,stride,padding,H",
                         [(5, 3, 2, "SAME", 10), (4, 3, 2, "VALID", 9)])
def test_conv_transpose_vs_torch(tmp_path, h, R, stride, padding, H):
    import torch
    w, x = _deconv_data(h, R, seed=3)
    model = _load(tmp_path, _deconv_graph(h, R, stride, padding, H, w))
    got = model.predict({"input": x})["y"]
    full = torch.nn.functional.conv_transpose2d(
        torch.from_numpy(x).permute(0, 3, 1, 2),
        torch.from_numpy(w).permute(3, 2, 0, 1), stride=stride)
    pt = _fwd_pads(h, R, stride, padding, H)
    want = full[:, :, pt:pt + H, pt:pt + H].permute(0, 2, 3, 1).numpy()
    assert want.shape == got.shape
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)


def _kinds(model):
    return [op.kind for op in model.plan.ops]


def test_conv_transpose_plan_shapes(tmp_path):
    w2, x2 = _deconv_data(4, 2)
    w3, x3 = _deconv_data(5, 3)
    a = _load(tmp_path, _deconv_graph(4, 2, 2, "VALID", 8, w2), name="a")
    assert _kinds(a) == ["gemm", "transpose"]
    assert a.plan.ops[1].params["perm"] == [0, 1, 3, 2, 4, 5]
    b = _load(tmp_path, _deconv_graph(5, 3, 2, "SAME", 10, w3), name="b")
    assert _kinds(b) == ["zero_insert", "conv2d"]

    tail = ("BiasAdd", "Relu")
    bias = np.linspace(-0.5, 0.5, COUT).astype(np.float32)
    a2 = _load(tmp_path, _deconv_graph(4, 2, 2, "VALID", 8, w2, tail=tail),
               name="a2")
    assert _kinds(a2) == ["gemm", "transpose"]
    assert a2.plan.ops[0].params["act"] == "relu"
    np.testing.assert_allclose(
        a2.predict({"input": x2})["y"],
        np.maximum(_naive_deconv(x2, w2, 2, "VALID", 8) + bias, 0.0),
        rtol=RTOL, atol=ATOL)
    b2 = _load(tmp_path, _deconv_graph(5, 3, 2, "SAME", 10, w3, tail=tail),
               name="b2")
    assert _kinds(b2) == ["zero_insert", "conv2d"]
    assert b2.plan.ops[1].params["act"] == "relu"
    np.testing.assert_allclose(
        b2.predict({"input": x3})["y"],
        np.maximum(_naive_deconv(x3, w3, 2, "SAME", 10) + bias, 0.0),
        rtol=RTOL, atol=ATOL)


def test_conv_transpose_residual_takes_general_lowering(tmp_path):
    w, x = _deconv_data(4, 2)
    m = _load(tmp_path, _deconv_graph(4, 2, 2, "VALID", 8, w,
                                      residual=True, tail=("Relu",)))
    assert _kinds(m) == ["zero_insert", "conv2d"]
    assert m.plan.ops[1].params.get("residual") is True
    assert m.plan.ops[1].params["act"] == "relu"
    skip = np.random.default_rng(5).standard_normal(
        (2, 8, 8, COUT)).astype(np.float32)
    got = m.predict({"input": x, "skip": skip})["y"]
    want = np.maximum(_naive_deconv(x, w, 2, "VALID", 8) + skip, 0.0)
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)


# -- integer shape folding ---------------------------------------------------

@pytest.mark.parametrize("h,R,stride,padding,H",
                         [(4, 2, 2, "VALID", 8), (5, 3, 2, "SAME", 10)])
def test_input_sizes_from_shape_arithmetic_folds(tmp_path, h, R, stride,
                                                 padding, H):
    w, x = _deconv_data(h, R)
    lit = _load(tmp_path, _deconv_graph(h, R, stride, padding, H, w),
                name="lit")
    dyn = _load(tmp_path, _deconv_graph(h, R, stride, padding, H, w,
                                        sizes="shape"), name="dyn")
    assert _kinds(dyn) == _kinds(lit)
    np.testing.assert_array_equal(dyn.predict({"input": x})["y"],
                                  lit.predict({"input": x})["y"])


def test_resize_size_from_shape_times_const_folds(tmp_path):
    """UpSampling2D: size = StridedSlice(Shape(x))[1:3] * [2, 2]."""
    gb = GraphBuilder()
    f32, i32 = gb.a_type(1), gb.a_type(3)
    x = gb.placeholder("input", np.float32, [-1, 5, 7, 3],
                       signature_name="input")
    shp = gb.node("Shape", "shape", [x], T=f32, out_type=i32)
    hw = gb.node("StridedSlice", "hw",
                 [shp, gb.const("b", np.array([1], np.int32)),
                  gb.const("e", np.array([3], np.int32)),
                  gb.const("s", np.array([1], np.int32))],
                 T=i32, Index=i32)
    size = gb.node("Mul", "size",
                   [hw, gb.const("two", np.array([2, 2], np.int32))], T=i32)
    y = gb.node("ResizeNearestNeighbor", "up", [x, size], T=f32,
                half_pixel_centers=gb.a_bool(True))
    gb.mark_output("y", y)
    model = _load(tmp_path, gb.build())
    assert _kinds(model) == ["resize"]
    assert tuple(model.plan.ops[0].params["out_hw"]) == (10, 14)
    xv = np.random.default_rng(2).standard_normal(
        (2, 5, 7, 3)).astype(np.float32)
    np.testing.assert_array_equal(
        model.predict({"input": xv})["y"],
        xv.repeat(2, axis=1).repeat(2, axis=2))


# -- loud rejects ------------------------------------------------------------

def _placeholder_size_graph():
    gb = GraphBuilder()
    f32 = gb.a_type(1)
    x = gb.placeholder("input", np.float32, [-1, 5, 7, 3],
                       signature_name="input")
    size = gb.placeholder("size", np.int32, [2], signature_name="size")
    y = gb.node("ResizeBilinear", "resize", [x, size], T=f32)
    gb.mark_output("y", y)
    return gb.build()


def _w():
    return _deconv_data(5, 3)[0]


_REJECTS = {
    "placeholder_size": _placeholder_size_graph,
    "both_resize_flags": lambda: _resize_graph((5, 7), (10, 14), "bilinear",
                                               True, True),
    "nchw": lambda: _deconv_graph(
        5, 3, 2, "SAME", 10, _w(),
        data_format=GraphBuilder.a_str("NCHW")),
    "dilations": lambda: _deconv_graph(
        5, 3, 2, "SAME", 10, _w(),
        dilations=GraphBuilder.a_ints([1, 2, 2, 1])),
    "inconsistent_input_sizes": lambda: _deconv_graph(5, 3, 2, "SAME", 12,
                                                      _w()),
    "explicit_padding": lambda: _deconv_graph(
        5, 3, 2, "EXPLICIT", 10, _w(),
        explicit_paddings=GraphBuilder.a_ints([0, 0, 1, 1, 1, 1, 0, 0])),
}


@pytest.mark.parametrize("case", sorted(_REJECTS))
def test_loud_rejects(tmp_path, case):
    with pytest.raises(PlanError):
        _load(tmp_path, _REJECTS[case]())


# -- build_unet ---------------------------------------------------------------

@pytest.mark.parametrize("upsample", ["deconv", "nearest", "bilinear"])
def test_unet_serves_cpu(tmp_path, upsample):
    model = _load(tmp_path, build_unet(image_size=32, upsample=upsample))
    kinds = _kinds(model)
    assert "bn_act" not in kinds            # every BN folded
    if upsample == "deconv":
        assert kinds.count("zero_insert") == 1
        assert kinds.count("transpose") >= 1
    else:
        assert kinds.count("resize") == 2
        assert {op.params["mode"] for op in model.plan.ops
                if op.kind == "resize"} == {upsample}
    x = (np.random.default_rng(0).standard_normal((2, 32, 32, 3))
         * 0.5).astype(np.float32)
    out = model.predict({"input": x})
    assert out["probs"].shape == (2, 32, 32, 4)
    assert np.all(np.isfinite(out["probs"]))
    np.testing.assert_allclose(out["probs"].sum(-1), 1.0, atol=1e-5)
