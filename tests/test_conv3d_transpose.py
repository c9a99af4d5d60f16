"""Conv3DBackpropInputV2 through the planner, the CPU executor and call
emission. The reference is torch float64 conv_transpose3d, cropped at the
forward conv's low pads and zero-padded at the high end where it is shorter.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tfservingcache_amd.engine import emit
from tfservingcache_amd.engine.planner import PlanError
from tfservingcache_amd.engine.savedmodel import GraphBuilder
from tfservingcache_amd.models import build_unet3d
from test_conv3d import EPS, _compile, geometry

DHW, CI, CO = (3, 4, 5), 4, 6


def reference(x, w, stride, out_dhw, pads):
    """x [N,D,H,W,Ci], w [T,R,S,Co,Ci] (float64) -> y [N,*out_dhw,Co]."""
    full = F.conv_transpose3d(x.permute(0, 4, 1, 2, 3),
                              w.permute(4, 3, 0, 1, 2), stride=stride)
    short = [max(lo + o - n, 0) for lo, o, n in
             zip(pads, out_dhw, full.shape[2:])]
    full = F.pad(full, (0, short[2], 0, short[1], 0, short[0]))
    (pf, pt, pl), (Do, Ho, Wo) = pads, out_dhw
    return full[:, :, pf:pf + Do, pt:pt + Ho, pl:pl + Wo].permute(
        0, 2, 3, 4, 1)


def _graph(out_dhw, w, in_shape=(-1, *DHW, CI), sizes=None, bn=None,
           **attrs):
    # one Conv3DBackpropInputV2 (optionally + BN + residual + Relu)
    gb = GraphBuilder()
    f32 = gb.a_type(1)
    x = gb.placeholder("input", np.float32, list(in_shape),
                       signature_name="input")
    if sizes is None:
        sizes = gb.const("sizes", np.array([1, *out_dhw, w.shape[3]],
                                           np.int32))
    elif sizes == "fed":
        sizes = gb.placeholder("sizes", np.int32, [5], signature_name="sizes")
    else:
        sizes = gb.const("sizes", np.array(sizes, np.int32))
    if bn is not None:
        r = gb.placeholder("res", np.float32, [-1, *out_dhw, w.shape[3]],
                           signature_name="res")
    attrs.setdefault("data_format", "NDHWC")
    y = gb.node("Conv3DBackpropInputV2", "n_e", [sizes, gb.const("w", w), x],
                T=f32, **{k: gb.a_str(v) if isinstance(v, str)
                          else gb.a_ints(v) for k, v in attrs.items()})
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


# (filter, stride, padding, out_dhw or None for the forward conv's largest)
_CASES = {
    "k3_s2_same": ((3, 3, 3), (2, 2, 2), "SAME", None),
    "k3_s2_same_odd": ((3, 3, 3), (2, 2, 2), "SAME", (5, 7, 9)),
    "k2_s2_valid": ((2, 2, 2), (2, 2, 2), "VALID", None),
    "k3_s2_valid_slack": ((3, 3, 3), (2, 2, 2), "VALID", (8, 10, 12)),
    "k1x2x2_s2_empty_phase": ((1, 2, 2), (2, 2, 2), "VALID", None),
    "k2x3x4_s212_same": ((2, 3, 4), (2, 1, 2), "SAME", None),
    "k3_s1_same": ((3, 3, 3), (1, 1, 1), "SAME", None),
}


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", list(_CASES))
def test_conv3d_transpose_cpu_vs_torch(tmp_path, name, fused):
    trs, stride, padding, out_dhw = _CASES[name]
    if out_dhw is None:     # SAME: D*s; VALID: (D-1)*s + T
        out_dhw = tuple(n * s if padding == "SAME" else (n - 1) * s + k
                        for n, s, k in zip(DHW, stride, trs))
    geom = geometry(out_dhw, trs, stride, padding)
    assert tuple(o for o, _, _ in geom) == DHW      # the case is consistent
    pads = tuple(lo for _, lo, _ in geom)
    rng = np.random.default_rng(len(name))
    w = (rng.standard_normal((*trs, CO, CI)) * 0.3).astype(np.float32)
    x = rng.standard_normal((2, *DHW, CI)).astype(np.float32)
    want = reference(torch.from_numpy(x).double(),
                     torch.from_numpy(w).double(), stride, out_dhw,
                     pads).numpy()
    feeds, bn = {"input": x}, None
    if fused:
        bn = [(np.abs(rng.standard_normal(CO)) * 0.5 + 0.5 if i in (0, 3)
               else rng.standard_normal(CO) * 0.1).astype(np.float32)
              for i in range(4)]                # gamma, beta, mean, var
        gamma, beta, mean, var = (v.astype(np.float64) for v in bn)
        feeds["res"] = rng.standard_normal((2, *out_dhw, CO)).astype(
            np.float32)
        want = np.maximum((want - mean) / np.sqrt(var + EPS) * gamma + beta
                          + feeds["res"], 0.0)
    lm = _compile(tmp_path, _graph(out_dhw, w, bn=bn, padding=padding,
                                   strides=[1, *stride, 1]))
    (op,) = lm.plan.ops                 # BN, add and relu folded
    assert op.kind == "conv3d_transpose" and op.params["pads"] == pads
    np.testing.assert_allclose(lm.predict(feeds)["y"], want, rtol=1e-4,
                               atol=1e-5)


def test_emission_24_int_form(tmp_path):
    w = np.ones((3, 2, 3, 24, 16), np.float32)
    lm = _compile(tmp_path, _graph((6, 4, 10), w, in_shape=(-1, 3, 4, 5, 16),
                                   padding="SAME", strides=[1, 2, 1, 2, 1]))
    (call,) = emit.build_template(lm.plan, 4, "bf16").calls
    # 18 taps of 16 channels; the last phase starts at k = 256 (16 taps) and
    # its K tile ends at 320: a row of 20 taps
    assert call[0] == "CONV" and call[2] == [
        4, 4, 5, 16, 24, 2, 3, 1, 2, 0, 0, 4, 10, 320, 0, 1, 1, 1, 3, 3, 2,
        0, 6, 1]
    # C = 12 -> 16 through PAD_LAST and the cpad weight. 2x2x2 / 2: eight
    # one-tap phases; the last starts at k = 112 and its tile ends at 176,
    # so the row has 11 taps (3 of zeros)
    w = np.ones((2, 2, 2, 8, 12), np.float32)
    rgb = _compile(tmp_path, _graph((6, 8, 10), w, in_shape=(-1, 3, 4, 5, 12),
                                    padding="VALID", strides=[1, 2, 2, 2, 1]),
                   "b")
    assert rgb.plan.tensors[rgb.plan.ops[0].inputs[1]].shape == (11, 1, 12, 8)
    pad, conv = emit.build_template(rgb.plan, 2, "bf16").calls
    assert pad[0] == "PAD_LAST" and pad[2] == [2 * 3 * 4 * 5, 12, 16]
    assert conv[0] == "CONV" and conv[1][0] == pad[1][1]
    assert conv[1][1][0] == ("cw", rgb.plan.ops[0].inputs[1], "cpad", 16)
    assert conv[2] == [2, 4, 5, 16, 8, 2, 2, 2, 2, 0, 0, 8, 10, 192, 0, 1, 1,
                       1, 3, 2, 2, 0, 6, 1]


_W = np.ones((3, 3, 3, CO, CI), np.float32)
_OUT = tuple(2 * n for n in DHW)
_S2 = dict(padding="SAME", strides=[1, 2, 2, 2, 1])
_PLAN_ERRORS = {
    "ncdhw": dict(_S2, data_format="NCDHW"),
    "dilated": dict(_S2, dilations=[1, 2, 2, 2, 1]),
    "sizes_not_const": dict(_S2, sizes="fed"),
    "sizes_inconsistent": dict(_S2, sizes=[1, 6, 8, 12, CO]),
    "channel_mismatch": dict(_S2, in_shape=(-1, *DHW, CI + 1)),
}


@pytest.mark.parametrize("name", list(_PLAN_ERRORS))
def test_plan_errors_name_the_node(tmp_path, name):
    with pytest.raises(PlanError, match="n_e"):
        _compile(tmp_path, _graph(_OUT, _W, **_PLAN_ERRORS[name]))


def test_unet3d_fixture_cpu(tmp_path):
    lm = _compile(tmp_path, build_unet3d())
    kinds = [op.kind for op in lm.plan.ops]
    assert kinds.count("conv3d_transpose") == 2 and \
        kinds.count("conv3d") == 6 and kinds.count("pool3d") == 2
    x = (np.random.default_rng(0).standard_normal((2, 8, 16, 16, 3)) * 0.3
         ).astype(np.float32)
    probs = lm.predict({"input": x})["probs"]
    assert probs.shape == (2, 8, 16, 16, 4)
    np.testing.assert_allclose(probs.sum(-1), 1.0, atol=1e-4)
