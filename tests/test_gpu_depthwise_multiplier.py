"""Depthwise conv with a depth multiplier on the GPU: the multiplier
kernels at kernel level, the 13-int / 14-int K_DEPTHWISE forms, the
launcher's reject and build_separable_cnn end to end.

Kernel level goes through ExecPlan([(K_DEPTHWISE, ptrs, ints)]) on torch
bf16 tensors: x [N,H,W,C], w [R,S,C*M] (k = c*M + m), bias [C*M]. The
reference is torch CPU f32 conv2d(groups=C) on the same bf16-rounded
values. Tolerance, derived: bf16 x bf16 products are exact in f32, there
are at most R*S + 1 f32 adds, and the result is rounded to bf16 once
(2^-9 relative). Asserted: |got - want| <= 2^-8 * max|want|, the bound
test_gpu_grouped_conv.py uses for the same arithmetic.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tfservingcache_amd.engine.model import load_model_from_dir  # noqa: E402
from tfservingcache_amd.engine.savedmodel import (GraphBuilder,  # noqa: E402
                                                  write_saved_model)
from tfservingcache_amd.models import build_separable_cnn  # noqa: E402

SENTINEL = 1.0e30
TAIL = 64
ACT = {"none": 0, "relu": 1, "relu6": 5}


def _torch_ext():
    import torch
    from tfservingcache_amd.engine import _tfsc_engine as ext
    return torch, ext


def _same(n, k, s):
    out = -(-n // s)
    tot = max((out - 1) * s + k - n, 0)
    return out, tot // 2, tot - tot // 2


def _case(C, M, N=2, H=6, W=5, R=3, S=3, sh=1, sw=1, padding="SAME",
          seed=0):
    """bf16-rounded x, w, bias and the conv geometry. padding: "SAME",
    "VALID" or explicit (pt, pb, pl, pr)."""
    torch, _ = _torch_ext()
    g = torch.Generator().manual_seed(seed)
    K = C * M
    x = torch.randn(N, H, W, C, generator=g).to(torch.bfloat16)
    w = (torch.randn(R, S, K, generator=g) * 0.3).to(torch.bfloat16)
    b = (torch.randn(K, generator=g) * 0.5).to(torch.bfloat16)
    if padding == "SAME":
        Ho, pt, pb = _same(H, R, sh)
        Wo, pl, pr = _same(W, S, sw)
    else:
        pt, pb, pl, pr = (0, 0, 0, 0) if padding == "VALID" else padding
        Ho = (H + pt + pb - R) // sh + 1
        Wo = (W + pl + pr - S) // sw + 1
    return dict(N=N, H=H, W=W, C=C, M=M, K=K, R=R, S=S, sh=sh, sw=sw,
                pads=(pt, pb, pl, pr), Ho=Ho, Wo=Wo, x=x, w=w, b=b)


def _reference(c, act="none"):
    torch, _ = _torch_ext()
    pt, pb, pl, pr = c["pads"]
    xt = torch.nn.functional.pad(c["x"].float().permute(0, 3, 1, 2),
                                 (pl, pr, pt, pb))
    wt = c["w"].float().permute(2, 0, 1).unsqueeze(1).contiguous()
    y = torch.nn.functional.conv2d(xt, wt, c["b"].float(),
                                   stride=(c["sh"], c["sw"]), groups=c["C"])
    y = y.permute(0, 2, 3, 1)
    if act == "relu":
        y = torch.relu(y)
    elif act == "relu6":
        y = torch.clamp(y, 0.0, 6.0)
    return y.contiguous()


def _ints(c, act="none"):
    return [c["N"], c["H"], c["W"], c["C"], c["R"], c["S"], c["sh"],
            c["sw"], c["pads"][0], c["pads"][2], c["Ho"], c["Wo"], ACT[act]]


def _run(c, ints, expect_error=False):
    torch, ext = _torch_ext()
    n_out = c["N"] * c["Ho"] * c["Wo"] * c["K"]
    buf = torch.full((n_out + TAIL,), SENTINEL, dtype=torch.bfloat16,
                     device="cuda")
    x = c["x"].cuda().contiguous()
    w = c["w"].cuda().contiguous()
    b = c["b"].cuda().contiguous()
    ptrs = [x.data_ptr(), w.data_ptr(), b.data_ptr(), buf.data_ptr()]
    plan = ext.ExecPlan([(ext.K_DEPTHWISE, ptrs, ints, [])])
    if expect_error:
        with pytest.raises(RuntimeError):
            plan.run()
    else:
        plan.run()
    torch.cuda.synchronize()
    out = buf[:n_out].view(c["N"], c["Ho"], c["Wo"], c["K"]).cpu()
    return out, buf[n_out:].cpu()


def _check(c, what, act="none"):
    torch, _ = _torch_ext()
    got, tail = _run(c, _ints(c, act) + [c["M"]])
    sent = torch.tensor(SENTINEL, dtype=torch.bfloat16)
    assert not (got == sent).any(), f"unwritten output, {what}"
    assert (tail == sent).all(), f"wrote past the end, {what}"
    want = _reference(c, act)
    bound = 2.0 ** -8 * float(want.abs().max())
    err = float((got.float() - want).abs().max())
    print(f"{what}: max|err|={err:.4g} bound={bound:.4g}")
    assert err <= bound, (what, err, bound)


# (C, M) -> kernel variant, at N=2, H=6, W=5, 3x3 / 1 SAME
_VARIANT_CASES = {
    "v8_m2": (8, 2),            # k_depthwise_mult_v8<4>, 8-byte x load
    "v8_m2_c20": (20, 2),       # the same, 5 vectors per pixel
    "v8_m4": (4, 4),            # k_depthwise_mult_v8<2>, 4-byte x load
    "v8_m8": (3, 8),            # k_depthwise_mult_v8<1>, bf16 broadcast
    "v8_m16": (2, 16),          # the same, two vectors share a channel
    "scalar_m3": (6, 3),        # k_depthwise_mult_scalar: M not 2/4/8k
    "scalar_k6": (3, 2),        # k_depthwise_mult_scalar: C*M % 8 != 0
}


@pytest.mark.parametrize("name", list(_VARIANT_CASES))
def test_depthwise_multiplier_kernel_variants(name):
    C, M = _VARIANT_CASES[name]
    _check(_case(C, M, seed=len(name)), name)


# geometry on one vector variant (8, 2) and the scalar one (6, 3)
_GEOMETRY_CASES = {
    # H=6, 3x3 / 2 SAME: pad 0 on top, 1 at the bottom
    "s2_same": dict(sh=2, sw=2),
    "valid": dict(padding="VALID"),
    "sh_ne_sw": dict(sh=2, sw=1),
    "5x1": dict(R=5, S=1),              # an R/S swap reads other taps
    "explicit_pt2_pl0": dict(padding=(2, 0, 0, 1)),
}


@pytest.mark.parametrize("C,M", [(8, 2), (6, 3)])
@pytest.mark.parametrize("name", list(_GEOMETRY_CASES))
def test_depthwise_multiplier_kernel_geometry(name, C, M):
    c = _case(C, M, seed=10 + len(name), **_GEOMETRY_CASES[name])
    if name == "s2_same":
        assert c["pads"][:2] == (0, 1)
    _check(c, f"{name}_c{C}m{M}")


@pytest.mark.parametrize("act", ["relu", "relu6"])
@pytest.mark.parametrize("C,M", [(4, 4), (6, 3)])
def test_depthwise_multiplier_kernel_epilogue(act, C, M):
    c = _case(C, M, sh=2, sw=2, seed=3)
    c["x"] = c["x"] * 4.0       # exact in bf16; spreads y past [0, 6]
    # the activation must clip on both sides for the case to mean anything
    want = _reference(c)
    assert float(want.min()) < 0.0 and float(want.max()) > 6.0
    _check(c, f"{act}_c{C}m{M}", act=act)


def test_depthwise_multiplier_kernel_grid_stride():
    """4*64*64*512/8 = 1,048,576 vector items > 2048 blocks * 256
    threads: every thread runs the grid-stride loop twice."""
    c = _case(128, 4, N=4, H=64, W=64, seed=9)
    assert c["N"] * c["Ho"] * c["Wo"] * c["K"] // 8 > 2048 * 256
    _check(c, "grid_stride", act="relu")


def test_multiplier_1_same_kernels_13_and_14_ints():
    """M == 1: the 13-int form and a 14th int of 1 are bit-identical
    (vector C % 4 == 0 and scalar paths)."""
    torch, _ = _torch_ext()
    sent = torch.tensor(SENTINEL, dtype=torch.bfloat16)
    for C in (8, 6):
        c = _case(C, 1, sh=2, sw=2, seed=C)
        a, tail_a = _run(c, _ints(c, "relu6"))
        b, tail_b = _run(c, _ints(c, "relu6") + [1])
        assert (tail_a == sent).all() and (tail_b == sent).all()
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
        want = _reference(c, "relu6")
        assert float((a.float() - want).abs().max()) <= \
            2.0 ** -8 * float(want.abs().max())


def test_launcher_rejects_multiplier_0():
    torch, _ = _torch_ext()
    c = _case(8, 2, seed=1)
    got, tail = _run(c, _ints(c) + [0], expect_error=True)
    sent = torch.tensor(SENTINEL, dtype=torch.bfloat16)
    assert (got == sent).all() and (tail == sent).all()


# -- single-op graphs and build_separable_cnn: GPU vs CPU --------------------

def _gpu_model(tmp_path, sm, name="m", version=1, max_batch=8):
    from tfservingcache_amd.engine.gpu import GpuModel
    d = tmp_path / name / str(version)
    write_saved_model(sm, str(d))
    lm = load_model_from_dir(str(d), name, version)
    lm._gpu = GpuModel(lm.plan, device="cuda:0", max_batch=max_batch,
                       model_name=name, model_version=version)
    return lm


def _cpu_model(tmp_path, sm, name="mcpu", version=1):
    d = tmp_path / name / str(version)
    write_saved_model(sm, str(d))
    return load_model_from_dir(str(d), name, version)


@pytest.mark.parametrize("C,M", [(32, 2), (6, 3)])
def test_single_op_graph_gpu_vs_cpu(tmp_path, C, M):
    """Planner -> emitter -> executor for one DepthwiseConv2dNative + BN
    + Relu6, at the tolerance of test_depthwise_gpu_vs_cpu."""
    rng = np.random.default_rng(11 + C)
    gb = GraphBuilder()
    f32 = gb.a_type(1)
    K = C * M
    x_ph = gb.placeholder("input", np.float32, [-1, 14, 14, C],
                          signature_name="input")
    w = (rng.standard_normal((3, 3, C, M)) * 0.3).astype(np.float32)
    y = gb.node("DepthwiseConv2dNative", "dw", [x_ph, gb.const("w", w)],
                T=f32, strides=gb.a_ints([1, 2, 2, 1]),
                padding=gb.a_str("SAME"), data_format=gb.a_str("NHWC"))
    consts = [gb.const(n, (np.abs(rng.standard_normal(K)) * 0.5 + 0.5
                           ).astype(np.float32))
              for n in ("gamma", "beta", "mean", "var")]
    y = gb.node("FusedBatchNormV3", "bn", [y] + consts, T=f32, U=f32,
                epsilon=gb.a_float(1e-3), is_training=gb.a_bool(False),
                data_format=gb.a_str("NHWC"))
    y = gb.node("Relu6", "r6", [y], T=f32)
    gb.mark_output("y", y)
    sm = gb.build()
    gm = _gpu_model(tmp_path, sm, name=f"dwm{C}")
    try:
        cm = _cpu_model(tmp_path, sm, name=f"dwm{C}cpu")
        assert [op.kind for op in gm.plan.ops] == ["depthwise_conv"]
        x = (rng.standard_normal((3, 14, 14, C)) * 0.8).astype(np.float32)
        want = cm.predict({"input": x})["y"]
        got = gm.predict({"input": x})["y"]         # batch 3 -> bucket 4
    finally:
        gm._gpu.release()
    assert got.shape == want.shape == (3, 7, 7, K)
    print(f"max|gpu-cpu|={float(np.abs(got - want).max()):.4g}")
    np.testing.assert_allclose(got, want, rtol=0.05, atol=0.03)


PROBS_ATOL = 0.04           # test_mobilenet_v2_gpu_vs_cpu
MARGIN = 2 * PROBS_ATOL     # below it a 0.04 error may flip the argmax


def _images():
    # model seed 0, input seed 1: CPU top-2 margins 0.16, 0.13, 0.30, 0.30
    return (np.random.default_rng(1).standard_normal((4, 32, 32, 3)) * 0.5
            ).astype(np.float32)


def _compare_probs(got, want):
    top2 = np.sort(want["probs"], axis=-1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > MARGIN
    print(f"max|gpu-cpu| probs="
          f"{float(np.abs(got['probs'] - want['probs']).max()):.4g} "
          f"margins={np.round(top2[:, 1] - top2[:, 0], 3)}")
    np.testing.assert_allclose(got["probs"], want["probs"],
                               atol=PROBS_ATOL)
    assert np.all(np.isfinite(got["logits"]))
    assert (got["probs"].argmax(1)[clear] ==
            want["probs"].argmax(1)[clear]).all()
    return clear


def test_separable_cnn_gpu_vs_cpu(tmp_path):
    sm = build_separable_cnn(image_size=32)
    gm = _gpu_model(tmp_path, sm, name="sep")
    try:
        cm = _cpu_model(tmp_path, sm, name="sepcpu")
        assert sorted(op.params.get("mult", 1) for op in gm.plan.ops
                      if op.kind == "depthwise_conv") == [2, 3, 4, 8]
        x = _images()
        for batch in (4, 3):                    # 3 -> bucket 4
            feeds = {"input": x[:batch]}
            want = cm.predict(feeds)
            got = gm.predict(feeds)
            again = gm.predict(feeds)           # graph replay
            assert got["probs"].shape == (batch, 10)
            clear = _compare_probs(got, want)
            if batch == 4:
                # the seed is chosen so the CPU executor alone gives
                # argmax something to check
                assert int(clear.sum()) >= 3
            np.testing.assert_array_equal(again["probs"], got["probs"])
            np.testing.assert_array_equal(again["logits"], got["logits"])
        ctxs = [c for lst in gm._gpu._contexts.values() for c in lst]
        assert any(c.captured and c.exec_plan.has_graph() for c in ctxs)
    finally:
        gm._gpu.release()


def test_separable_cnn_template_context_and_capture_only_prewarm(tmp_path):
    """A second model loaded from the same SavedModel shares the plan:
    its context comes from the cached call template (14-int DEPTHWISE
    calls included) and is prewarmed by graph capture alone."""
    from tfservingcache_amd.engine.gpu import GpuModel
    sm = build_separable_cnn(image_size=32)
    gm = _gpu_model(tmp_path, sm, name="sep_t")
    gm2 = None
    try:
        cm = _cpu_model(tmp_path, sm, name="sep_tcpu")
        x = _images()
        first = gm.predict({"input": x})        # registers the template
        gm2 = load_model_from_dir(str(tmp_path / "sep_t" / "1"),
                                  "sep_t2", 1)
        assert gm2.plan is gm.plan
        gm2._gpu = GpuModel(gm2.plan, device="cuda:0", max_batch=8,
                            model_name="sep_t2", model_version=1)
        gm2._gpu.prewarm(4, limit=1)
        ctxs = [c for lst in gm2._gpu._contexts.values() for c in lst]
        assert ctxs and all(getattr(c, "_from_template", False) and
                            c.captured and c.exec_plan.has_graph()
                            for c in ctxs)
        second = gm2.predict({"input": x})
        want = cm.predict({"input": x})
    finally:
        gm._gpu.release()
        if gm2 is not None and getattr(gm2, "_gpu", None) is not None:
            gm2._gpu.release()
    _compare_probs(second, want)
    np.testing.assert_allclose(second["probs"], first["probs"], rtol=1e-6)
