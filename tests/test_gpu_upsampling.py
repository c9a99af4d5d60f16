"""Upsampling decoders on the GPU: the resize and zero-insert kernels,
both transposed-conv lowerings and build_unet.

Resize runs at kernel level through ExecPlan([(K_RESIZE, ...)]) on torch
bf16 tensors against the CPU executor's f32 resize applied to the same
bf16 values. Nearest must be bit-identical. Bilinear tolerance, derived:
the result is a convex combination of inputs, so it is bounded by
max|x|, and it is rounded to bf16 once (2^-9 relative). Asserted:
atol = 2^-8 * max|x|, rtol = 0 — twice the bound, for the f32 lerp
weights.

Transposed convs and the U-Net compare the GPU engine with the CPU
executor at the tolerances of tests/test_gpu_engine.py.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tfservingcache_amd.engine.executor_cpu import _resize  # noqa: E402
from tfservingcache_amd.engine.model import load_model_from_dir  # noqa: E402
from tfservingcache_amd.engine.savedmodel import (GraphBuilder,  # noqa: E402
                                                  write_saved_model)
from tfservingcache_amd.models import build_unet  # noqa: E402


def _torch_ext():
    import torch
    from tfservingcache_amd.engine import _tfsc_engine as ext
    return torch, ext


def _gpu_model(tmp_path, sm, name="m", version=1, max_batch=64):
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


# -- resize, kernel level ----------------------------------------------------

_SIZES = [((5, 7), (10, 14)), ((5, 7), (7, 9)), ((9, 6), (4, 3)),
          ((4, 4), (1, 1))]
_CHANNELS = [8, 24, 6]      # one vector group, three, the scalar path
SENTINEL = 1.0e30           # randn inputs never get near it
TAIL = 64


def _run_resize(x, out_hw, mode, align, half):
    """Returns (out [N,Ho,Wo,C], tail): the output buffer is pre-filled
    with SENTINEL and allocated TAIL elements too long."""
    torch, ext = _torch_ext()
    N, H, W, C = x.shape
    Ho, Wo = out_hw
    n_out = N * Ho * Wo * C
    buf = torch.full((n_out + TAIL,), SENTINEL, dtype=torch.bfloat16,
                     device="cuda")
    ext.ExecPlan([(ext.K_RESIZE, [x.data_ptr(), buf.data_ptr()],
                   [N, H, W, C, Ho, Wo, 1 if mode == "bilinear" else 0,
                    int(align), int(half)], [])]).run()
    torch.cuda.synchronize()
    return buf[:n_out].view(N, Ho, Wo, C).cpu(), buf[n_out:].cpu()


@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
@pytest.mark.parametrize("align,half", [(False, False), (True, False),
                                        (False, True)])
def test_resize_kernel(mode, align, half):
    torch, _ = _torch_ext()
    g = torch.Generator().manual_seed(17)
    sent = torch.tensor(SENTINEL, dtype=torch.bfloat16)
    for in_hw, out_hw in _SIZES:
        for C in _CHANNELS:
            x = torch.randn((2,) + in_hw + (C,), generator=g).to(
                torch.bfloat16)
            got, tail = _run_resize(x.cuda().contiguous(), out_hw, mode,
                                    align, half)
            what = f"{in_hw}->{out_hw} C={C}"
            assert not (got == sent).any(), f"unwritten output, {what}"
            assert (tail == sent).all(), f"wrote past the end, {what}"
            want = torch.from_numpy(
                _resize(x.float().numpy(), out_hw, mode, align, half))
            if mode == "nearest":
                # a gather of bf16 values: exact
                assert torch.equal(got, want.to(torch.bfloat16)), what
                continue
            atol = 2.0 ** -8 * float(x.float().abs().max())
            err = float((got.float() - want).abs().max())
            print(f"{what}: max|err|={err:.4g} atol={atol:.4g}")
            assert err <= atol, (what, err, atol)


def test_resize_launcher_rejects_bad_arguments():
    torch, ext = _torch_ext()
    x = torch.zeros(2 * 4 * 4 * 8, dtype=torch.bfloat16, device="cuda")
    y = torch.zeros(2 * 8 * 8 * 8, dtype=torch.bfloat16, device="cuda")
    ptrs = [x.data_ptr(), y.data_ptr()]
    for ints in ([2, 4, 4, 8, 8, 8, 1, 1, 1],      # both flags
                 [2, 4, 4, 8, 8, 8, 2, 0, 0],      # unknown mode
                 [2, 4, 4, 8, 0, 8, 0, 0, 0]):     # empty output
        with pytest.raises(RuntimeError):
            ext.ExecPlan([(ext.K_RESIZE, ptrs, ints, [])]).run()


# -- zero-insert, kernel level -----------------------------------------------

@pytest.mark.parametrize("C", [8, 24, 6])
def test_zero_insert_kernel(C):
    torch, ext = _torch_ext()
    g = torch.Generator().manual_seed(C)
    sent = torch.tensor(SENTINEL, dtype=torch.bfloat16)
    for (h, w), (sh, sw) in [((5, 7), (2, 2)), ((4, 3), (3, 2)),
                             ((1, 1), (2, 2)), ((19, 23), (2, 2))]:
        x = torch.randn(3, h, w, C, generator=g).to(torch.bfloat16)
        Ho, Wo = (h - 1) * sh + 1, (w - 1) * sw + 1
        n_out = 3 * Ho * Wo * C
        buf = torch.full((n_out + TAIL,), SENTINEL, dtype=torch.bfloat16,
                         device="cuda")
        xc = x.cuda().contiguous()
        ext.ExecPlan([(ext.K_ZERO_INSERT, [xc.data_ptr(), buf.data_ptr()],
                       [3, h, w, C, sh, sw], [])]).run()
        torch.cuda.synchronize()
        want = torch.zeros(3, Ho, Wo, C, dtype=torch.bfloat16)
        want[:, ::sh, ::sw] = x
        assert torch.equal(buf[:n_out].view(3, Ho, Wo, C).cpu(), want)
        assert (buf[n_out:].cpu() == sent).all()


# -- transposed conv: GPU engine vs CPU executor -----------------------------

# (h, R, stride, padding, H): general lowering with SAME on even and odd
# H, the gemm+transpose lowering, and a 4x4 filter
_DECONV_CASES = [(5, 3, 2, "SAME", 10), (5, 3, 2, "SAME", 9),
                 (4, 2, 2, "VALID", 8), (3, 4, 2, "SAME", 6)]


def _deconv_relu_graph(h, R, stride, padding, H, w):
    Cout, Cin = w.shape[2], w.shape[3]
    gb = GraphBuilder()
    f32 = gb.a_type(1)
    x = gb.placeholder("input", np.float32, [-1, h, h, Cin],
                       signature_name="input")
    sz = gb.const("sizes", np.array([-1, H, H, Cout], np.int32))
    y = gb.node("Conv2DBackpropInput", "deconv", [sz, gb.const("w", w), x],
                T=f32, strides=gb.a_ints([1, stride, stride, 1]),
                padding=gb.a_str(padding), data_format=gb.a_str("NHWC"))
    y = gb.node("Relu", "relu", [y], T=f32)
    gb.mark_output("y", y)
    return gb.build()


@pytest.mark.parametrize("cin", [8, 6])     # 6: scalar zero-insert and
                                            # channel-padded conv
@pytest.mark.parametrize("h,R,stride,padding,H", _DECONV_CASES)
def test_conv_transpose_gpu_vs_cpu(tmp_path, h, R, stride, padding, H, cin):
    rng = np.random.default_rng(h * 100 + R * 10 + cin)
    w = (rng.standard_normal((R, R, 16, cin)) * 0.3).astype(np.float32)
    sm = _deconv_relu_graph(h, R, stride, padding, H, w)
    gm = _gpu_model(tmp_path, sm, name="dc")
    try:
        cm = _cpu_model(tmp_path, sm, name="dccpu")
        kinds = [op.kind for op in gm.plan.ops]
        assert kinds == (["gemm", "transpose"] if R == stride
                         else ["zero_insert", "conv2d"])
        x = (rng.standard_normal((3, h, h, cin)) * 0.8).astype(np.float32)
        want = cm.predict({"input": x})["y"]
        got = gm.predict({"input": x})["y"]     # batch 3 -> bucket 4
        again = gm.predict({"input": x})["y"]   # replay over a used arena
    finally:
        gm._gpu.release()
    assert got.shape == want.shape == (3, H, H, 16)
    print(f"max|gpu-cpu|={float(np.abs(got - want).max()):.4g}")
    np.testing.assert_allclose(got, want, rtol=0.05, atol=0.03)
    np.testing.assert_array_equal(again, got)


# -- build_unet: GPU vs CPU --------------------------------------------------

@pytest.mark.parametrize("upsample", ["deconv", "nearest", "bilinear"])
def test_unet_gpu_vs_cpu(tmp_path, upsample):
    sm = build_unet(image_size=32, upsample=upsample)
    gm = _gpu_model(tmp_path, sm, name="unet")
    try:
        cm = _cpu_model(tmp_path, sm, name="unetcpu")
        x = (np.random.default_rng(4).standard_normal((4, 32, 32, 3))
             * 0.5).astype(np.float32)
        want = cm.predict({"input": x})["probs"]
        got = gm.predict({"input": x})["probs"]
        replay = gm.predict({"input": x})["probs"]      # graph replay
        ctxs = [c for lst in gm._gpu._contexts.values() for c in lst]
        assert any(c.captured and c.exec_plan.has_graph() for c in ctxs)
    finally:
        gm._gpu.release()
    assert got.shape == (4, 32, 32, 4)
    print(f"max|gpu-cpu|={float(np.abs(got - want).max()):.4g}")
    np.testing.assert_allclose(got, want, atol=0.04)
    np.testing.assert_allclose(replay, got, rtol=1e-6)


def test_unet_template_context_and_capture_only_prewarm(tmp_path):
    """A second model loaded from the same SavedModel shares the plan:
    its context is instantiated from the relocatable call template (the
    resize / zero-insert calls carry workspace pointers only) and
    prewarmed by graph capture alone, with no eager run before it."""
    sm = build_unet(image_size=32, upsample="deconv")
    gm = _gpu_model(tmp_path, sm, name="unet_t")
    gm2 = None
    try:
        x = (np.random.default_rng(8).standard_normal((4, 32, 32, 3))
             * 0.5).astype(np.float32)
        first = gm.predict({"input": x})["probs"]   # registers the template
        from tfservingcache_amd.engine.gpu import GpuModel
        gm2 = load_model_from_dir(str(tmp_path / "unet_t" / "1"),
                                  "unet_t2", 1)
        assert gm2.plan is gm.plan
        gm2._gpu = GpuModel(gm2.plan, device="cuda:0", max_batch=64,
                            model_name="unet_t2", model_version=1)
        gm2._gpu.prewarm(4, limit=1)
        ctxs = [c for lst in gm2._gpu._contexts.values() for c in lst]
        assert ctxs and all(getattr(c, "_from_template", False) and
                            c.captured and c.exec_plan.has_graph()
                            for c in ctxs)
        second = gm2.predict({"input": x})["probs"]
    finally:
        gm._gpu.release()
        if gm2 is not None and getattr(gm2, "_gpu", None) is not None:
            gm2._gpu.release()
    np.testing.assert_allclose(second, first, rtol=1e-6)
