"""Dilated convs on the GPU: the dilated implicit-GEMM kernel and its
dead-tap skipping, the two dilated depthwise kernels, the launchers'
argument checks, the old call forms, and build_deeplab.

Kernel level goes through ExecPlan([(K_CONV | K_DEPTHWISE, ptrs, ints)])
on torch bf16 tensors; the output buffer is pre-filled with a sentinel and
has a 64-element tail. The reference is torch CPU float64
conv2d(dilation=, groups=) on the same bf16-rounded values. Tolerance,
derived: accumulation is f32 and the result is rounded to bf16 once (2^-9
relative). Asserted: |got - want| <= 2^-8 * max|want| - twice the rounding
bound, the slack is for accumulation order.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tfservingcache_amd.engine.model import (LoadedModel,  # noqa: E402
                                             load_model_from_dir)
from tfservingcache_amd.engine.savedmodel import write_saved_model  # noqa: E402
from tfservingcache_amd.models import build_deeplab  # noqa: E402

SENTINEL = 1.0e30
TAIL = 64
ACT = {"none": 0, "relu": 1, "relu6": 5}


def _torch_ext():
    import torch
    from tfservingcache_amd.engine import _tfsc_engine as ext
    return torch, ext


def _pad64(k):
    return (k + 63) // 64 * 64


def _axis(size, R, stride, d, padding, explicit):
    """(out size, pad before, pad after) of one axis, TF rules on the
    effective extent (R-1)*d + 1."""
    Re = (R - 1) * d + 1
    if padding == "SAME":
        out = -(-size // stride)
        tot = max((out - 1) * stride + Re - size, 0)
        return out, tot // 2, tot - tot // 2
    lo, hi = explicit if padding == "EXPLICIT" else (0, 0)
    return (size + lo + hi - Re) // stride + 1, lo, hi


def _case(N, H, W, C, K, R, S, stride, dil, padding, seed, depthwise=False):
    """bf16-rounded x [N,H,W,C], w (torch layout [K,C,R,S], depthwise
    [C,1,R,S]), bias, and the geometry. padding: "SAME", "VALID" or
    (pt, pb, pl, pr)."""
    torch, _ = _torch_ext()
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, C, generator=g).to(torch.bfloat16)
    w = (torch.randn(K, 1 if depthwise else C, R, S, generator=g) * 0.2
         ).to(torch.bfloat16)
    b = (torch.randn(K, generator=g) * 0.5).to(torch.bfloat16)
    ex = padding if isinstance(padding, tuple) else (0, 0, 0, 0)
    mode = "EXPLICIT" if isinstance(padding, tuple) else padding
    Ho, pt, pb = _axis(H, R, stride, dil[0], mode, ex[:2])
    Wo, pl, pr = _axis(W, S, stride, dil[1], mode, ex[2:])
    return dict(N=N, H=H, W=W, C=C, K=K, R=R, S=S, stride=stride, dil=dil,
                Ho=Ho, Wo=Wo, pads=(pt, pb, pl, pr), x=x, w=w, b=b,
                groups=C if depthwise else 1)


def _reference(c, act="none", res=None):
    torch, _ = _torch_ext()
    pt, pb, pl, pr = c["pads"]
    xt = torch.nn.functional.pad(c["x"].double().permute(0, 3, 1, 2),
                                 (pl, pr, pt, pb))
    y = torch.nn.functional.conv2d(xt, c["w"].double(), c["b"].double(),
                                   stride=c["stride"], dilation=c["dil"],
                                   groups=c["groups"]).permute(0, 2, 3, 1)
    if res is not None:
        y = y + res.double()
    if act == "relu":
        y = torch.relu(y)
    elif act == "relu6":
        y = torch.clamp(y, 0.0, 6.0)
    return y.contiguous()


def _conv_call(c, act="none", res=None, tail_ints=None):
    """K_CONV pointers and ints; w laid out [K][pad64(R*S*C)],
    k = (r*S+s)*C + c. The bias is padded to the 128-column tile the
    epilogue reads."""
    torch, ext = _torch_ext()
    K, rsc = c["K"], c["R"] * c["S"] * c["C"]
    w = torch.zeros(K, _pad64(rsc), dtype=torch.bfloat16)
    w[:, :rsc] = c["w"].permute(0, 2, 3, 1).reshape(K, rsc)
    b = torch.zeros(_pad64(K) * 2, dtype=torch.bfloat16)
    b[:K] = c["b"]
    dev = [c["x"].cuda().contiguous(), w.cuda(), b.cuda(),
           res.cuda().contiguous() if res is not None else None,
           torch.zeros(64, dtype=torch.bfloat16, device="cuda")]
    ints = [c["N"], c["H"], c["W"], c["C"], K, c["R"], c["S"], c["stride"],
            c["stride"], c["pads"][0], c["pads"][2], c["Ho"], c["Wo"],
            _pad64(rsc), ACT[act]]
    ints += [1, *c["dil"]] if tail_ints is None else tail_ints
    return ext.K_CONV, dev, ints


def _depthwise_call(c, act="none", res=None, tail_ints=None):
    """K_DEPTHWISE pointers and ints; w is [R,S,C] flat."""
    _, ext = _torch_ext()
    dev = [c["x"].cuda().contiguous(),
           c["w"][:, 0].permute(1, 2, 0).contiguous().cuda(), c["b"].cuda()]
    ints = [c["N"], c["H"], c["W"], c["C"], c["R"], c["S"], c["stride"],
            c["stride"], c["pads"][0], c["pads"][2], c["Ho"], c["Wo"],
            ACT[act]]
    ints += [1, *c["dil"]] if tail_ints is None else tail_ints
    return ext.K_DEPTHWISE, dev, ints


def _run(c, call):
    torch, ext = _torch_ext()
    kind, dev, ints = call
    n_out = c["N"] * c["Ho"] * c["Wo"] * c["K"]
    buf = torch.full((n_out + TAIL,), SENTINEL, dtype=torch.bfloat16,
                     device="cuda")
    ptrs = [t.data_ptr() if t is not None else 0 for t in dev] + \
        [buf.data_ptr()]
    ext.ExecPlan([(kind, ptrs, ints, [])]).run()
    torch.cuda.synchronize()
    sent = torch.tensor(SENTINEL, dtype=torch.bfloat16)
    out = buf[:n_out].view(c["N"], c["Ho"], c["Wo"], c["K"]).cpu()
    assert not (out == sent).any(), "unwritten output"
    assert (buf[n_out:].cpu() == sent).all(), "wrote past the end"
    return out


def _check(c, make_call, what, act="none", with_res=False):
    torch, _ = _torch_ext()
    res = None
    if with_res:
        g = torch.Generator().manual_seed(99)
        res = torch.randn(c["N"], c["Ho"], c["Wo"], c["K"],
                          generator=g).to(torch.bfloat16)
    got = _run(c, make_call(c, act, res))
    want = _reference(c, act, res)
    bound = 2.0 ** -8 * float(want.abs().max())
    err = float((got.double() - want).abs().max())
    print(f"{what}: max|err|={err:.4g} bound={bound:.4g}")
    assert err <= bound, (what, err, bound)
    return got


# (N, H, W, C, K, R, S, stride, (dh, dw), padding[, act, residual])
_DENSE_CASES = {
    # K tail 144 -> 192, partial M tile, partial N tile
    "d2_same": (2, 7, 7, 16, 24, 3, 3, 1, (2, 2), "SAME"),
    # rectangular image, per-axis dilation, asymmetric pads
    "per_axis_explicit": (2, 6, 9, 16, 16, 3, 3, 1, (3, 1), (3, 1, 0, 2)),
    # stride together with dilation
    "s2_d2_valid": (2, 11, 11, 8, 16, 3, 3, 2, (2, 2), "VALID"),
    # 8 of 9 taps skipped in every block
    "all_but_centre_dead": (2, 5, 5, 64, 16, 3, 3, 1, (6, 6), "SAME"),
    # M = 160: the bottom tap row is live in M tile 0 and dead in tile 1
    "dead_differs_by_tile": (1, 20, 8, 64, 16, 3, 3, 1, (12, 1), "SAME"),
    # C % 64 != 0: dead taps exist but K tiles straddle them
    "dead_but_straddling": (2, 5, 5, 16, 16, 3, 3, 1, (6, 6), "SAME"),
    # no live K tile: with W = 4, pl = 5 and dw = 9 the three taps of
    # output column wo read wi = wo-5, wo+4, wo+13, all outside [0, 4) for
    # wo = 0..3 (pr = 13 makes Wo = 4); the output is bias everywhere
    "no_live_tap": (1, 4, 4, 64, 16, 1, 3, 1, (1, 9), (0, 0, 5, 13)),
    # several M tiles, the last one partial; relu + residual
    "m300_relu_res": (3, 10, 10, 64, 16, 3, 3, 1, (2, 2), "SAME", "relu",
                      True),
}


@pytest.mark.parametrize("skip", [2, 0])
@pytest.mark.parametrize("name", list(_DENSE_CASES))
def test_dilated_conv_kernel(name, skip):
    """skip = 2 forces dead-tap skipping wherever C % 64 == 0 (the
    default mode leaves it out on grids this small), 0 compiles it out."""
    torch, ext = _torch_ext()
    spec = _DENSE_CASES[name]
    c = _case(*spec[:10], seed=len(name))
    ext.set_conv_dilated_skip(skip)
    try:
        got = _check(c, _conv_call, f"{name}/skip{skip}", *spec[10:])
    finally:
        ext.set_conv_dilated_skip(1)
    if name == "no_live_tap":
        assert torch.equal(got, c["b"].expand_as(got))


# (N, H, W, C, R, stride, (dh, dw), padding, act)
_DEPTHWISE_CASES = {
    "v8_d2": (2, 7, 7, 8, 3, 1, (2, 2), "SAME", "none"),
    # stride, per-axis dilation, fused activation
    "v8_s2_per_axis": (2, 9, 6, 24, 3, 2, (1, 3), "SAME", "relu6"),
    "scalar_c5": (2, 6, 6, 5, 3, 1, (2, 2), "VALID", "none"),
    # C % 8 != 0; only the centre tap is in the image
    "scalar_c12_d_gt_image": (1, 4, 4, 12, 3, 1, (5, 5), "SAME", "relu"),
}


@pytest.mark.parametrize("name", list(_DEPTHWISE_CASES))
def test_dilated_depthwise_kernel(name):
    N, H, W, C, R, stride, dil, padding, act = _DEPTHWISE_CASES[name]
    c = _case(N, H, W, C, C, R, R, stride, dil, padding, seed=len(name),
              depthwise=True)
    _check(c, _depthwise_call, name, act)


@pytest.mark.parametrize("make_call,depthwise", [(_conv_call, False),
                                                 (_depthwise_call, True)])
def test_trailing_ones_equal_the_short_form(make_call, depthwise):
    """[..., act, groups | M = 1, dh = 1, dw = 1] takes the same path as
    the 15-int CONV / 13-int DEPTHWISE: bit-identical output."""
    torch, _ = _torch_ext()
    c = _case(2, 7, 7, 16, 16 if depthwise else 24, 3, 3, 2, (1, 1), "SAME",
              seed=8, depthwise=depthwise)
    short = _run(c, make_call(c, "relu", tail_ints=[]))
    long_ = _run(c, make_call(c, "relu", tail_ints=[1, 1, 1]))
    assert torch.equal(short.view(torch.int16), long_.view(torch.int16))
    want = _reference(c, "relu")
    assert float((short.double() - want).abs().max()) <= \
        2.0 ** -8 * float(want.abs().max())


@pytest.mark.parametrize("make_call,C,K,tail", [
    (_conv_call, 16, 16, [1, 0, 2]),            # dh = 0
    (_conv_call, 16, 16, [2, 2, 2]),            # dilation with groups = 2
    (_conv_call, 12, 16, [1, 2, 2]),            # dilated CONV with C = 12
    (_depthwise_call, 16, 16, [2, 2, 2]),       # dilated DEPTHWISE, M = 2
    (_depthwise_call, 16, 16, [1, 2, 0]),       # dw = 0
])
def test_launchers_reject(make_call, C, K, tail):
    """RuntimeError before any launch: the sentinel output is untouched."""
    torch, ext = _torch_ext()
    c = _case(1, 5, 5, C, K, 3, 3, 1, (1, 1), "SAME", seed=3,
              depthwise=make_call is _depthwise_call)
    kind, dev, ints = make_call(c, tail_ints=tail)
    # sized for the M = 2 reading of the same ints
    y = torch.full((2 * 25 * K + TAIL,), SENTINEL, dtype=torch.bfloat16,
                   device="cuda")
    ptrs = [t.data_ptr() if t is not None else 0 for t in dev] + \
        [y.data_ptr()]
    with pytest.raises(RuntimeError):
        ext.ExecPlan([(kind, ptrs, ints, [])]).run()
    torch.cuda.synchronize()
    assert (y.cpu() == torch.tensor(SENTINEL, dtype=torch.bfloat16)).all()


def test_deeplab_gpu_vs_cpu(tmp_path):
    from tfservingcache_amd.engine.gpu import GpuModel
    d = str(tmp_path / "dl" / "1")
    write_saved_model(build_deeplab(image_size=33), d)
    gm = load_model_from_dir(d, "dl", 1)
    cm = LoadedModel("dl_cpu", 1, gm.plan)
    gm._gpu = GpuModel(gm.plan, device="cuda:0", max_batch=8,
                       model_name="dl", model_version=1)
    try:
        assert sum("dilation" in op.params for op in gm.plan.ops) == 5
        for batch in (2, 3):                    # 3 -> bucket 4
            x = (np.random.default_rng(batch).standard_normal(
                (batch, 33, 33, 3)) * 0.3).astype(np.float32)
            want = cm.predict({"input": x})
            got = gm.predict({"input": x})
            again = gm.predict({"input": x})    # graph replay
            assert got["probs"].shape == (batch, 33, 33, 5)
            assert np.all(np.isfinite(got["logits"]))
            print(f"b{batch}: max|gpu-cpu| probs="
                  f"{float(np.abs(got['probs'] - want['probs']).max()):.4g}")
            np.testing.assert_allclose(got["probs"], want["probs"],
                                       rtol=0.25, atol=0.05)
            np.testing.assert_allclose(again["probs"], got["probs"],
                                       rtol=1e-6)
    finally:
        gm._gpu.release()
