"""The 3-D conv and pool kernels and build_video_resnet on the GPU, against
torch CPU float64 on the same bf16 values. Bound, derived: one bf16 rounding
(2^-9), doubled for accumulation order: 2^-8 * max|want|. Max pooling: exact.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tfservingcache_amd.engine.model import (LoadedModel,  # noqa: E402
                                             load_model_from_dir)
from tfservingcache_amd.engine.savedmodel import write_saved_model  # noqa: E402
from tfservingcache_amd.models import build_video_resnet  # noqa: E402
from tfservingcache_amd.engine.emit import _pad64  # noqa: E402
from test_conv3d import geometry, padded, pool_reference  # noqa: E402

SENTINEL = 1.0e30
TAIL = 64
BF = torch.bfloat16


def _ext():
    from tfservingcache_amd.engine import _tfsc_engine as ext
    return ext


def _run(kind, dev, ints, out_shape, expect_error=False):
    ext = _ext()
    n_out = int(np.prod(out_shape))
    buf = torch.full((n_out + TAIL,), SENTINEL, dtype=BF, device="cuda")
    ptrs = [t.data_ptr() if t is not None else 0 for t in dev + [buf]]
    sent = torch.tensor(SENTINEL, dtype=BF)
    if expect_error:
        with pytest.raises(RuntimeError):
            ext.ExecPlan([(kind, ptrs, ints, [])]).run()
        torch.cuda.synchronize()
        return (buf.cpu() == sent).all()
    ext.ExecPlan([(kind, ptrs, ints, [])]).run()
    torch.cuda.synchronize()
    out = buf[:n_out].view(*out_shape).cpu()
    assert not (out == sent).any(), "unwritten output"
    assert (buf[n_out:].cpu() == sent).all(), "wrote past the end"
    return out


def _assert_close(what, got, want):
    bound = 2.0 ** -8 * float(want.abs().max())
    err = float((got.double() - want).abs().max())
    print(f"{what}: max|err|={err:.4g} bound={bound:.4g}")
    assert err <= bound, (what, err, bound)


def _conv(N, dhw, C, K, trs, stride, padding, act=0, with_res=False,
          seed=0, override=None):
    """The K_CONV call (bias padded to a 128-column tile) and reference."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, *dhw, C, generator=g).to(BF)
    w = (torch.randn(K, C, *trs, generator=g) * 0.2).to(BF)
    b = (torch.randn(K, generator=g) * 0.5).to(BF)
    geom = geometry(dhw, trs, stride, padding)
    (Do, pf, _), (Ho, pt, _), (Wo, pl, _) = geom
    out_shape = (N, Do, Ho, Wo, K)
    res = torch.randn(*out_shape, generator=g).to(BF) if with_res else None
    want = torch.nn.functional.conv3d(padded(x, geom), w.double(), b.double(),
                                      stride=stride).permute(0, 2, 3, 4, 1)
    if with_res:
        want = want + res.double()
    if act:
        want = torch.relu(want)
    trsc = int(np.prod(trs)) * C
    wk = torch.zeros(K, _pad64(trsc), dtype=BF)
    wk[:, :trsc] = w.permute(0, 2, 3, 4, 1).reshape(K, trsc)
    bk = torch.zeros(_pad64(K) * 2, dtype=BF)
    bk[:K] = b
    dev = [x.cuda(), wk.cuda(), bk.cuda(), res.cuda() if with_res else None,
           torch.zeros(64, dtype=BF, device="cuda")]
    ints = [N, dhw[1], dhw[2], C, K, trs[1], trs[2], stride[1], stride[2],
            pt, pl, Ho, Wo, _pad64(trsc), act, 1, 1, 1, dhw[0], trs[0],
            stride[0], pf, Do]
    for i, v in (override or {}).items():
        ints[i] = v
    return (_ext().K_CONV, dev, ints, out_shape), want.contiguous()


# (N, (D,H,W), C, K, (T,R,S), strides, padding[, act, residual])
_CONV_CASES = {
    # K = 432 -> 448, M = 150, padding on all six faces
    "k_tail": (2, (3, 5, 5), 16, 24, (3, 3, 3), (1, 1, 1), "SAME"),
    "tap_uniform": (1, (4, 5, 5), 64, 16, (3, 3, 3), (1, 1, 1), "SAME"),
    # C = 24: chunks cross taps and planes inside a K tile
    "c24_crossing": (1, (3, 4, 4), 24, 16, (3, 3, 3), (1, 1, 1), "SAME"),
    "temporal_stride": (1, (7, 6, 6), 8, 16, (3, 3, 3), (2, 1, 1), "VALID"),
    "asymmetric_same": (2, (4, 7, 6), 16, 16, (3, 3, 3), (2, 2, 2), "SAME"),
    "spatial_1x3x3": (2, (4, 6, 6), 16, 32, (1, 3, 3), (1, 1, 1), "SAME"),
    "temporal_3x1x1": (2, (4, 6, 6), 16, 32, (3, 1, 1), (1, 1, 1), "SAME"),
    "deep_filter": (2, (1, 5, 5), 16, 16, (3, 3, 3), (1, 1, 1), "SAME"),
    # M = 294: three M tiles, the last partial; relu + residual
    "m294_relu_res": (3, (2, 7, 7), 64, 16, (3, 3, 3), (1, 1, 1), "SAME", 1,
                      True),
}


@pytest.mark.parametrize("name", list(_CONV_CASES))
def test_conv3d_kernel(name):
    call, want = _conv(*_CONV_CASES[name], seed=len(name))
    _assert_close(name, _run(*call), want)


# ((D,H,W), C, window, strides, padding), N = 2
_POOL_CASES = {
    # v8 kernel; the divisor differs at corners, edges and faces
    "c16_w3_s2_same": ((4, 7, 6), 16, (3, 3, 3), (2, 2, 2), "SAME"),
    "c5_scalar_valid": ((4, 7, 6), 5, (2, 2, 2), (2, 2, 2), "VALID"),
    "temporal_only": ((4, 7, 6), 16, (3, 1, 1), (1, 1, 1), "SAME"),
    "deep_window": ((2, 7, 6), 16, (3, 3, 3), (1, 1, 1), "SAME"),
}


@pytest.mark.parametrize("mode", ["max", "avg"])
@pytest.mark.parametrize("name", list(_POOL_CASES))
def test_pool3d_kernel(name, mode):
    dhw, C, win, stride, padding = _POOL_CASES[name]
    x = torch.randn(2, *dhw, C, generator=torch.Generator().manual_seed(
        len(name))).to(BF)
    geom = geometry(dhw, win, stride, padding)
    want = pool_reference(x, geom, mode == "max", win, stride)
    (Do, pf, _), (Ho, pt, _), (Wo, pl, _) = geom
    got = _run(_ext().K_POOL, [x.cuda()],
               [int(mode == "max"), 2, *dhw, C, Do, Ho, Wo, *win, *stride,
                pf, pt, pl], (2, Do, Ho, Wo, C))
    if mode == "max":
        assert torch.equal(got.double(), want)
    else:
        _assert_close(f"{name}/avg", got, want)


# ints 13 = k_pad (pad64(27 * 16) is 448), 15 = groups, 16 = dh, 19 = T
@pytest.mark.parametrize("C,override", [
    (16, {15: 2}), (16, {16: 2}), (12, {}), (16, {13: 512}), (16, {19: 0})])
def test_launcher_rejects(C, override):
    call, _ = _conv(1, (3, 5, 5), C, 16, (3, 3, 3), (1, 1, 1), "SAME",
                    override=override)
    assert _run(*call, expect_error=True), "a rejected call wrote"


def test_video_resnet_gpu_vs_cpu(tmp_path):
    from tfservingcache_amd.engine.gpu import GpuModel
    d = str(tmp_path / "vid" / "1")
    write_saved_model(build_video_resnet(), d)
    gm = load_model_from_dir(d, "vid", 1)
    cm = LoadedModel("vid_cpu", 1, gm.plan)
    gm._gpu = GpuModel(gm.plan, device="cuda:0", max_batch=8,
                       model_name="vid", model_version=1)
    try:
        for batch in (2, 3):                    # 3 -> bucket 4
            x = (np.random.default_rng(batch).standard_normal(
                (batch, 8, 32, 32, 3)) * 0.3).astype(np.float32)
            want = cm.predict({"input": x})
            got = gm.predict({"input": x})
            again = gm.predict({"input": x})    # graph replay
            assert got["probs"].shape == (batch, 10)
            np.testing.assert_allclose(got["probs"], want["probs"],
                                       rtol=0.25, atol=0.05)
            np.testing.assert_array_equal(again["probs"], got["probs"])
    finally:
        gm._gpu.release()
