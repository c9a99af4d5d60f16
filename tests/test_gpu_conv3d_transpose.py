"""The 3-D transposed conv kernel (K_CONV's 24-int form) and build_unet3d on
the GPU, against torch CPU float64 on the same bf16 values. Bound, derived:
one bf16 rounding (2^-9), doubled for accumulation order: 2^-8 * max|want|.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tfservingcache_amd.engine.emit import _pad64  # noqa: E402
from tfservingcache_amd.engine.model import (LoadedModel,  # noqa: E402
                                             load_model_from_dir)
from tfservingcache_amd.engine.planner import (  # noqa: E402
    conv3d_transpose_phases, conv3d_transpose_taps)
from tfservingcache_amd.engine.savedmodel import write_saved_model  # noqa: E402
from tfservingcache_amd.models import build_unet3d  # noqa: E402
from test_conv3d import geometry  # noqa: E402
from test_conv3d_transpose import reference  # noqa: E402
from test_gpu_conv3d import BF, _assert_close, _ext, _run  # noqa: E402


def _deconv(N, dhw, C, K, trs, stride, padding, out_dhw=None, act=0,
            with_res=False, seed=0, override=None):
    """The K_CONV call (bias padded to a 128-column tile) and reference."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, *dhw, C, generator=g).to(BF)
    w = (torch.randn(*trs, K, C, generator=g) * 0.2).to(BF)  # [T,R,S,Co,Ci]
    b = (torch.randn(K, generator=g) * 0.5).to(BF)
    if out_dhw is None:     # SAME: D*s; VALID: (D-1)*s + T
        out_dhw = tuple(n * s if padding == "SAME" else (n - 1) * s + k
                        for n, s, k in zip(dhw, stride, trs))
    geom = geometry(out_dhw, trs, stride, padding)
    assert tuple(o for o, _, _ in geom) == tuple(dhw)
    pf, pt, pl = (lo for _, lo, _ in geom)
    out_shape = (N, *out_dhw, K)
    res = torch.randn(*out_shape, generator=g).to(BF) if with_res else None
    want = reference(x.double(), w.double(), stride, out_dhw,
                     (pf, pt, pl)) + b.double()
    if with_res:
        want = want + res.double()
    if act:
        want = torch.relu(want)
    k_pad = _pad64(conv3d_transpose_taps(trs, stride, C) * C)
    wk = torch.zeros(K, k_pad, dtype=BF)
    for _phase, taps, first in conv3d_transpose_phases(trs, stride):
        for i, (t, r, s) in enumerate(taps):
            wk[:, (first + i) * C:(first + i + 1) * C] = w[t, r, s]
    bk = torch.zeros(_pad64(K) * 2, dtype=BF)
    bk[:K] = b
    dev = [x.cuda(), wk.cuda(), bk.cuda(), res.cuda() if with_res else None,
           torch.zeros(64, dtype=BF, device="cuda")]
    ints = [N, dhw[1], dhw[2], C, K, trs[1], trs[2], stride[1], stride[2],
            pt, pl, out_dhw[1], out_dhw[2], k_pad, act, 1, 1, 1, dhw[0],
            trs[0], stride[0], pf, out_dhw[0], 1]
    for i, v in (override or {}).items():
        ints[i] = v
    return (_ext().K_CONV, dev, ints, out_shape), want.contiguous()


# (N, x (D,H,W), C, Kc, (T,R,S), strides, padding[, input_sizes dhw, act,
# residual])
_CASES = {
    # 1 or 2 taps per axis; M_phase = 150: two M tiles, the last partial
    "uneven_phases": (2, (3, 5, 5), 64, 16, (3, 3, 3), (2, 2, 2), "SAME"),
    # phases with different Q
    "odd_output": (2, (3, 5, 5), 64, 16, (3, 3, 3), (2, 2, 2), "SAME",
                   (5, 9, 9)),
    # one tap per phase, K = 16 in a 64 tile over the next phase's weights,
    # the row's zero taps for the last; Kc tail in a 128-column tile
    "kernel_eq_stride": (2, (3, 4, 4), 16, 24, (2, 2, 2), (2, 2, 2), "VALID"),
    # chunks cross taps inside a K tile: the per-lane cursor
    "c24_crossing": (1, (3, 4, 4), 24, 16, (3, 3, 3), (2, 2, 2), "SAME"),
    # pd = 1 has no tap: those voxels are relu(bias)
    "empty_phase": (1, (3, 4, 4), 16, 16, (1, 2, 2), (2, 2, 2), "VALID",
                    None, 1),
    "asymmetric": (2, (3, 6, 4), 16, 32, (2, 3, 4), (2, 1, 2), "SAME"),
    "spatial_only": (1, (4, 4, 4), 16, 16, (1, 4, 4), (1, 2, 2), "SAME"),
    "valid_overlap": (1, (3, 4, 4), 64, 16, (3, 3, 3), (2, 2, 2), "VALID"),
    # the residual is read at the scattered offset
    "relu_res": (3, (2, 4, 4), 64, 16, (3, 3, 3), (2, 2, 2), "SAME", None, 1,
                 True),
}


@pytest.mark.parametrize("name", list(_CASES))
def test_conv3d_transpose_kernel(name):
    call, want = _deconv(*_CASES[name], seed=len(name))
    _assert_close(name, _run(*call), want)


# ints 3 = C, 13 = k_pad (448 = pad64(27 * 16) lacks the row's zero taps:
# the last phase's tile spans k = 416..480, so the row is 512), 19 = T,
# 23 = the transposed flag
@pytest.mark.parametrize("override", [{3: 12}, {13: 448}, {23: 2}, {19: 0}])
def test_launcher_rejects(override):
    call, _ = _deconv(1, (3, 4, 4), 16, 16, (3, 3, 3), (2, 2, 2), "SAME",
                      override=override)
    assert _run(*call, expect_error=True), "a rejected call wrote"


def test_unet3d_gpu_vs_cpu(tmp_path):
    from tfservingcache_amd.engine.gpu import GpuModel
    d = str(tmp_path / "unet3d" / "1")
    write_saved_model(build_unet3d(), d)
    gm = load_model_from_dir(d, "unet3d", 1)
    cm = LoadedModel("unet3d_cpu", 1, gm.plan)
    gm._gpu = GpuModel(gm.plan, device="cuda:0", max_batch=8,
                       model_name="unet3d", model_version=1)
    try:
        for batch in (2, 3):                    # 3 -> bucket 4
            x = (np.random.default_rng(batch).standard_normal(
                (batch, 8, 16, 16, 3)) * 0.3).astype(np.float32)
            want = cm.predict({"input": x})
            got = gm.predict({"input": x})
            again = gm.predict({"input": x})    # graph replay
            assert got["probs"].shape == (batch, 8, 16, 16, 4)
            np.testing.assert_allclose(got["probs"], want["probs"],
                                       rtol=0.25, atol=0.05)
            np.testing.assert_array_equal(again["probs"], got["probs"])
    finally:
        gm._gpu.release()
