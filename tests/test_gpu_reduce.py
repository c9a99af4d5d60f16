"""The reduce kernels of ops/reduce.hip, one call at a time, and the
pooling encoder through them.

Harness as in test_gpu_topk.py: one ExecPlan call with the ints laid out
by hand (P too, so a split is forced at small sizes); output and scratch
pre-filled with a sentinel and followed by guard elements. Reference:
numpy float64 over the same bf16 values. Max and min are exact. Sum and
mean: |err| <= 2^-8 |ref| + red 2^-23 sum|x_j| (one bf16 rounding plus
f32 accumulation, doubled). Prod: relative 2^-8 + red 2^-23, inputs
+-U[0.9, 1.1] and red <= 300. NaN order in max / min is not tested.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

from tfservingcache_amd.engine import _tfsc_engine as ext  # noqa: E402
from tfservingcache_amd.engine.model import (  # noqa: E402
    load_model_from_dir)
from tfservingcache_amd.engine.savedmodel import (  # noqa: E402
    write_saved_model)
from tfservingcache_amd.models import build_pooling_encoder  # noqa: E402

FNS = ["mean", "sum", "max", "min", "prod"]           # the call's fn codes
NP_FN = dict(zip(FNS, (np.mean, np.sum, np.max, np.min, np.prod)))
WAVE_MAX = 2048         # ext.reduce_wave_max_cols(), asserted below
TX_MAX = 64             # ext.reduce_cols_tx_max(); TY = 256 / TX
WG_TARGET = 512         # tiles narrow to 8 lanes below this many workgroups
TAIL = 64


def _check(x, fn, P, what, offset=0, plant=None):
    """x: f32 [outer, red, inner] -> runs the call on its bf16 rounding."""
    assert (ext.reduce_wave_max_cols(), ext.reduce_cols_tx_max(),
            ext.reduce_cols_wg_target()) == (WAVE_MAX, TX_MAX, WG_TARGET)
    outer, red, inner = x.shape
    buf = torch.zeros(x.numel() + 8, dtype=torch.bfloat16)
    buf[offset:offset + x.numel()] = x.reshape(-1).to(torch.bfloat16)
    xd = buf.cuda()[offset:offset + x.numel()]
    n, n_scr = outer * inner, (outer * inner * P if P > 1 else 0)
    y = torch.full((n + TAIL,), 1.0e30, dtype=torch.bfloat16, device="cuda")
    scr = torch.full((n_scr + TAIL,), 1.0e30, dtype=torch.float32,
                     device="cuda")
    ptrs = [xd.data_ptr(), y.data_ptr(), scr.data_ptr() if P > 1 else 0]
    code = FNS.index(fn)
    call = (ext.K_MEAN_LAST, ptrs, [outer, red, code, P], []) if inner == 1 \
        else (ext.K_MEAN_MID, ptrs, [outer, red, inner, code, P], [])
    ext.ExecPlan([call]).run()
    torch.cuda.synchronize()
    for name, t, used in (("y", y, n), ("scratch", scr, n_scr)):
        assert (t[used:].cpu() == torch.tensor(1.0e30, dtype=t.dtype)).all(), \
            f"wrote past the end of {name}, {what}"
    got = y[:n].double().cpu().numpy().reshape(outer, inner)
    v = xd.double().cpu().numpy().reshape(outer, red, inner)
    ref = NP_FN[fn](v, axis=1)
    if fn in ("max", "min"):
        bound = np.zeros_like(ref)
    elif fn == "prod":
        assert red <= 300
        bound = (2.0 ** -8 + red * 2.0 ** -23) * np.abs(ref)
    else:
        acc = red * 2.0 ** -23 * np.abs(v).sum(axis=1)
        bound = 2.0 ** -8 * np.abs(ref) + (acc / red if fn == "mean" else acc)
    err = np.abs(got - ref)
    print(f"{what}: worst err/bound {np.max(err / np.maximum(bound, 1e-300))}"
          if bound.any() else f"{what}: {int((err != 0).sum())} differ")
    assert (err <= bound).all(), (what, np.argwhere(err > bound)[:4].tolist())
    if plant is not None:
        assert (got == plant).all(), what


def _data(fn, shape, seed):
    g = torch.Generator().manual_seed(seed)
    if fn == "prod":
        sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
        return (torch.rand(shape, generator=g) * 0.2 + 0.9) * sign
    return torch.randn(shape, generator=g)


SEG = 20002             # segment length of a 40003-column row at P = 2
# cols, P, offset: 8 is one vector, 64 * 8 one wave's sweep (past it a
# lane holds 2, past 128 * 8 it holds 4 loads), WAVE_MAX the
# wave-to-workgroup handover; 40003 at P = 2 has a ragged last segment
ROWS = [(c, 1, 0) for c in (1, 7, 8, 9, 64 * 8 - 1, 64 * 8 + 1, WAVE_MAX - 1,
                            WAVE_MAX, WAVE_MAX + 1, 9001)] + \
    [(513, 1, 1), (1500, 1, 1), (40003, 2, 0), (299, 2, 1)]


@pytest.mark.parametrize("fn", FNS)
@pytest.mark.parametrize("cols,P,offset", ROWS)
def test_reduce_rows(fn, cols, P, offset):
    if fn == "prod" and cols > 300:
        cols = 300 - cols % 7         # prod's bound holds to red = 300
    _check(_data(fn, (5, cols, 1), cols + P), fn, P,
           f"{fn} rows [5,{cols}] P={P} +{offset}", offset)


TY16 = 256 // 2         # TY of inner = 16: two lanes of 8 channels
# outer, red, inner, P, offset: one slice, a few, TY + 1, the scalar path,
# a ragged split whose segments run the 4-deep loop, a ragged last tile
# (8 lanes wide, then past the 4-deep loop, then TX_MAX wide once the
# launch has WG_TARGET workgroups), 16-byte loads refused by the pointer,
# a split on the scalar path
COLS = [(3, 1, 8, 1, 0), (3, 5, 8, 1, 0), (2, TY16 + 1, 16, 1, 0),
        (2, 37, 12, 1, 0), (1, 2500, 8, 3, 0), (2, 9, 8 * TX_MAX + 8, 1, 0),
        (2, 37, 8 * TX_MAX + 8, 1, 0),
        (WG_TARGET // 2, 9, 8 * TX_MAX + 8, 1, 0), (3, 5, 8, 1, 1),
        (2, 300, 12, 4, 0)]


@pytest.mark.parametrize("fn", FNS)
@pytest.mark.parametrize("outer,red,inner,P,offset", COLS)
def test_reduce_cols(fn, outer, red, inner, P, offset):
    if fn == "prod" and red > 300:
        red = 300
    _check(_data(fn, (outer, red, inner), red + inner), fn, P,
           f"{fn} cols [{outer},{red},{inner}] P={P} +{offset}", offset)


@pytest.mark.parametrize("fn,value", [("max", 100.0), ("min", -100.0)])
@pytest.mark.parametrize("shape,P,offset,pos", [
    ((5, 40003, 1), 2, 0, p) for p in (0, 40002, 40001, SEG - 1, SEG)] + [
    ((5, WAVE_MAX - 3, 1), 1, 1, p) for p in (0, WAVE_MAX - 4)] + [
    ((1, 2500, 8), 3, 0, p) for p in (0, 2499, 833, 834)])
def test_max_min_find_a_planted_extreme(fn, value, shape, P, offset, pos):
    # first and last index, the masked tail, both sides of a segment edge
    x = _data(fn, shape, pos)
    x[:, pos, :] = value
    _check(x, fn, P, f"{fn} planted at {pos} of {shape} P={P}", offset,
           plant=value)


GEMM_RTOL, GEMM_ATOL = 0.05, 0.02       # test_gpu_topk's retrieval fixture


def test_pooling_encoder_gpu_vs_cpu_and_graph_replay(tmp_path):
    from tfservingcache_amd.engine.gpu import GpuModel
    # seed 46: on the CPU every top-3 score of these inputs stands clear
    # of its neighbours by about twice the tolerance
    k, n_items = 3, 24
    d = str(tmp_path / "enc" / "1")
    write_saved_model(build_pooling_encoder(n_items=n_items, k=k, seed=46), d)
    cm = load_model_from_dir(d, "enc", 1)
    gm = load_model_from_dir(d, "enc", 1)
    gm._gpu = GpuModel(gm.plan, device="cuda:0", max_batch=4,
                       model_name="enc", model_version=1)
    rng = np.random.default_rng(6)
    ids = rng.integers(0, 101, (3, 12)).astype(np.int32)
    mask = (np.arange(12)[None, :] < np.array([[12], [5], [1]])).astype(
        np.int32)
    compared = skipped = 0
    try:
        for batch in (1, 3):                        # 3 -> bucket 4
            feeds = {"input_ids": ids[:batch], "input_mask": mask[:batch]}
            want, got, again = (cm.predict(feeds), gm.predict(feeds),
                                gm.predict(feeds))
            for name in ("embedding", "logits", "scores"):
                np.testing.assert_allclose(got[name], want[name],
                                           rtol=GEMM_RTOL, atol=GEMM_ATOL)
            for name in got:                        # hipGraph replay
                np.testing.assert_array_equal(got[name], again[name])
            # an index is pinned where the CPU score stands clear of both
            # neighbours in the descending order
            s = -np.sort(-want["logits"].astype(np.float64), -1)[:, :k + 1]
            tol = GEMM_ATOL + GEMM_RTOL * np.abs(s)
            gap = np.full_like(s, np.inf)
            gap[:, 1:] = s[:, :-1] - s[:, 1:]
            clear = (gap[:, :k] > tol[:, :k]) & (gap[:, 1:] > tol[:, :k])
            compared += int(clear.sum())
            skipped += int((~clear).sum())
            np.testing.assert_array_equal(got["ids"][clear],
                                          want["ids"][clear])
    finally:
        gm._gpu.release()
    assert skipped <= 0.1 * (compared + skipped), (compared, skipped)
