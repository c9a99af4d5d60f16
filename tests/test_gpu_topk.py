"""The top-k kernels of ops/topk.hip, one call at a time, and TopKV2
through a retrieval model.

Harness as in test_gpu_memory_kernels.py: one ExecPlan call with the
ints [rows, cols, k, P] laid out by hand; outputs and scratch pre-filled
with a sentinel and followed by 64 guard elements. Reference: a float64
numpy stable argsort of the bf16-rounded input. Exact: indices equal,
values bit-equal to x[row, idx]. SORT_BOUND is the widest row the sort
kernel takes, SORT_BOUND + 1 the narrowest the radix select does.
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
from tfservingcache_amd.models import build_retrieval  # noqa: E402

SENTINEL = 1.0e30
SENTINEL_INT = 0x7F7F7F7F
TAIL = 64
GRID_CAP = 2048                 # blocks per launch, both kernels
SORT_BOUND = 256                # ext.topk_sort_max_cols(), asserted below


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy()


def _reference(x, k):
    v = x.to(torch.float64).numpy()
    return np.argsort(-v, axis=-1, kind="stable")[:, :k].astype(np.int32)


def _check_topk(x, k, P, what):
    assert ext.topk_sort_max_cols() == SORT_BOUND
    rows, cols = x.shape
    n = rows * k
    idx = torch.full((n + TAIL,), SENTINEL_INT, dtype=torch.int32,
                     device="cuda")
    vals = torch.full((n + TAIL,), SENTINEL, dtype=torch.bfloat16,
                      device="cuda")
    n_scr = rows * P * k if P > 1 else 0
    scr = torch.full((n_scr + TAIL,), SENTINEL_INT, dtype=torch.int64,
                     device="cuda")
    xd = x.contiguous().cuda()
    ext.ExecPlan([(ext.K_ARGMAX_LAST,
                   [xd.data_ptr(), idx.data_ptr(), vals.data_ptr(),
                    scr.data_ptr() if P > 1 else 0],
                   [rows, cols, k, P], [])]).run()
    torch.cuda.synchronize()
    for name, buf, used in (("idx", idx, n), ("vals", vals, n),
                            ("scratch", scr, n_scr)):
        sent = torch.tensor(SENTINEL if buf is vals else SENTINEL_INT,
                            dtype=buf.dtype)
        assert (buf[used:].cpu() == sent).all(), \
            f"wrote past the end of {name}, {what}"
    got_idx = idx[:n].cpu().numpy().reshape(rows, k)
    want_idx = _reference(x, k)
    bad = np.argwhere(got_idx != want_idx)
    print(f"{what}: {len(bad)} of {n} indices differ")
    assert len(bad) == 0, (what, bad[:4].tolist(),
                           got_idx[tuple(bad[0])], want_idx[tuple(bad[0])])
    want_bits = np.take_along_axis(_bits(x), want_idx.astype(np.int64), -1)
    np.testing.assert_array_equal(
        _bits(vals[:n]).reshape(rows, k), want_bits, what)


def _random_rows(rows, cols, seed):
    # normal scores; rows 2, 4, ... few distinct values and both zeros
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g)
    few = torch.randint(-3, 4, (rows, cols), generator=g).float() * \
        (torch.randint(0, 2, (rows, cols), generator=g).float() * 2 - 1)
    x[2::2] = few[2::2] * 0.5
    return x.to(torch.bfloat16)


COLS = sorted({1, 7, 255, 256, 257, 1001, SORT_BOUND, SORT_BOUND + 1,
               70001})
# k = 1, 2, 10, cols and 1024 wherever the row has that many columns
UNSPLIT = [(c, k) for c in COLS
           for k in sorted({k for k in (1, 2, 10, c, 1024)
                            if k <= min(c, 1024)})]


@pytest.mark.parametrize("cols,k", UNSPLIT)
def test_topk_unsplit(cols, k):
    _check_topk(_random_rows(3, cols, 7 * cols + k), k, 1,
                f"topk [3,{cols}] k={k}")


@pytest.mark.parametrize("cols,k,P", [
    (70001, 10, 8), (70001, 1024, 3), (1001, 1001, 3), (1001, 2, 7),
    (9, 4, 4), (40000, 10, 2)])
def test_topk_split(cols, k, P):
    # cols % P != 0; segments shorter than k (1001, 1001, 3), an empty
    # one (9, 4, 4), ones too long for the LDS cache (40000, 10, 2)
    _check_topk(_random_rows(3, cols, cols + k + P), k, P,
                f"topk [3,{cols}] k={k} P={P}")


@pytest.mark.parametrize("cols,k,P", [
    (7, 2, 1), (SORT_BOUND + 1, 2, 1), (37, 2, 2)])
def test_topk_rows_past_the_grid_cap(cols, k, P):
    rows = GRID_CAP // P + 1
    for r in (1, rows):
        _check_topk(_random_rows(r, cols, r + cols), k, P,
                    f"topk [{r},{cols}] k={k} P={P}")


def _special_rows(cols, P):
    seglen = -(-cols // P) if P > 1 else cols // 2
    rows = {}
    rows["all_equal"] = torch.full((cols,), 1.5)
    r = torch.zeros(cols)
    r[1::3] = 2.0
    r[[5 % cols, cols // 2, cols - 1]] = 5.0
    rows["ties_straddle_threshold"] = r
    r = torch.full((cols,), -1.0)
    r[max(seglen - 3, 0):seglen + 3] = 2.5
    rows["ties_straddle_segment_boundary"] = r
    a, b = cols // 3, cols - 1
    r = torch.full((cols,), -1.0)
    r[a], r[b] = 0.0, -0.0
    rows["plus_zero_then_minus_zero"] = r
    r = torch.full((cols,), -1.0)
    r[a], r[b] = -0.0, 0.0
    rows["minus_zero_then_plus_zero"] = r
    rows["all_minus_inf"] = torch.full((cols,), float("-inf"))
    r = torch.zeros(cols)
    r[-1] = 3.0
    rows["max_at_last_index"] = r
    return torch.stack(list(rows.values())).to(torch.bfloat16), list(rows)


@pytest.mark.parametrize("cols,P", [
    (SORT_BOUND, 1), (SORT_BOUND + 1, 1), (1001, 1), (1001, 3), (70001, 1),
    (70001, 8)])
@pytest.mark.parametrize("k", [2, 10])
def test_topk_special_rows(cols, P, k):
    x, names = _special_rows(cols, P)
    _check_topk(x, k, P, f"topk special {names} cols={cols} k={k} P={P}")


def test_launcher_refuses_before_any_launch():
    x = torch.zeros(4, 16, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(4 * 16 * 2, dtype=torch.int64, device="cuda")
    ptrs = [x.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr()]
    for ints, scratch in (([4, 16, 0, 1], 1), ([4, 16, 17, 1], 1),
                          ([4, 2000, 1025, 1], 1), ([4, 16, 2, 0], 1),
                          ([4, 16, 2, 17], 1), ([4, 16, 2, 2], 0)):
        with pytest.raises(RuntimeError, match="topk"):
            ext.ExecPlan([(ext.K_ARGMAX_LAST,
                           ptrs[:3] + [ptrs[3] * scratch], ints, [])]).run()
    with pytest.raises(RuntimeError, match="argmax_last"):
        ext.ExecPlan([(ext.K_ARGMAX_LAST, ptrs[:3], [4, 16, 2], [])]).run()


GEMM_RTOL, GEMM_ATOL = 0.05, 0.02       # test_mlp_gpu_vs_cpu


@pytest.mark.parametrize("n_items,split", [(3001, False), (20011, True)])
def test_retrieval_model_predict_and_fast_path(tmp_path, n_items, split):
    # eager, hipGraph replay, C++ fast path; 20011 items split the rows
    from tfservingcache_amd.engine import emit
    from tfservingcache_amd.engine.gpu import GpuModel
    from tfservingcache_amd.wire import messages as m
    from tfservingcache_amd.wire.tensor import (numpy_to_tensorproto,
                                                tensorproto_to_numpy)
    k = 10
    assert all((emit.topk_segments(b, n_items, k) > 1) == split
               for b in (1, 8))
    sm = build_retrieval(n_items=n_items, k=k, seed=3)
    d = str(tmp_path / "retr" / "1")
    write_saved_model(sm, d)
    cm = load_model_from_dir(d, "retr", 1)
    gm = load_model_from_dir(d, "retr", 1)
    gm._gpu = GpuModel(gm.plan, device="cuda:0", max_batch=8,
                       model_name="retr", model_version=1)
    try:
        assert [op.kind for op in gm.plan.ops][-1] == "topk_last"
        q = np.random.default_rng(5).standard_normal((5, 32)).astype(
            np.float32)
        for batch in (1, 5):                        # 5 -> bucket 8
            feeds = {"query": q[:batch]}
            want = cm.predict(feeds)
            outs = {"predict": gm.predict(feeds),
                    "replay": gm.predict(feeds)}
            req = m.PredictRequest(
                model_spec=m.ModelSpec(name="retr",
                                       version=m.Int64Value(value=1)),
                inputs={"query": numpy_to_tensorproto(q[:batch])}).encode()
            resp = m.PredictResponse.decode(gm._gpu.fast_predict(req))
            outs["fast"] = {a: tensorproto_to_numpy(t)
                            for a, t in resp.outputs.items()}
            for path, got in outs.items():
                what = f"{path} batch {batch}"
                logits = got["logits"]
                assert logits.shape == (batch, n_items), what
                assert got["ids"].dtype == np.int32, what
                ids = np.argsort(-logits.astype(np.float64), axis=-1,
                                 kind="stable")[:, :k]
                np.testing.assert_array_equal(got["ids"], ids, what)
                np.testing.assert_array_equal(
                    got["scores"], np.take_along_axis(logits, ids, -1), what)
                np.testing.assert_allclose(logits, want["logits"],
                                           rtol=GEMM_RTOL, atol=GEMM_ATOL,
                                           err_msg=what)
    finally:
        gm._gpu.release()
