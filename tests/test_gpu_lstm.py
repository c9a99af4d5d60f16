"""The LSTM kernels (K_LSTM, both geometries) and build_lstm_tagger on the
GPU. Reference: test_lstm.reference in fp64 on the same bf16 values, with
the two roundings the design fixes (pre to bf16, h to bf16 each step); the
cell state is never rounded. Bound, derived: |h| < 1, so 2^-7 absolute is
two bf16 ulps of the top binade, one flipped rounding plus its echo; for cs
2^-7 * max(1, |cs|) plus cs's own bf16 store (2^-9 relative). The same
maths in f32 with reversed summation differs from fp64 by at most 2^-17 on
h, so only rounding flips from the device's fast exp consume the bound."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tfservingcache_amd.engine.emit import _pad64  # noqa: E402
from tfservingcache_amd.engine.model import (LoadedModel,  # noqa: E402
                                             load_model_from_dir)
from tfservingcache_amd.engine.planner import lstm_cols, lstm_pack  # noqa: E402
from tfservingcache_amd.engine.savedmodel import write_saved_model  # noqa: E402
from tfservingcache_amd.models import build_lstm_tagger  # noqa: E402
from test_gpu_conv3d import BF, SENTINEL, TAIL, _ext, _run  # noqa: E402
from test_lstm import reference  # noqa: E402


def _bf(a):
    """Round an array to bf16 values, as float64."""
    return torch.as_tensor(np.asarray(a, np.float64)).to(BF).double().numpy()


def _lstm(T, B, I, H, state=False, peephole=False, clip=0.0,
          batch_major=False, cs=False, seed=0):
    """Device pointers (all but the outputs), ints and the reference."""
    rng = np.random.default_rng(seed)
    x = _bf(rng.standard_normal((T, B, I)))
    w = _bf(0.5 * rng.standard_normal((I + H, 4 * H)) / np.sqrt(H))
    b = _bf(0.5 * rng.standard_normal(4 * H))
    peep = [_bf(rng.standard_normal(H)) for _ in range(3)] if peephole \
        else None
    h0, c0 = (_bf(0.5 * rng.standard_normal((B, H))) for _ in range(2)) \
        if state else (None, None)
    want = reference(x, w, b, "icfo", clip=clip, peep=peep, h0=h0, c0=c0,
                     rnd=_bf)
    N = lstm_cols(H)
    pre = lstm_pack(_bf(x @ w[:I] + b).reshape(T, B, 4, H), H)   # [T,B,N]
    wh = np.zeros((N, _pad64(H)))
    wh[:, :H] = lstm_pack(w[I:].reshape(H, 4, H), H).T
    if batch_major:
        pre = pre.transpose(1, 0, 2)
    dev = [torch.as_tensor(np.ascontiguousarray(v)).to(BF).cuda()
           if v is not None else None
           for v in [pre, wh, *(peep or [None] * 3), h0, c0]]
    dev.append(torch.full((B, H), 7.0, device="cuda"))  # stale cell state
    ints = [T, B, H, H, T * H, 1, T] if batch_major else \
        [T, B, H, B * H, H, B, 1]
    return dev, ints, clip, cs, want, batch_major


def _outputs(call, max_h):
    """Run the call with the resident limit at max_h; (h, cs) as [T,B,H]."""
    dev, ints, clip, want_cs, _, batch_major = call
    T, B, H = ints[:3]
    ext = _ext()
    bufs = [torch.full((T * B * H + TAIL,), SENTINEL, dtype=BF,
                       device="cuda") for _ in range(2)]
    ptrs = [t.data_ptr() if t is not None else 0 for t in dev] + \
        [bufs[0].data_ptr(), bufs[1].data_ptr() if want_cs else 0]
    ext.set_lstm_resident_max_h(max_h)
    try:
        ext.ExecPlan([(ext.K_LSTM, ptrs, ints, [clip])]).run()
        torch.cuda.synchronize()
    finally:
        ext.set_lstm_resident_max_h(-1)
    sent = torch.tensor(SENTINEL, dtype=BF)
    outs = []
    for buf in bufs[:2 if want_cs else 1]:
        out = buf.cpu()
        assert not (out[:T * B * H] == sent).any(), "unwritten output"
        assert (out[T * B * H:] == sent).all(), "wrote past the end"
        out = out[:T * B * H].double().numpy()
        outs.append(out.reshape(B, T, H).transpose(1, 0, 2)
                    if batch_major else out.reshape(T, B, H))
    if not want_cs:
        assert (bufs[1].cpu() == sent).all(), "wrote an unrequested cs"
    return outs


# (T, B, I, H[, kwargs])
_CASES = {
    "one_tile_step0": (1, 1, 8, 16),
    "state_handover": (3, 3, 8, 16, dict(state=True)),
    "two_batch_tiles": (4, 17, 8, 32),
    "h20_tails": (3, 2, 8, 20),
    "resident_limit": (3, 2, 8, 128),
    "stepped_only_k136": (3, 2, 8, 136),
    "peephole_clip": (3, 3, 8, 48, dict(peephole=True, clip=0.25)),
    "batch_major_cs": (3, 3, 8, 16, dict(batch_major=True, cs=True)),
}


@pytest.mark.parametrize("name", list(_CASES))
def test_lstm_kernel(name):
    case = _CASES[name]
    kwargs = case[4] if len(case) > 4 else {}
    call = _lstm(*case[:4], seed=len(name), **kwargs)
    want_h, want_cs = call[4]
    if kwargs.get("clip"):
        assert (np.abs(want_cs) == kwargs["clip"]).any(), "clip never binds"
    H = case[3]
    limit = _ext().lstm_resident_max_h()
    for geom, max_h in [("resident", limit)] * (H <= limit) + \
            [("stepped", 0)]:
        outs = _outputs(call, max_h)
        err = float(np.abs(outs[0] - want_h).max())
        print(f"{name}/{geom}: h max|err|={err:.4g} bound={2.0 ** -7:.4g}")
        assert err <= 2.0 ** -7, (name, geom, err)
        if kwargs.get("cs"):
            bound = 2.0 ** -7 * np.maximum(1.0, np.abs(want_cs)) + \
                2.0 ** -9 * np.abs(want_cs)
            err = np.abs(outs[1] - want_cs)
            print(f"{name}/{geom}: cs max|err|={float(err.max()):.4g}")
            assert (err <= bound).all(), (name, geom, float(err.max()))


# ints 0 = T, 2 = H, 3 = st_t (rows of H elements H apart on both axes);
# pointer 7 = the cell scratch
@pytest.mark.parametrize("ints,null", [({0: 0}, None), ({2: 0}, None),
                                       ({3: 16, 4: 16}, None), ({}, 7)],
                         ids=["T=0", "H=0", "overlap", "null-cstate"])
def test_launcher_rejects(ints, null):
    dev, base = _lstm(3, 3, 8, 16)[:2]
    for i, v in ints.items():
        base[i] = v
    if null is not None:
        dev[null] = None
    h = torch.full((3 * 3 * 16,), SENTINEL, dtype=BF, device="cuda")
    assert _run(_ext().K_LSTM, dev + [h], base, (3, 3, 16),
                expect_error=True), "a rejected call wrote cs"
    assert (h.cpu() == torch.tensor(SENTINEL, dtype=BF)).all(), \
        "a rejected call wrote h"


def test_lstm_tagger_gpu_vs_cpu(tmp_path):
    from tfservingcache_amd.engine.gpu import GpuModel
    d = str(tmp_path / "tagger" / "1")
    write_saved_model(build_lstm_tagger(), d)
    gm = load_model_from_dir(d, "tagger", 1)
    # layer 2's h also feeds final_h, so the Transpose behind it stays an op
    assert [op.kind for op in gm.plan.ops] == [
        "gather", "lstm", "lstm", "transpose", "gemm", "softmax",
        "strided_copy"]
    cm = LoadedModel("tagger_cpu", 1, gm.plan)
    _geometry_run(gm, cm, GpuModel, -1)         # H = 48: resident
    _geometry_run(gm, cm, GpuModel, 0)          # stepped: c in the scratch


def _geometry_run(gm, cm, GpuModel, max_h):
    _ext().set_lstm_resident_max_h(max_h)
    gm._gpu = GpuModel(gm.plan, device="cuda:0", max_batch=8,
                       model_name="tagger", model_version=1)
    try:
        for batch in (2, 3):                    # 3 -> bucket 4
            ids = np.random.default_rng(batch).integers(
                0, 101, (batch, 12)).astype(np.int32)
            want = cm.predict({"input_ids": ids})
            got = gm.predict({"input_ids": ids})
            again = gm.predict({"input_ids": ids})      # graph replay
            assert got["probs"].shape == (batch, 12, 7)
            for k in ("probs", "final_h"):
                np.testing.assert_allclose(got[k], want[k], rtol=0.25,
                                           atol=0.05)
                # the replay started from the same (zero) state
                np.testing.assert_array_equal(again[k], got[k])
    finally:
        gm._gpu.release()
        _ext().set_lstm_resident_max_h(-1)
