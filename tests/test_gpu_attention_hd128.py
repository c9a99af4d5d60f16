"""head_dim 128 geometry of the fused flash-attention kernel (GPU).

Kernel-level cases drive ExecPlan([(K_ATTENTION, ...)]) on torch bf16
tensors against an fp32 reference computed from the same bf16 values,
at B=2, H=3, D=128 (row stride 384: a wrong head offset cannot alias).

Inputs: scale = 128**-0.5, Q = 2*randn, K = randn, V = randn: a score
std of about 2, so the softmax is peaked and a contraction over the
wrong part of D moves the output by O(1). test_reference_has_teeth
asserts that on the CPU for every S used: the reference computed from
d < 64 of Q and K only differs from the full one by more than 10*atol.

Tolerance, derived as in test_gpu_attention_mask.py: the kernel rounds
P to bf16 once (relative 2^-9), rounds the output to bf16 (2^-9) and
normalises by an unrounded l, so |err| <= 3 * 2^-9 * max|V|. Asserted:
atol = 2^-7 * max|V|, rtol = 0. V rows at masked keys are multiplied by
16 AFTER max|V| is taken.

Sequence lengths, each the smallest that reaches its path (kv tiles of
64 processed in pairs; one ring of 2 tile slots for every S, restaged
between pairs, so the variant boundary of the D=64 kernel at S=128 is
here the first restage):
  40  one partial tile, S % 16 != 0
  128 two full tiles, one pair, no restage
  129 just above that boundary: the first restage, for one valid key
      (unmasked case only)
  200 two pairs (one restage), tail in the second pair
  300 three pairs (the slots are restaged twice), the last pair's
      second tile lies wholly past S
"""
import numpy as np
import pytest

from tfservingcache_amd.engine.model import (LoadedModel,
                                             load_model_from_dir)
from tfservingcache_amd.engine.planner import _Lowerer
from tfservingcache_amd.engine.savedmodel import (read_saved_model,
                                                  write_saved_model)
from tfservingcache_amd.models import build_bert

B, H, D = 2, 3, 128
SCALE = 128 ** -0.5
NEG = -10000.0
SEQS = [40, 128, 129, 200, 300]


def _torch():
    import torch
    return torch


def _ext():
    from tfservingcache_amd.engine import _tfsc_engine as ext
    return ext


def _qkv_cpu(S, seed, masked_keys=None, d=D, h=H):
    """Q = 2*randn, K = randn, V = randn, rounded to bf16 (CPU tensors);
    V rows at masked keys (bool [B, S]) scaled by 16. Returns q, k, v
    and max|V| of the unscaled V."""
    torch = _torch()
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, S, h, d, generator=g) * 2.0
    k = torch.randn(B, S, h, d, generator=g)
    v = torch.randn(B, S, h, d, generator=g)
    vmax = float(v.to(torch.bfloat16).float().abs().max())
    if masked_keys is not None:
        v = v * torch.where(masked_keys, 16.0, 1.0)[:, :, None, None]
    return [t.to(torch.bfloat16).contiguous() for t in (q, k, v)] + [vmax]


def _qkv(S, seed, masked_keys=None):
    q, k, v, vmax = _qkv_cpu(S, seed, masked_keys)
    return q.cuda(), k.cuda(), v.cuda(), vmax


def _run(q, k, v, bias=None, strides=(0, 0, 0)):
    torch, ext = _torch(), _ext()
    _, S, h, d = q.shape
    out = torch.zeros_like(q)
    ptrs = [q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()]
    ints = [B, S, h, d]
    if bias is not None:
        assert bias.dtype == torch.bfloat16 and bias.is_contiguous()
        ptrs.append(bias.data_ptr())
        ints += list(strides)
    ext.ExecPlan([(ext.K_ATTENTION, ptrs, ints, [SCALE])]).run()
    torch.cuda.synchronize()
    return out.float().cpu()


def _reference(q, k, v, bias4=None, keep=None, d_used=D):
    """fp32 softmax(scale*QK^T + bias) @ V from the bf16 values. `keep`
    (bool, broadcastable to [B,H,S,S]) drops keys instead of biasing
    them; d_used < D contracts QK^T over the first d_used columns only
    (the teeth check)."""
    torch = _torch()
    qf, kf, vf = (t.float().cpu() for t in (q, k, v))
    sc = torch.einsum("bqhd,bkhd->bhqk", qf[..., :d_used],
                      kf[..., :d_used]) * SCALE
    if bias4 is not None:
        sc = sc + bias4.float().cpu()
    if keep is not None:
        sc = sc.masked_fill(~keep, float("-inf"))
    return torch.einsum("bhqk,bkhd->bqhd", torch.softmax(sc, -1), vf)


def _check(got, want, vmax):
    torch = _torch()
    atol = 2.0 ** -7 * vmax
    assert torch.isfinite(got).all()
    err = float((got - want).abs().max())
    print(f"max|err|={err:.4g} atol={atol:.4g}")
    assert err <= atol, (err, atol)


def _valid_keys(S, spans):
    """bool [B, S]: valid key ranges per batch row."""
    torch = _torch()
    m = torch.zeros(B, S, dtype=torch.bool)
    for b, (lo, hi) in enumerate(spans):
        m[b, lo:hi] = True
    return m


@pytest.mark.parametrize("S", SEQS)
def test_reference_has_teeth(S):
    """CPU only: with these inputs a kernel that contracted QK^T over
    d < 64 alone would miss the tolerance by more than 10x."""
    q, k, v, vmax = _qkv_cpu(S, seed=S)
    atol = 2.0 ** -7 * vmax
    full = _reference(q, k, v)
    half = _reference(q, k, v, d_used=64)
    diff = float((full - half).abs().max())
    uniform = float((full - v.float().mean(1, keepdim=True)).abs().max())
    print(f"S={S} |full-half|={diff:.3g} |full-uniform|={uniform:.3g} "
          f"atol={atol:.3g}")
    assert diff > 10 * atol, (diff, atol)
    assert uniform > 10 * atol, (uniform, atol)


@pytest.mark.gpu
@pytest.mark.parametrize("S", SEQS)
def test_unmasked(S):
    q, k, v, vmax = _qkv(S, seed=S)
    _check(_run(q, k, v), _reference(q, k, v), vmax)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [40, 200])
def test_zero_bias_is_bit_identical(S):
    torch = _torch()
    q, k, v, vmax = _qkv(S, seed=S)
    base = _run(q, k, v)
    zb = torch.zeros(B, S, dtype=torch.bfloat16, device="cuda")
    assert torch.equal(_run(q, k, v, zb, (S, 0, 0)), base)
    zfull = torch.zeros(B, H, S, S, dtype=torch.bfloat16, device="cuda")
    assert torch.equal(
        _run(q, k, v, zfull, (H * S * S, S * S, S)), base)
    _check(base, _reference(q, k, v), vmax)


# (S, valid key span of batch row 0, of batch row 1): the _PAD_CASES of
# test_gpu_attention_mask.py
_PAD_CASES = [
    (40, (0, 23), (5, 40)),        # one partial tile, S % 16 != 0
    (128, (0, 70), (64, 128)),     # two full tiles; tile 0 masked
    (200, (150, 200), (0, 10)),    # first 128-col pair all masked /
                                   # right-padded, tail in pair 2
]


@pytest.mark.gpu
@pytest.mark.parametrize("S,span0,span1", _PAD_CASES)
@pytest.mark.parametrize("fill", [NEG, float("-inf")], ids=["m10000", "ninf"])
def test_key_padding_bias(S, span0, span1, fill):
    torch = _torch()
    valid = _valid_keys(S, [span0, span1])
    q, k, v, vmax = _qkv(S, seed=S + 1, masked_keys=~valid)
    bias = torch.where(valid, 0.0, fill).to(torch.bfloat16).cuda()
    got = _run(q, k, v, bias.contiguous(), (S, 0, 0))
    want = _reference(q, k, v, keep=valid[:, None, None, :])
    _check(got, want, vmax)


@pytest.mark.gpu
def test_all_keys_neg_inf_gives_zeros():
    torch = _torch()
    S = 200
    q, k, v, vmax = _qkv(S, seed=9)
    valid = _valid_keys(S, [(0, 0), (30, 180)])     # row 0: nothing valid
    bias = torch.where(valid, 0.0, float("-inf")).to(torch.bfloat16).cuda()
    got = _run(q, k, v, bias.contiguous(), (S, 0, 0))
    assert torch.isfinite(got).all()
    assert torch.equal(got[0], torch.zeros_like(got[0]))
    want = _reference(q, k, v, keep=valid[:, None, None, :])
    _check(got[1:], want[1:], vmax)


@pytest.mark.gpu
def test_causal_bias_exact_size_buffer():
    """[1,1,S,S] causal (sb=0, sh=0, sq=S) at S=200: the last q block and
    kv pair run past S; the bias tensor is exactly S*S elements."""
    torch = _torch()
    S = 200
    q, k, v, vmax = _qkv(S, seed=11)
    keep = torch.tril(torch.ones(S, S, dtype=torch.bool))
    bias = torch.where(keep, 0.0, NEG).to(torch.bfloat16).cuda().contiguous()
    assert bias.numel() == S * S
    got = _run(q, k, v, bias, (0, 0, S))
    _check(got, _reference(q, k, v, keep=keep[None, None]), vmax)


@pytest.mark.gpu
def test_full_random_bias():
    torch = _torch()
    S = 200
    q, k, v, vmax = _qkv(S, seed=12)
    g = torch.Generator().manual_seed(5)
    bias = ((torch.rand(B, H, S, S, generator=g) * 4 - 2)
            .to(torch.bfloat16).cuda().contiguous())
    got = _run(q, k, v, bias, (H * S * S, S * S, S))
    _check(got, _reference(q, k, v, bias4=bias), vmax)
    # [B,1,S,S]: head-broadcast view of the same data
    b1 = bias[:, :1].contiguous()
    got = _run(q, k, v, b1, (S * S, 0, S))
    _check(got, _reference(q, k, v, bias4=b1), vmax)


@pytest.mark.gpu
def test_head_dim_96_raises_before_any_launch():
    """An argument check in the launcher, not a fault: the output buffer
    is untouched and the device is fine afterwards."""
    torch, ext = _torch(), _ext()
    S = 40
    q, k, v, _ = _qkv_cpu(S, seed=3, d=96)
    q, k, v = q.cuda(), k.cuda(), v.cuda()
    out = torch.full_like(q, 7.0)
    plan = ext.ExecPlan([(ext.K_ATTENTION,
                          [q.data_ptr(), k.data_ptr(), v.data_ptr(),
                           out.data_ptr()], [B, S, H, 96], [SCALE])])
    with pytest.raises(Exception, match="64 or 128"):
        plan.run()
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(q, 7.0))


# -- end to end: masked BERT with 128-wide heads through the engine ----------
_BERT = dict(with_mask=True, seq_len=128, hidden=256, layers=2, heads=2,
             intermediate=256, vocab=500, seed=31)


def _gpu_model(d, name):
    from tfservingcache_amd.engine.gpu import GpuModel
    lm = load_model_from_dir(str(d), name, 1)
    lm._gpu = GpuModel(lm.plan, device="cuda:0", max_batch=64,
                       model_name=name, model_version=1)
    return lm


@pytest.fixture(scope="module")
def bert(tmp_path_factory):
    """One masked BERT: SavedModel dir, GPU model (fused), and the feeds
    / CPU results shared by the tests below (never mutated)."""
    root = tmp_path_factory.mktemp("mbert128")
    d = root / "mb128" / "1"
    write_saved_model(build_bert(**_BERT), str(d))
    rng = np.random.default_rng(6)
    ids = rng.integers(0, 500, (3, 128)).astype(np.int32)

    def mask(*lens):
        m = np.zeros((len(lens), 128), np.int32)
        for i, n in enumerate(lens):
            m[i, :n] = 1
        return m

    feeds = {
        "A": {"input_ids": ids[:2], "input_mask": mask(128, 37)},
        "B": {"input_ids": ids[:2], "input_mask": mask(64, 128)},
        "C3": {"input_ids": ids, "input_mask": mask(100, 5, 128)},
    }
    cpu = load_model_from_dir(str(d), "mb128_cpu", 1)
    want = {k: cpu.predict(f) for k, f in feeds.items()}
    gm = _gpu_model(d, "mb128")
    yield {"dir": d, "gm": gm, "feeds": feeds, "want": want}
    gm._gpu.release()


def _compare_bert(got, want):
    """Tolerances of test_bert_fused_attention_gpu_vs_cpu."""
    np.testing.assert_allclose(got["pooled_output"], want["pooled_output"],
                               rtol=0.1, atol=0.08)
    np.testing.assert_allclose(got["sequence_output"],
                               want["sequence_output"], rtol=0.2, atol=0.15)


@pytest.mark.gpu
def test_masked_bert_hd128_fused_vs_cpu_and_unfused(bert):
    gm = bert["gm"]
    att = [op for op in gm.plan.ops if op.kind == "attention"]
    assert len(att) == 2 and all(len(op.inputs) == 4 for op in att)
    assert all(op.params["head_dim"] == 128 for op in att)
    f, want = bert["feeds"]["A"], bert["want"]["A"]
    got = gm.predict(f)
    _compare_bert(got, want)

    # the parent commit's behaviour for this graph: the unfused plan
    from tfservingcache_amd.engine.gpu import GpuModel
    gd, sigs = read_saved_model(str(bert["dir"]))
    um = LoadedModel("mb128_unfused", 1,
                     _Lowerer(gd, next(iter(sigs.values()))).run())
    assert not any(op.kind == "attention" for op in um.plan.ops)
    um._gpu = GpuModel(um.plan, device="cuda:0", max_batch=64,
                       model_name="mb128_unfused", model_version=1)
    try:
        unf = um.predict(f)
    finally:
        um._gpu.release()
    e_fused = float(np.abs(got["sequence_output"] -
                           want["sequence_output"]).max())
    e_unf = float(np.abs(unf["sequence_output"] -
                         want["sequence_output"]).max())
    print(f"max|fused-cpu|={e_fused:.5f} max|unfused-cpu|={e_unf:.5f}")
    assert e_fused <= 1.5 * e_unf + 1e-2, (e_fused, e_unf)


@pytest.mark.gpu
def test_hd128_replay_reads_the_mask_live(bert):
    gm = bert["gm"]
    fa, fb = bert["feeds"]["A"], bert["feeds"]["B"]
    a1 = gm.predict(fa)
    a2 = gm.predict(fa)                  # hipGraph replay
    b = gm.predict(fb)
    a3 = gm.predict(fa)
    ctxs = [c for lst in gm._gpu._contexts.values() for c in lst]
    assert any(c.captured and c.exec_plan.has_graph() for c in ctxs)
    _compare_bert(b, bert["want"]["B"])
    assert np.abs(b["sequence_output"] - a2["sequence_output"]).max() > 0.05
    np.testing.assert_array_equal(a3["sequence_output"],
                                  a2["sequence_output"])
    np.testing.assert_array_equal(a3["pooled_output"], a2["pooled_output"])
    _compare_bert(a1, bert["want"]["A"])


@pytest.mark.gpu
def test_hd128_batch_bucket_padding(bert):
    f, want = bert["feeds"]["C3"], bert["want"]["C3"]
    got = bert["gm"].predict(f)          # batch 3 pads to bucket 4
    assert got["sequence_output"].shape == (3, 128, 256)
    assert got["pooled_output"].shape == (3, 256)
    _compare_bert(got, want)
