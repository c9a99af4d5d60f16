"""The memory-bound kernels of ops_memory.hip, one call at a time, against
float64 references written from each operation's definition
(memory_kernel_oracle.py; test_memory_kernel_oracle.py checks those
references and the sharpness of the inputs on the CPU).

Harness: inputs from a seeded torch.Generator, rounded to bf16 before
either side sees them; the kernel runs through
ExecPlan([(K_..., ptrs, ints, floats)]).run() with the ints laid out by
hand as executor.cpp's launch_call reads them; the output buffer is
pre-filled with a sentinel (1e30, or 0x7F7F7F7F for the i32 outputs of
argmax and cast) and followed by 64 guard elements. Every test asserts
that no sentinel is left in the output and that the guard is untouched.

Shapes are the smallest that reach a branch: the 4-wide vector body
against the scalar tail (n = 1, 3, 4, 5, 1027), the softmax dispatch at
cols 128 | 129 and 512 | 513, C % 8 in pooling, the 16-byte transpose
gate, block_reduce with partly idle waves (cols 255, 256, 257), and one
case per grid-stride loop just past the cap of 2048 blocks of 256.

Tolerances, derived. A kernel computes in f32 and rounds to bf16 once:
2^-9 relative. The asserted base term is twice that, 2^-8, per element
on |want|; for softmax and layernorm on the row's max|want| (their
errors are absolute in the normalised row). An absolute floor of 2^-126,
bf16's smallest normal, is added where an output may flush to zero.
  - Copy kernels (transpose, strided copy, scatter, gather, pad_nhwc,
    pad_last), max-pool, argmax and both casts: exact. Copies are
    compared as int16 views.
  - unary relu / neg / square / sqrt / rsqrt / relu6 and every binary
    function: the base term alone. One f32 operation is 2^-24 relative
    and sqdiff is two of them, far inside the doubling.
  - tanh, erf, gelu, sigmoid, exp: an extra term for the f32 evaluation
    of the formula itself, e.g. 1 + erf(v/sqrt 2) cancels for v ~ -5.
    It is measured, not guessed: the error of a plain float32 numpy
    evaluation of the kernel's formula against the float64 reference
    over the test's own inputs, and 4x its maximum is allowed (the
    margin is for the device's math library differing from numpy's by a
    few f32 ulp). Absolute for tanh, erf and gelu, which end in a sum
    that can cancel; relative to |want| for exp and sigmoid, which are a
    bare exponential (x runs to +-20, so an absolute term taken at e^20
    would swallow e^-20). Measured maxima over n in {1,3,4,5,1027}:
    tanh 5.9e-8, erf 5.5e-8, gelu 3.8e-7 (absolute); sigmoid 1.4e-7,
    exp 1.4e-7 (relative).
  - bn_act: base + 2^-22 (|x*scale| + |shift|) for the f32 multiply-add
    (each of the two roundings is 2^-24 of its result, which is at most
    |x*scale| + |shift|; four times that is stated), and for tanh /
    sigmoid / gelu 4x the measured error of the float32 formula on the
    test's inputs, absolute (measured maxima 1.2e-7 / 6.0e-8 / 4.8e-7
    over the five shapes; their slopes are at most 1.13, which the factor
    4 in the multiply-add term covers).
  - means: base + cols * 2^-24 * mean|x| of the reduced row (one f32
    rounding per addition, each at most 2^-24 of a partial sum that
    stays below cols * mean|x|).
  - average pool: base + kh*kw * 2^-24 * max|x|, likewise; the divisor
    is the count of taps inside the image.

f32_to_bf16 and bf16_to_f32 have no call kind: they run inside
FastModel.predict on the model's staging buffers. They are reached
through GpuModel.fast_predict on a one-op Neg graph over [1, n], whose
response is -bf16(x); exact, compared as uint32 views (NaN as NaN).

Softmax of a row of -inf is NaN, as in TF; asserted beside the bounded
cases.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import memory_kernel_oracle as mk  # noqa: E402
from tfservingcache_amd.engine.model import (  # noqa: E402
    load_model_from_dir)
from tfservingcache_amd.engine.savedmodel import (  # noqa: E402
    GraphBuilder, write_saved_model)

SENTINEL = 1.0e30
SENTINEL_I32 = 0x7F7F7F7F
TAIL = 64
BF16, I32 = torch.bfloat16, torch.int32


def _ext():
    from tfservingcache_amd.engine import _tfsc_engine as ext
    return ext


def _dev(t):
    return t.contiguous().cuda()


def _out_buffer(n, dtype):
    return torch.full((n + TAIL,), SENTINEL if dtype is BF16 else
                      SENTINEL_I32, dtype=dtype, device="cuda")


def _sentinel(dtype):
    return torch.tensor(SENTINEL if dtype is BF16 else SENTINEL_I32,
                        dtype=dtype)


def _launch(kind, ins, n_out, ints, floats=(), dtype=BF16, what=""):
    """Run one call whose last pointer is the output; `ins` are device
    tensors or raw addresses. Returns the n_out outputs on the CPU."""
    ext = _ext()
    buf = _out_buffer(n_out, dtype)
    ptrs = [t if isinstance(t, int) else t.data_ptr() for t in ins]
    ext.ExecPlan([(getattr(ext, "K_" + kind), ptrs + [buf.data_ptr()],
                   [int(i) for i in ints], list(floats))]).run()
    torch.cuda.synchronize()
    out, tail = buf[:n_out].cpu(), buf[n_out:].cpu()
    sent = _sentinel(dtype)
    assert (tail == sent).all(), f"wrote past the end, {what}"
    assert not (out == sent).any(), f"unwritten output, {what}"
    return out


def _check(what, got, want, bound):
    """got: bf16 tensor; want, bound: float64 arrays of its shape."""
    got = mk.f64(got).reshape(want.shape)
    err = np.abs(got - want).reshape(-1)
    bound = np.broadcast_to(bound, want.shape).reshape(-1)
    m = int(np.argmax(err))
    ratio = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)
    w = int(np.argmax(ratio))                # the element nearest its bound
    print(f"{what}: max|err|={float(err[m]):.4g} bound={float(bound[m]):.4g}"
          f" worst |err|/bound={float(ratio[w]):.3g}")
    assert np.all(err <= bound), (what, float(err[w]), float(bound[w]))


def _check_bits(what, got, want):
    """got, want: bf16 tensors; bit-identical."""
    same = np.array_equal(mk.bits(got).reshape(-1), mk.bits(want).reshape(-1))
    print(f"{what}: bit-identical={same}")
    assert same, what


# -- copy kernels ------------------------------------------------------------

def _transpose(x, perm, what):
    out_shape = [x.shape[p] for p in perm]
    st = mk.strides(list(x.shape))
    ints = [len(perm)] + out_shape + [st[p] for p in perm] + [x.numel()]
    got = _launch("TRANSPOSE", [_dev(x)], x.numel(), ints, what=what)
    _check_bits(what, got, x.permute(*perm).contiguous())


@pytest.mark.parametrize("name,shape,perm", [
    ("v8_head_split", [2, 3, 4, 8], [0, 2, 1, 3]),
    ("last12_scalar", [2, 3, 4, 12], [0, 2, 1, 3]),
    ("last_dim_moves", [2, 3, 4, 8], [0, 3, 1, 2]),
    ("2d_5x7", [5, 7], [1, 0]),
    ("6d", [2, 3, 2, 4, 2, 3], [5, 3, 0, 4, 1, 2]),
    ("grid_stride", [174763, 3], [1, 0]),           # n = 2048*256 + 1
])
def test_transpose(name, shape, perm):
    if name == "grid_stride":
        assert int(np.prod(shape)) == mk.GRID + 1
    _transpose(mk.randn(mk.gen(len(name)), *shape), perm, name)


@pytest.mark.parametrize("name", list(mk.SLICE_CASES))
def test_strided_copy_kernel(name):
    """A slice as emit.py spells it: a TRANSPOSE call whose source pointer
    is advanced by the slice's offset and whose strides are the sliced
    tensor's. The first two cases sit 6 and 132 bytes off a 16-byte
    boundary; the last two are aligned and keep the 16-byte kernel."""
    shape, idx, off, out_shape, st, _v8 = mk.SLICE_CASES[name]
    x = mk.randn(mk.gen(len(name)), *shape)
    xd = _dev(x)
    assert xd.data_ptr() % 16 == 0
    n = int(np.prod(out_shape))
    ints = [len(out_shape)] + out_shape + st + [n]
    got = _launch("TRANSPOSE", [xd.data_ptr() + 2 * off], n, ints, what=name)
    _check_bits(name, got, x[idx].contiguous())


def _slice_graph(name):
    gb = GraphBuilder()
    f32, i32 = gb.a_type(1), gb.a_type(3)
    shape = mk.SLICE_CASES[name][0]
    x = gb.placeholder("x", np.float32, [-1] + shape[1:],
                       signature_name="x")
    begin, end, step, shrink = {
        "cols_3_11": ([0, 3], [0, 11], [1, 1], 0),
        "stepped": ([0, 1, 2], [0, 8, 62], [1, 2, 3], 0),
        "cls": ([0, 0, 0], [0, 1, 0], [1, 1, 1], 0b010),
        "aligned_8_24": ([0, 8], [0, 24], [1, 1], 0),
    }[name]
    full = 0b101 if name == "cls" else 0b001        # dims taken whole
    y = gb.node("StridedSlice", "y",
                [x, gb.const("b", np.array(begin, np.int32)),
                 gb.const("e", np.array(end, np.int32)),
                 gb.const("s", np.array(step, np.int32))],
                T=f32, Index=i32, begin_mask=gb.a_int(full),
                end_mask=gb.a_int(full), shrink_axis_mask=gb.a_int(shrink),
                ellipsis_mask=gb.a_int(0), new_axis_mask=gb.a_int(0))
    gb.mark_output("y", y)
    return gb.build()


@pytest.mark.parametrize("name", list(mk.SLICE_CASES))
def test_strided_copy_graph(name, tmp_path):
    """The same slices as single-StridedSlice graphs through
    load_model_from_dir."""
    from tfservingcache_amd.engine.gpu import GpuModel
    shape, idx = mk.SLICE_CASES[name][:2]
    d = str(tmp_path / name / "1")
    write_saved_model(_slice_graph(name), d)
    lm = load_model_from_dir(d, name, 1)
    assert [op.kind for op in lm.plan.ops].count("strided_copy") == 1
    lm._gpu = GpuModel(lm.plan, device="cuda:0", max_batch=8,
                       model_name=name, model_version=1)
    try:
        x = mk.randn(mk.gen(len(name)), *shape)
        got = lm.predict({"x": x.float().numpy()})["y"]
        again = lm.predict({"x": x.float().numpy()})["y"]      # replay
    finally:
        lm._gpu.release()
    want = x[idx].contiguous()
    for g in (got, again):
        assert g.shape == tuple(want.shape)
        _check_bits(name, torch.from_numpy(np.ascontiguousarray(g)).to(BF16),
                    want)


def _scatter(src, dst_shape, offset, what):
    """src scattered into a sentinel-filled dst of dst_shape at `offset`
    elements; returns dst as a bf16 tensor."""
    n_dst = int(np.prod(dst_shape))
    ext = _ext()
    buf = _out_buffer(n_dst, BF16)
    s = _dev(src)
    ints = ([src.dim()] + list(src.shape) + mk.strides(dst_shape) +
            [src.numel()])
    ext.ExecPlan([(ext.K_SCATTER, [s.data_ptr(),
                                   buf.data_ptr() + 2 * offset],
                   ints, [])]).run()
    torch.cuda.synchronize()
    assert (buf[n_dst:].cpu() == _sentinel(BF16)).all(), \
        f"wrote past the end, {what}"
    return buf[:n_dst].cpu().view(*dst_shape)


@pytest.mark.parametrize("name,shapes,dst_shape,view", [
    ("concat_4x32", [[4, 32], [4, 32]], [4, 64], None),
    ("concat_odd", [[2, 3, 5], [2, 4, 5]], [2, 7, 5], None),
    # Pack on axis 1: each [4,32] input lands as [4,1,32] in [4,2,32]
    ("pack_axis1", [[4, 32], [4, 32]], [4, 2, 32], [4, 1, 32]),
])
def test_scatter(name, shapes, dst_shape, view):
    g = mk.gen(len(name))
    parts = [mk.randn(g, *s) for s in shapes]
    if view:
        parts = [p.view(*view) for p in parts]
    want_all = torch.cat(parts, dim=1)
    ostr = mk.strides(dst_shape)
    sent = _sentinel(BF16)
    off, lo = 0, 0
    for k, p in enumerate(parts):
        dst = _scatter(p, dst_shape, off, f"{name}[{k}]")
        hi = lo + p.shape[1]
        _check_bits(f"{name}[{k}] written part", dst[:, lo:hi], p)
        untouched = torch.cat([dst[:, :lo], dst[:, hi:]], dim=1)
        assert (untouched == sent).all(), f"{name}[{k}] wrote outside"
        off += p.shape[1] * ostr[1]
        lo = hi
    assert list(want_all.shape) == dst_shape


@pytest.mark.parametrize("row", [24, 7])
@pytest.mark.parametrize("idx", [[10], [0, 10, 3, 3, 7, 0, 10, 5, 1, 9, 2,
                                       10, 0]])
def test_gather(row, idx):
    table = mk.randn(mk.gen(row), 11, row)
    i = torch.tensor(idx, dtype=I32)
    what = f"gather row={row} n_idx={len(idx)}"
    got = _launch("GATHER", [_dev(table), _dev(i)], len(idx) * row,
                  [len(idx), row], what=what)
    _check_bits(what, got, table[i.long()].contiguous())


@pytest.mark.parametrize("pads", [(1, 2, 0, 3), (0, 0, 0, 0)])
def test_pad_nhwc(pads):
    pt, pb, pl, pr = pads
    x = mk.randn(mk.gen(3), 2, 3, 4, 5)
    want = torch.nn.functional.pad(x, (0, 0, pl, pr, pt, pb))
    assert list(want.shape) == [2, 3 + pt + pb, 4 + pl + pr, 5]
    got = _launch("PAD_NHWC", [_dev(x)], want.numel(),
                  [2, 3, 4, 5, pt, pb, pl, pr], what=f"pad{pads}")
    _check_bits(f"pad_nhwc{pads}", got, want.contiguous())


@pytest.mark.parametrize("c_in,c_out", [(3, 8), (8, 8)])
def test_pad_last(c_in, c_out):
    x = mk.randn(mk.gen(c_in), 5, c_in)
    want = torch.zeros(5, c_out, dtype=BF16)
    want[:, :c_in] = x
    got = _launch("PAD_LAST", [_dev(x)], 5 * c_out, [5, c_in, c_out],
                  what=f"pad_last {c_in}->{c_out}")
    _check_bits(f"pad_last {c_in}->{c_out}", got, want)


# -- elementwise -------------------------------------------------------------

def _elt(fn):
    return getattr(_ext(), "ELT_" + fn.upper())


def _unary(fn, n, seed):
    x = mk.unary_input(fn, n, seed)
    what = f"{fn} n={n}"
    got = _launch("ELT_UNARY", [_dev(x)], n, [n, _elt(fn)], what=what)
    xf = mk.f64(x)
    want = mk.ref_unary(fn, xf)
    _check(what, got, want, mk.unary_bound(fn, xf, want))
    return xf, got


@pytest.mark.parametrize("fn", mk.UNARY)
def test_unary(fn):
    for n in (1, 3, 4, 5, 1027):
        xf, _ = _unary(fn, n, seed=n)
        if n == 1027 and fn == "relu6":
            assert xf.min() < 0 and xf.max() > 6
        if n == 1027 and fn in ("sigmoid", "exp"):
            assert xf.min() <= -20 and xf.max() >= 20
        if fn in ("sqrt", "rsqrt"):
            assert xf.min() > 0


def test_unary_grid_stride():
    """Vector body and scalar tail both past one pass of the capped grid:
    relu is exact up to rounding, so any element missed or done twice
    shows."""
    _unary("relu", mk.GRID * 4 + 5, seed=2)


@pytest.mark.parametrize("fn", mk.BINARY)
def test_binary_same_shape(fn):
    for n in (3, 4, 1027):
        a, b = mk.binary_input(fn, [n], [n], seed=n)
        what = f"{fn} n={n}"
        got = _launch("ELT_BINARY", [_dev(a), _dev(b)], n,
                      [n, _elt(fn), 1, n, 1, 1], what=what)
        want = mk.ref_binary(fn, mk.f64(a), mk.f64(b))
        _check(what, got, want, mk.binary_bound(want))
        if fn == "div":
            assert not (mk.f64(b) == 0).any()


@pytest.mark.parametrize("fn", ["add", "div"])
@pytest.mark.parametrize("case", list(mk.BCAST_CASES))
def test_binary_broadcast(case, fn):
    sa, sb = mk.BCAST_CASES[case]
    a, b = mk.binary_input(fn, sa, sb, seed=len(case))
    ints = mk.bcast_ints(_elt(fn), sa, sb)
    want = mk.ref_binary(fn, mk.f64(a), mk.f64(b))
    assert want.size == ints[0] and ints[2] == want.ndim
    what = f"{fn} bcast {case}"
    # a 0-d operand still needs one element on the device
    got = _launch("ELT_BINARY", [_dev(a.reshape(-1)), _dev(b.reshape(-1))],
                  want.size, ints, what=what)
    _check(what, got, want, mk.binary_bound(want))


@pytest.mark.parametrize("act", mk.ACTS)
def test_bn_act(act):
    for rows, c in mk.BN_SHAPES:
        x, scale, shift = mk.bn_input(rows, c, seed=rows + c)
        what = f"bn_act {act} [{rows},{c}]"
        got = _launch("BN_ACT", [_dev(x), _dev(scale), _dev(shift)],
                      rows * c, [rows, c, mk.ACTS.index(act)], what=what)
        xf, sf, hf = mk.f64(x), mk.f64(scale), mk.f64(shift)
        want = mk.ref_bn_act(xf, sf, hf, act)
        bound, measured = mk.bn_bound(xf, sf, hf, act, want)
        if measured:
            print(f"{what}: float32 formula off by {measured:.3g}")
        _check(what, got, want, bound)
        if act == "relu6" and rows * c > 100:
            v = xf * sf + hf
            assert v.min() < 0 and v.max() > 6


def test_act_codes_match_the_extension():
    ext = _ext()
    for code, act in enumerate(mk.ACTS):
        assert getattr(ext, "ACT_" + act.upper()) == code


# -- row kernels -------------------------------------------------------------

def _softmax(x, what):
    rows, cols = x.shape
    got = _launch("SOFTMAX", [_dev(x)], rows * cols, [rows, cols], what=what)
    want = mk.ref_softmax(mk.f64(x))
    _check(what, got, want, mk.rowmax_bound(want))


@pytest.mark.parametrize("cols", mk.SOFTMAX_COLS)
def test_softmax(cols):
    _softmax(mk.softmax_input(5, cols, seed=cols), f"softmax [5,{cols}]")


@pytest.mark.parametrize("rows,cols", mk.SOFTMAX_GRID)
def test_softmax_grid_stride(rows, cols):
    _softmax(mk.softmax_input(rows, cols, seed=rows),
             f"softmax [{rows},{cols}]")


@pytest.mark.parametrize("cols", [64, 129, 513])
def test_softmax_all_neg_inf_row_is_nan(cols):
    x = mk.softmax_input(2, cols, seed=1, special=False)
    x[0] = float("-inf")
    got = mk.f64(_launch("SOFTMAX", [_dev(x)], 2 * cols, [2, cols],
                         what=f"softmax -inf [2,{cols}]")).reshape(2, cols)
    assert np.isnan(got[0]).all()
    want = mk.ref_softmax(mk.f64(x[1:]))
    assert np.all(np.abs(got[1:] - want) <= mk.rowmax_bound(want))


_LN = mk.layernorm_cases()


@pytest.mark.parametrize("eps", mk.LN_EPS)
@pytest.mark.parametrize("name", list(_LN))
def test_layernorm(name, eps):
    x, gamma, beta = _LN[name]
    rows, cols = x.shape
    what = f"layernorm {name} eps={eps}"
    got = _launch("LAYERNORM", [_dev(x), _dev(gamma), _dev(beta)],
                  rows * cols, [rows, cols], [eps], what=what)
    want = mk.ref_layernorm(mk.f64(x), mk.f64(gamma), mk.f64(beta), eps)
    _check(what, got, want, mk.rowmax_bound(want))
    if name.startswith("cols") or name.startswith("outliers"):
        # row 2 is constant: beta exactly
        _check_bits(what + " constant row", got.view(rows, cols)[2], beta)


@pytest.mark.parametrize("rows", mk.MEAN_LAST_ROWS)
@pytest.mark.parametrize("cols", mk.MEAN_LAST_COLS)
def test_mean_last(cols, rows):
    x = mk.mean_input((rows, cols), seed=rows + cols)
    what = f"mean_last [{rows},{cols}]"
    got = _launch("MEAN_LAST", [_dev(x)], rows, [rows, cols], what=what)
    xf = mk.f64(x)
    want = xf.mean(axis=1)
    _check(what, got, want, mk.mean_bound(xf, want, 1))


@pytest.mark.parametrize("d0,d1,d2", mk.MEAN_MID)
def test_mean_mid(d0, d1, d2):
    x = mk.mean_input((d0, d1, d2), seed=d1 + d2)
    what = f"mean_mid [{d0},{d1},{d2}]"
    got = _launch("MEAN_MID", [_dev(x)], d0 * d2, [d0, d1, d2], what=what)
    xf = mk.f64(x)
    want = xf.mean(axis=1)
    _check(what, got, want, mk.mean_bound(xf, want, 1))


def _argmax(x, what):
    rows, cols = x.shape
    got = _launch("ARGMAX_LAST", [_dev(x)], rows, [rows, cols], dtype=I32,
                  what=what).numpy()
    want = mk.ref_argmax(mk.f64(x))
    wrong = int((got != want).sum())
    print(f"{what}: {wrong} of {rows} rows differ")
    return got, want


@pytest.mark.parametrize("rows", mk.ARGMAX_ROWS)
@pytest.mark.parametrize("cols", mk.ARGMAX_COLS)
def test_argmax(cols, rows):
    x = mk.randn(mk.gen(rows + cols), rows, cols, scale=2.0)
    got, want = _argmax(x, f"argmax [{rows},{cols}]")
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("cols", mk.ARGMAX_COLS)
def test_argmax_special_rows(cols):
    x, names = mk.argmax_special(cols)
    got, want = _argmax(x, f"argmax special cols={cols}")
    for r, name in enumerate(names):
        print(f"  {name}: got {int(got[r])} want {int(want[r])}")
    for name in ("all_equal", "all_neg_inf", "all_-3.3e38"):
        assert want[names.index(name)] == 0
    assert dict(zip(names, got.tolist())) == dict(zip(names, want.tolist()))


def test_cast_i32_to_bf16():
    g = mk.gen(21)
    for n in mk.CAST_N:
        x = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g,
                          dtype=torch.int64).to(I32)
        k = min(n, len(mk.CAST_I2F_VALUES))
        x[:k] = torch.tensor(mk.CAST_I2F_VALUES[:k], dtype=torch.int64).to(
            I32)
        what = f"cast i32->bf16 n={n}"
        got = _launch("CAST", [_dev(x)], n, [n, 0], what=what)
        want = mk.ref_cast_i2bf(x.numpy())
        same = np.array_equal(mk.bits(got), want.view(np.int16))
        print(f"{what}: bit-identical={same}")
        assert same, what


def test_cast_bf16_to_i32():
    g = mk.gen(22)
    for n in mk.CAST_N:
        x = torch.randn(n, generator=g) * 1000.0
        k = min(n, len(mk.CAST_F2I_VALUES))
        x[:k] = torch.tensor(mk.CAST_F2I_VALUES[:k])
        x = x.to(BF16)
        what = f"cast bf16->i32 n={n}"
        got = _launch("CAST", [_dev(x)], n, [n, 1], dtype=I32,
                      what=what).numpy()
        want = mk.ref_cast_bf2i(mk.f64(x))
        print(f"{what}: {int((got != want).sum())} of {n} differ")
        np.testing.assert_array_equal(got, want)


def _neg_model(n, tmp_path):
    """x [-1, n] -> Neg -> y on the GPU, named for the fast path."""
    from tfservingcache_amd.engine.gpu import GpuModel
    gb = GraphBuilder()
    x = gb.placeholder("x", np.float32, [-1, n], signature_name="x")
    gb.mark_output("y", gb.node("Neg", "y", [x], T=gb.a_type(1)))
    name = f"neg{n}"
    d = str(tmp_path / name / "1")
    write_saved_model(gb.build(), d)
    lm = load_model_from_dir(d, name, 1)
    assert [op.kind for op in lm.plan.ops] == ["eltwise"]
    lm._gpu = GpuModel(lm.plan, device="cuda:0", max_batch=8,
                       model_name=name, model_version=1)
    return lm, name


@pytest.mark.parametrize("n", mk.F32_N)
def test_f32_bf16_staging_casts(n, tmp_path):
    """k_f32_to_bf16 and k_bf16_to_f32 run only inside the C++ fast
    predict path, on its staging buffers, with n = rows * row elements.
    A one-op Neg graph over [1, n] float32 puts them around a kernel that
    only flips the sign bit, so the response is -bf16(x) bit for bit:
    n = 1, 3, 4, 5, 1027 for the 4-wide body and the tail; +-0, the two
    round-to-nearest-even ties, FLT_MAX -> inf and NaN -> NaN (n = 1 sends
    one request per named value)."""
    from tfservingcache_amd.wire import messages as m
    from tfservingcache_amd.wire.tensor import (numpy_to_tensorproto,
                                                tensorproto_to_numpy)
    lm, name = _neg_model(n, tmp_path)
    try:
        warm = np.ones((1, n), np.float32)
        lm.predict({"x": warm})
        lm.predict({"x": warm})          # captured -> fast-registered
        assert lm._gpu._fast.has_bucket(1)
        runs0 = lm._gpu._fast.stats()[0]
        firsts = range(len(mk.F32_VALUES)) if n == 1 else [0]
        for first in firsts:
            x = mk.f32_input(n, seed=n, first=first)
            req = m.PredictRequest(
                model_spec=m.ModelSpec(name=name,
                                       version=m.Int64Value(value=1)),
                inputs={"x": numpy_to_tensorproto(x.reshape(1, n))}).encode()
            resp = m.PredictResponse.decode(lm._gpu.fast_predict(req))
            got = np.ascontiguousarray(
                tensorproto_to_numpy(resp.outputs["y"]), np.float32)
            assert got.shape == (1, n)
            got = got.reshape(n)
            want = -mk.ref_f32_to_bf16(x)
            nan = np.isnan(want)
            same = (np.array_equal(np.isnan(got), nan) and
                    np.array_equal(got.view(np.uint32)[~nan],
                                   want.view(np.uint32)[~nan]))
            print(f"f32->bf16->f32 n={n} first value {x[0]!r}: "
                  f"bit-identical={same}")
            assert same, (n, first)
        # the C++ path served them (a fallback would have raised)
        assert lm._gpu._fast.stats()[0] == runs0 + len(firsts)
    finally:
        lm._gpu.release()


# -- pooling -------------------------------------------------------------------

def _pool(x, is_max, geom, what):
    H, W, kh, kw, sh, sw, pt, _pb, pl, _pr = geom
    N, C = x.shape[0], x.shape[3]
    Ho, Wo = mk.pool_out_hw(geom)
    got = _launch("POOL", [_dev(x)], N * Ho * Wo * C,
                  [1 if is_max else 0, N, H, W, C, Ho, Wo, kh, kw, sh, sw,
                   pt, pl], what=what)
    xf = mk.f64(x)
    want = mk.ref_pool(xf, is_max, geom)
    bound = (np.zeros_like(want) if is_max
             else mk.avgpool_bound(xf, want, geom))
    _check(what, got, want, bound)


@pytest.mark.parametrize("mode", ["max", "avg"])
@pytest.mark.parametrize("name", list(mk.POOL_GEOM))
def test_pool(name, mode):
    geom = mk.POOL_GEOM[name]
    for C in mk.POOL_C:
        x = mk.randn(mk.gen(C), 2, geom[0], geom[1], C, shift=0.25)
        _pool(x, mode == "max", geom, f"{mode}pool {name} C={C}")


@pytest.mark.parametrize("C", [8, 3])
def test_max_pool_negative_inputs_with_padding(C):
    """Every input below zero: a pad treated as 0 would win at the
    border."""
    geom = mk.POOL_GEOM["3x3s2_same7"]
    x = (-torch.randn(2, 7, 7, C, generator=mk.gen(C)).abs() - 0.5).to(BF16)
    _pool(x, True, geom, f"maxpool negative C={C}")


@pytest.mark.parametrize("C", [8, 3])
def test_max_pool_of_neg_inf_is_neg_inf(C):
    geom = mk.POOL_GEOM["3x3s2_same7"]
    x = torch.full((2, 7, 7, C), float("-inf"), dtype=BF16)
    Ho, Wo = mk.pool_out_hw(geom)
    got = _launch("POOL", [_dev(x)], 2 * Ho * Wo * C,
                  [1, 2, 7, 7, C, Ho, Wo, 3, 3, 2, 2, 1, 1],
                  what=f"maxpool -inf C={C}")
    worst = float(mk.f64(got).max())
    print(f"maxpool -inf C={C}: largest output {worst}")
    assert np.all(np.isneginf(mk.f64(got)))
