"""float64 references, input generators and derived bounds for the
memory-bound kernels (ops_memory.hip). Shared by
test_gpu_memory_kernels.py, which runs the kernels, and
test_memory_kernel_oracle.py, which checks on the CPU that these
references are right and that the inputs can tell a wrong kernel from a
right one. The derivations of the bounds are in the GPU file's docstring.

Every input is generated from a seeded torch.Generator and rounded to
bf16 before anybody sees it; every reference is numpy float64 written
from the operation's definition.
"""
import math

import numpy as np
import torch

EPS_BF16 = 2.0 ** -8          # twice one bf16 rounding (2^-9 relative)
TINY = 2.0 ** -126            # bf16's smallest normal
GRID = 2048 * 256             # threads in a capped grid


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(g, *shape, scale=1.0, shift=0.0):
    return (torch.randn(*shape, generator=g) * scale + shift).to(
        torch.bfloat16)


def bf(values):
    return torch.tensor(values, dtype=torch.float32).to(torch.bfloat16)


def f64(t):
    return t.to(torch.float64).numpy()


def bits(t):
    return t.contiguous().view(torch.int16).numpy()


def strides(shape):
    st = [1] * len(shape)
    for d in range(len(shape) - 2, -1, -1):
        st[d] = st[d + 1] * shape[d + 1]
    return st


# -- elementwise ---------------------------------------------------------------

UNARY = ["relu", "tanh", "sigmoid", "erf", "sqrt", "rsqrt", "exp", "neg",
         "square", "gelu", "relu6"]
BINARY = ["add", "sub", "mul", "div", "max", "min", "sqdiff"]
ACTS = ["none", "relu", "tanh", "sigmoid", "gelu", "relu6"]   # code = index
# how the measured float32 error of a transcendental enters its bound:
# relative to |want| where the function is a bare exponential, absolute
# where it ends in an addition that can cancel
TRANSCENDENTAL = {"tanh": "abs", "erf": "abs", "gelu": "abs",
                  "sigmoid": "rel", "exp": "rel"}

_UNARY_EDGES = {
    "relu6": [-1.0, 7.5, 6.0, 0.0, 3.0],
    "sigmoid": [-20.0, 20.0, -0.0, 10.0, -10.0],
    "exp": [-20.0, 20.0, -0.0, 10.0, -10.0],
    "sqrt": [4.0, 1.0e-3, 1.0e4, 1.0, 2.0],
    "rsqrt": [4.0, 1.0e-3, 1.0e4, 1.0, 2.0],
}
_DEFAULT_EDGES = [-5.0, 5.0, -0.0, 0.0, -3.0]


def unary_input(fn, n, seed):
    """Both sides of every clamp; positives only for sqrt and rsqrt."""
    g = gen(seed)
    if fn in ("sqrt", "rsqrt"):
        x = torch.randn(n, generator=g).abs() * 4.0 + 2.0 ** -6
    elif fn in ("sigmoid", "exp"):
        x = torch.randn(n, generator=g) * 6.0
    elif fn == "relu6":
        x = torch.randn(n, generator=g) * 4.0 + 3.0
    else:
        x = torch.randn(n, generator=g) * 3.0
    edges = _UNARY_EDGES.get(fn, _DEFAULT_EDGES)
    k = min(n, len(edges))
    x[:k] = torch.tensor(edges[:k])
    return x.to(torch.bfloat16)


_erf64 = np.vectorize(math.erf, otypes=[np.float64])


def _erf32(v):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(v))).numpy()


def ref_unary(fn, x):
    """x: float64 array."""
    if fn == "relu":
        return np.where(x > 0, x, 0.0)
    if fn == "tanh":
        return np.tanh(x)
    if fn == "sigmoid":
        return 1.0 / (1.0 + np.exp(-x))
    if fn == "erf":
        return _erf64(x)
    if fn == "sqrt":
        return np.sqrt(x)
    if fn == "rsqrt":
        return 1.0 / np.sqrt(x)
    if fn == "exp":
        return np.exp(x)
    if fn == "neg":
        return -x
    if fn == "square":
        return x * x
    if fn == "gelu":
        return 0.5 * x * (1.0 + _erf64(x / math.sqrt(2.0)))
    if fn == "relu6":
        return np.clip(x, 0.0, 6.0)
    if fn == "none":
        return x
    raise KeyError(fn)


def f32_unary(fn, x):
    """The kernel's formula, plainly, in float32 (x: float32 array)."""
    one, half = np.float32(1.0), np.float32(0.5)
    if fn == "tanh":
        return np.tanh(x)
    if fn == "sigmoid":
        return one / (one + np.exp(-x))
    if fn == "erf":
        return _erf32(x)
    if fn == "exp":
        return np.exp(x)
    if fn == "gelu":
        return half * x * (one + _erf32(x * np.float32(0.70710678)))
    raise KeyError(fn)


def transcendental_term(fn, x32, want):
    """(4 x the measured float32 error as a per-element bound term, the
    measured maximum)."""
    mode = TRANSCENDENTAL[fn]
    err = np.abs(f32_unary(fn, x32).astype(np.float64) - want)
    if mode == "rel":
        m = float(np.max(err / np.abs(want)))
        return 4.0 * m * np.abs(want), m
    m = float(np.max(err))
    return np.full(want.shape, 4.0 * m), m


def unary_bound(fn, x, want):
    b = EPS_BF16 * np.abs(want) + TINY
    if fn in TRANSCENDENTAL:
        b = b + transcendental_term(fn, x.astype(np.float32), want)[0]
    return b


def binary_input(fn, shape_a, shape_b, seed):
    g = gen(seed)
    a = torch.randn(tuple(shape_a), generator=g) * 3.0
    b = torch.randn(tuple(shape_b), generator=g) * 3.0
    if fn == "div":                                  # no zero divisors
        b = torch.where(b < 0, -1.0, 1.0) * (b.abs() * 2.0 + 0.25)
    return a.to(torch.bfloat16), b.to(torch.bfloat16)


def ref_binary(fn, a, b):
    return {"add": lambda: a + b, "sub": lambda: a - b,
            "mul": lambda: a * b, "div": lambda: a / b,
            "max": lambda: np.maximum(a, b),
            "min": lambda: np.minimum(a, b),
            "sqdiff": lambda: (a - b) ** 2}[fn]()


def binary_bound(want):
    return EPS_BF16 * np.abs(want) + TINY


# (a shape, b shape); a [] is a scalar
BCAST_CASES = {
    "last": ([2, 3, 4], [4]),
    "middle": ([2, 3, 4], [2, 1, 4]),
    "both": ([2, 1, 4], [1, 3, 1]),
    "left": ([1, 4], [3, 2, 4]),
    "scalar": ([2, 3, 4], []),
    "six": ([2, 1, 3, 1, 2, 2], [1, 2, 1, 3, 2, 1]),
}


def bcast_ints(n_fn, a_shape, b_shape):
    """[n_out, fn, ndim, dims, sa, sb]: element strides of each operand
    over the output's dims, 0 where it is broadcast."""
    out = list(np.broadcast_shapes(tuple(a_shape), tuple(b_shape)))
    nd = len(out)

    def st(shape):
        shape = [1] * (nd - len(shape)) + list(shape)
        cs = strides(shape)
        return [0 if shape[d] == 1 else cs[d] for d in range(nd)]

    return [int(np.prod(out)), n_fn, nd] + out + st(a_shape) + st(b_shape)


BN_SHAPES = [(5, 3), (4, 8), (1, 1), (3, 1000), (1030, 512)]


def bn_input(rows, c, seed):
    g = gen(seed)
    return (randn(g, rows, c, scale=3.0), randn(g, c, scale=1.5),
            randn(g, c, scale=2.0))


def ref_bn_act(x, scale, shift, act):
    return ref_unary(act, x * scale + shift)


def bn_bound(x, scale, shift, act, want):
    b = (EPS_BF16 * np.abs(want) + TINY +
         2.0 ** -22 * (np.abs(x * scale) + np.abs(shift)))
    m = 0.0
    if act in TRANSCENDENTAL:
        x32, s32, h32 = (v.astype(np.float32) for v in (x, scale, shift))
        got32 = f32_unary(act, x32 * s32 + h32).astype(np.float64)
        m = float(np.max(np.abs(got32 - want)))
        b = b + 4.0 * m
    return b, m


# -- row kernels ---------------------------------------------------------------

SOFTMAX_COLS = [1, 63, 64, 65, 128, 129, 512, 513, 1000]
SOFTMAX_GRID = [(8200, 8), (2050, 513)]
SM_MASKED, SM_EQUAL, SM_SPREAD40, SM_SPREAD100 = 1, 2, 3, 4


def softmax_input(rows, cols, seed, special=True):
    """4*N(0,1); with special, row 1 has every other entry at -1e9, row 2
    is all-equal, row 3 runs over +-40 and row 4 over +-100 (the only one
    on which exp overflows float32 without the max subtraction)."""
    x = torch.randn(rows, cols, generator=gen(seed)) * 4.0
    if special:
        x[SM_MASKED, ::2] = -1.0e9
        x[SM_EQUAL] = 1.5
        x[SM_SPREAD40] = torch.linspace(-40.0, 40.0, cols)
        x[SM_SPREAD100] = torch.linspace(-100.0, 100.0, cols)
    return x.to(torch.bfloat16)


def ref_softmax(x):
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def rowmax_bound(want):
    return (EPS_BF16 * np.abs(want).max(axis=-1, keepdims=True) + TINY +
            np.zeros_like(want))


LN_COLS = [1, 8, 255, 256, 257, 768, 1000]
LN_EPS = [1e-12, 1e-5]
OUTLIERS_8 = [0, 100, 200, 300, 400, 500, 600, 700]
OUTLIERS_2 = [5, 600]


def layernorm_cases():
    """name -> (x [rows, cols], gamma, beta), all bf16. Every case runs
    at both eps."""
    cases = {}
    for cols in LN_COLS:
        g = gen(1000 + cols)
        x = torch.randn(3, cols, generator=g)
        x[1] += 100.0
        x[2] = 3.25                                   # constant row
        cases[f"cols{cols}"] = (x.to(torch.bfloat16), randn(g, cols),
                                randn(g, cols))
    g = gen(7)
    x = torch.randn(2050, 64, generator=g)
    x[1::2] += 100.0
    cases["rows2050"] = (x.to(torch.bfloat16), randn(g, 64), randn(g, 64))
    x = torch.full((3, 768), 256.0)
    x[0, OUTLIERS_8] = 258.0
    x[1, OUTLIERS_2] = 258.0
    x = x.to(torch.bfloat16)
    cases["outliers_bare"] = (x, bf([1.0] * 768), bf([0.0] * 768))
    cases["outliers_affine"] = (x, randn(g, 768), randn(g, 768))
    return cases


def ref_layernorm(x, gamma, beta, eps):
    mean = x.mean(axis=-1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=-1, keepdims=True)
    return (x - mean) / np.sqrt(var + eps) * gamma + beta


def _f32_block_sum(v):
    """Sum of a float32 row the way a 256-thread block does it: a serial
    partial per thread over i = t, t+256, ..., then a halving tree over
    each wave of 64 and over the four wave sums."""
    part = np.zeros(256, np.float32)
    for i0 in range(0, len(v), 256):
        chunk = v[i0:i0 + 256]
        part[:len(chunk)] += chunk
    w = part.reshape(4, 64).copy()
    off = 32
    while off:
        w[:, :off] = w[:, :off] + w[:, off:2 * off]
        off //= 2
    s = w[:, 0].copy()
    s[:2] = s[:2] + s[2:4]
    return np.float32(s[0] + s[1])


def f32_layernorm(x, gamma, beta, eps, one_pass):
    """float32 emulation of the layernorm kernel. one_pass is the
    var = E[x^2] - mean^2 form with its var > 0 clamp; otherwise the mean
    comes first and var is the mean of squared deviations from it."""
    x, gamma, beta = (v.astype(np.float32) for v in (x, gamma, beta))
    out = np.empty(x.shape, np.float32)
    cols = np.float32(x.shape[-1])
    eps = np.float32(eps)
    for r, row in enumerate(x):
        mean = _f32_block_sum(row) / cols
        if one_pass:
            var = _f32_block_sum(row * row) / cols - mean * mean
            rstd = np.float32(1.0) / np.sqrt(var + eps if var > 0 else eps)
        else:
            d = row - mean
            var = _f32_block_sum(d * d) / cols
            rstd = np.float32(1.0) / np.sqrt(var + eps)
        out[r] = (row - mean) * rstd * gamma + beta
    return out.astype(np.float64)


MEAN_LAST_COLS = [1, 255, 256, 257, 4096]
MEAN_LAST_ROWS = [1, 3, 2050]
MEAN_MID = [(2, 49, 8), (3, 7, 5), (1, 1, 1), (2, 1, 300), (2, 2, 262145)]


def mean_input(shape, seed):
    return randn(gen(seed), *shape, shift=0.5)


def mean_bound(x, want, axis):
    """x: the float64 input; want = x.mean(axis)."""
    n = x.shape[axis]
    return (EPS_BF16 * np.abs(want) + TINY +
            n * 2.0 ** -24 * np.abs(x).mean(axis=axis))


ARGMAX_COLS = [1, 63, 64, 65, 1000]
ARGMAX_ROWS = [1, 5, 8200]


def argmax_special(cols):
    """(x [k, cols] bf16, names). Ties between neighbouring lanes (3, 4)
    and inside one lane (3, 67) where the row is long enough."""
    g = gen(cols)
    rows, names = [], []

    def add(name, row):
        names.append(name)
        rows.append(row)

    base = torch.randn(cols, generator=g)
    add("all_equal", torch.full((cols,), 0.75))
    last = base.clone()
    last[cols - 1] = 50.0
    add("max_last", last)
    add("all_negative", -base.abs() - 1.0)
    add("all_neg_inf", torch.full((cols,), float("-inf")))
    add("all_-3.3e38", torch.full((cols,), -3.3e38))
    if cols > 4:
        t = base.clone()
        t[3] = t[4] = 40.0
        add("tie_3_4", t)
    if cols > 67:
        t = base.clone()
        t[3] = t[67] = 40.0
        add("tie_3_67", t)
    return torch.stack(rows).to(torch.bfloat16), names


def ref_argmax(x):
    """First index holding the row's maximum."""
    out = np.empty(x.shape[0], np.int32)
    for r, row in enumerate(x):
        out[r] = np.flatnonzero(row == row.max())[0]
    return out


CAST_N = [1, 257, GRID + 3]
CAST_I2F_VALUES = [0, 1, -1, 255, 256, 257, 259, 16842753, 2 ** 31 - 1,
                   -2 ** 31]
CAST_F2I_VALUES = [2.875, -2.875, 0.996, -0.996, -0.0, 1.0e9]


def ref_cast_i2bf(x):
    """int32 -> float32 -> bf16, both round-to-nearest-even; returns the
    bf16 bit patterns as uint16."""
    u = x.astype(np.int64).astype(np.float32).view(np.uint32).astype(
        np.uint64)
    u = u + 0x7FFF + ((u >> 16) & 1)
    return (u >> 16).astype(np.uint16)


def ref_cast_bf2i(x):
    return np.trunc(x).astype(np.int32)


# f32 <-> bf16 staging conversions of the fast predict path
F32_N = [1, 3, 4, 5, 1027]
FLT_MAX = float(np.finfo(np.float32).max)
# (value, bf16 it must round to): signed zeros, both directions of a
# round-to-nearest-even tie, overflow to inf, NaN
F32_VALUES = [(0.0, 0.0), (-0.0, -0.0), (1.00390625, 1.0),
              (1.01171875, 1.015625), (FLT_MAX, float("inf")),
              (-FLT_MAX, float("-inf")), (float("nan"), float("nan"))]


def f32_input(n, seed, first=0):
    """float32 [n] that is NOT pre-rounded to bf16 (the rounding is what is
    under test): N(0,1)*3 with the named values from position 0 on,
    starting with F32_VALUES[first]."""
    x = (torch.randn(n, generator=gen(seed)) * 3.0).numpy()
    vals = [v for v, _ in F32_VALUES[first:] + F32_VALUES[:first]]
    k = min(n, len(vals))
    x[:k] = np.array(vals[:k], np.float32)
    return x


def ref_f32_to_bf16(x):
    """float32 array -> the float32 value of its round-to-nearest-even
    bf16 (NaN stays NaN), from the definition on the bit pattern."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    out = r.astype(np.uint32).view(np.float32).copy()
    out[np.isnan(x)] = np.nan
    return out


# -- pooling -------------------------------------------------------------------

# name -> (H, W, kh, kw, sh, sw, pt, pb, pl, pr)
POOL_GEOM = {
    "3x3s2_same7": (7, 7, 3, 3, 2, 2, 1, 1, 1, 1),
    "3x3s2_same6": (6, 6, 3, 3, 2, 2, 0, 1, 0, 1),
    "2x2s2_valid6": (6, 6, 2, 2, 2, 2, 0, 0, 0, 0),
    "3x3s1_same5": (5, 5, 3, 3, 1, 1, 1, 1, 1, 1),
    "1x3_s21": (5, 6, 1, 3, 2, 1, 0, 0, 1, 1),
    "window_is_image": (4, 4, 4, 4, 1, 1, 0, 0, 0, 0),
}
POOL_C = [8, 16, 3, 12]
POOL_PADDED = ["3x3s2_same7", "3x3s2_same6", "3x3s1_same5", "1x3_s21"]


def pool_out_hw(geom):
    H, W, kh, kw, sh, sw, pt, pb, pl, pr = geom
    return (H + pt + pb - kh) // sh + 1, (W + pl + pr - kw) // sw + 1


def ref_pool(x, is_max, geom, divide_by_window=False):
    """Direct loop over NHWC float64 x. Average divides by the number of
    taps inside the image (divide_by_window is the wrong rule, kept for
    the sharpness check)."""
    H, W, kh, kw, sh, sw, pt, _pb, pl, _pr = geom
    Ho, Wo = pool_out_hw(geom)
    N, C = x.shape[0], x.shape[3]
    out = np.empty((N, Ho, Wo, C), np.float64)
    for ho in range(Ho):
        for wo in range(Wo):
            taps = [x[:, hi, wi, :]
                    for hi in range(ho * sh - pt, ho * sh - pt + kh)
                    for wi in range(wo * sw - pl, wo * sw - pl + kw)
                    if 0 <= hi < H and 0 <= wi < W]
            t = np.stack(taps)
            if is_max:
                out[:, ho, wo, :] = t.max(axis=0)
            else:
                out[:, ho, wo, :] = t.sum(axis=0) / (
                    kh * kw if divide_by_window else len(taps))
    return out


def avgpool_bound(x, want, geom):
    return (EPS_BF16 * np.abs(want) + TINY +
            geom[2] * geom[3] * 2.0 ** -24 * float(np.abs(x).max()))


# -- strided copies --------------------------------------------------------------

# name -> (input shape, numpy index, offset in elements, output shape,
#          input stride per output dim, takes the 16-byte path)
SLICE_CASES = {
    "cols_3_11": ([4, 20], np.s_[:, 3:11], 3, [4, 8], [20, 1], False),
    "stepped": ([4, 9, 64], np.s_[:, 1:8:2, 2:62:3], 66, [4, 4, 20],
                [576, 128, 3], False),
    "cls": ([4, 9, 64], np.s_[:, 0, :], 0, [4, 64], [576, 1], True),
    "aligned_8_24": ([4, 32], np.s_[:, 8:24], 8, [4, 16], [32, 1], True),
}
