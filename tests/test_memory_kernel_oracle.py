"""CPU-side checks of what test_gpu_memory_kernels.py relies on
(memory_kernel_oracle.py): the float64 references agree with torch where
torch has the operation, the inputs can tell a wrong kernel from a right
one, and launch_transpose's vector gate, compiled for the host, sends
each strided copy to the kernel it is safe on.

Softmax without the max subtraction: on the +-40 row exp() stays inside
float32 (e^40 = 2.4e17), so the naive float32 form is as good as the
stable one there (measured: 3e-6 of the bound at 65 columns, 1.5e-5 of
it at 513) and that row cannot tell the two apart. The +-100 row can (e^100 overflows
float32) and is what the check below asserts on; the +-40 figure is
asserted to be inside the bound so that this stays known.
"""
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import torch

import memory_kernel_oracle as mk

CSRC = (Path(__file__).resolve().parent.parent / "tfservingcache_amd" /
        "engine" / "csrc")


def test_softmax_reference_matches_torch():
    for cols in mk.SOFTMAX_COLS:
        x = mk.softmax_input(5, cols, seed=cols)
        want = torch.softmax(x.to(torch.float64), dim=-1).numpy()
        np.testing.assert_allclose(mk.ref_softmax(mk.f64(x)), want,
                                   rtol=1e-12, atol=1e-300)


def test_layernorm_reference_matches_torch():
    for name, (x, gamma, beta) in mk.layernorm_cases().items():
        for eps in mk.LN_EPS:
            want = torch.nn.functional.layer_norm(
                x.to(torch.float64), (x.shape[-1],), gamma.to(torch.float64),
                beta.to(torch.float64), eps).numpy()
            got = mk.ref_layernorm(mk.f64(x), mk.f64(gamma), mk.f64(beta),
                                   eps)
            # float64 on both sides; a constant row divides 0 by sqrt(eps)
            np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9,
                                       err_msg=f"{name} eps={eps}")


def test_pool_reference_matches_torch_on_symmetric_pads():
    F = torch.nn.functional
    for name, geom in mk.POOL_GEOM.items():
        H, W, kh, kw, sh, sw, pt, pb, pl, pr = geom
        if pt != pb or pl != pr:
            continue
        x = mk.randn(mk.gen(3), 2, H, W, 12)
        xt = x.to(torch.float64).permute(0, 3, 1, 2)
        mx = F.max_pool2d(xt, (kh, kw), (sh, sw), (pt, pl))
        av = F.avg_pool2d(xt, (kh, kw), (sh, sw), (pt, pl),
                          count_include_pad=False)
        np.testing.assert_array_equal(
            mk.ref_pool(mk.f64(x), True, geom),
            mx.permute(0, 2, 3, 1).numpy(), err_msg=name)
        np.testing.assert_allclose(
            mk.ref_pool(mk.f64(x), False, geom),
            av.permute(0, 2, 3, 1).numpy(), rtol=1e-12, atol=1e-15,
            err_msg=name)


def test_argmax_reference_matches_torch():
    for cols in mk.ARGMAX_COLS:
        x, names = mk.argmax_special(cols)
        want = torch.argmax(x.to(torch.float64), dim=-1).numpy()
        np.testing.assert_array_equal(mk.ref_argmax(mk.f64(x)), want, names)
        r = mk.randn(mk.gen(cols), 5, cols, scale=2.0)
        np.testing.assert_array_equal(
            mk.ref_argmax(mk.f64(r)),
            torch.argmax(r.to(torch.float64), dim=-1).numpy())


def test_cast_reference_matches_torch():
    g = mk.gen(11)
    x = torch.cat([torch.tensor(mk.CAST_I2F_VALUES, dtype=torch.int32),
                   torch.randint(-2 ** 31, 2 ** 31 - 1, (4096,), generator=g,
                                 dtype=torch.int64).to(torch.int32)])
    want = x.to(torch.float32).to(torch.bfloat16)
    got = mk.ref_cast_i2bf(x.numpy())
    np.testing.assert_array_equal(got.view(np.int16), mk.bits(want))
    # 16842753 = 2^24 + 2^16 + 1 rounds DOWN twice (two ties to even);
    # one rounding straight from the integer would go up
    assert float(want[7]) == 2.0 ** 24
    f = mk.bf(mk.CAST_F2I_VALUES)
    np.testing.assert_array_equal(mk.ref_cast_bf2i(mk.f64(f)),
                                  [2, -2, 0, 0, 0, int(float(f[5]))])


def test_f32_to_bf16_reference_matches_torch():
    x = np.concatenate([mk.f32_input(n, seed=n, first=f)
                        for n in mk.F32_N
                        for f in range(len(mk.F32_VALUES))])
    want = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    got = mk.ref_f32_to_bf16(x)
    nan = np.isnan(want)
    assert nan.any() and np.array_equal(np.isnan(got), nan)
    np.testing.assert_array_equal(got.view(np.uint32)[~nan],
                                  want.view(np.uint32)[~nan])
    for v, w in mk.F32_VALUES:
        g = mk.ref_f32_to_bf16(np.array([v], np.float32))[0]
        assert (np.isnan(w) and np.isnan(g)) or (
            g == w and np.signbit(g) == np.signbit(np.float32(w))), (v, w)


def _ln_ratio(one_pass, x, gamma, beta, eps):
    """|emulation - reference| / bound, per element."""
    want = mk.ref_layernorm(mk.f64(x), mk.f64(gamma), mk.f64(beta), eps)
    got = mk.f32_layernorm(mk.f64(x), mk.f64(gamma), mk.f64(beta), eps,
                           one_pass)
    return np.abs(got - want) / mk.rowmax_bound(want)


def test_one_pass_variance_misses_the_eight_outlier_row():
    x, gamma, beta = mk.layernorm_cases()["outliers_bare"]
    row0 = float(_ln_ratio(True, x, gamma, beta, 1e-12)[0].max())
    print(f"one-pass E[x^2]-mean^2 on the eight-outlier row: "
          f"{row0:.2f} x the bound")
    assert row0 > 5.0


def test_two_pass_variance_meets_every_layernorm_bound():
    for name, (x, gamma, beta) in mk.layernorm_cases().items():
        for eps in mk.LN_EPS:
            worst = float(_ln_ratio(False, x, gamma, beta, eps).max())
            print(f"two-pass {name} eps={eps}: {worst:.3g} x the bound")
            assert worst <= 1.0, (name, eps, worst)


def _naive_softmax32(x):
    e = np.exp(x.astype(np.float32))
    with np.errstate(invalid="ignore"):
        return (e / e.sum(axis=-1, keepdims=True)).astype(np.float64)


def test_softmax_without_max_subtraction_misses():
    for cols in (65, 513):
        x = mk.f64(mk.softmax_input(5, cols, seed=cols))
        want = mk.ref_softmax(x)
        with np.errstate(over="ignore"):
            got = _naive_softmax32(x)
        ratio = np.abs(got - want) / mk.rowmax_bound(want)
        # nan counts as a miss
        assert not np.all(ratio[mk.SM_SPREAD100] <= 1.0)
        # see the module docstring: no float32 overflow at +-40
        print(f"cols={cols}: naive float32 softmax on the +-40 row is "
              f"{float(ratio[mk.SM_SPREAD40].max()):.3g} x the bound")
        assert np.all(ratio[mk.SM_SPREAD40] <= 1.0)


def test_average_by_window_size_misses_on_padded_cases():
    for name in mk.POOL_PADDED:
        geom = mk.POOL_GEOM[name]
        x = mk.f64(mk.randn(mk.gen(5), 2, geom[0], geom[1], 8, shift=1.0))
        want = mk.ref_pool(x, False, geom)
        wrong = mk.ref_pool(x, False, geom, divide_by_window=True)
        assert (np.abs(wrong - want) >
                mk.avgpool_bound(x, want, geom)).any(), name


def test_last_maximum_misses_on_tie_rows():
    for cols in (63, 64, 65, 1000):
        x, names = mk.argmax_special(cols)
        v = mk.f64(x)
        last = cols - 1 - np.argmax(v[:, ::-1], axis=-1)
        want = mk.ref_argmax(v)
        for tie in ("tie_3_4", "tie_3_67", "all_equal"):
            if tie in names:
                r = names.index(tie)
                assert want[r] == (0 if tie == "all_equal" else 3)
                assert last[r] != want[r], (cols, tie)
    assert "tie_3_67" in mk.argmax_special(1000)[1]


def test_transcendental_terms_are_small():
    """The measured float32 errors that enter the unary bounds; the GPU
    file's docstring quotes them."""
    for fn, mode in mk.TRANSCENDENTAL.items():
        worst = 0.0
        for n in (1, 3, 4, 5, 1027):
            x = mk.f64(mk.unary_input(fn, n, seed=n))
            _, m = mk.transcendental_term(fn, x.astype(np.float32),
                                          mk.ref_unary(fn, x))
            worst = max(worst, m)
        print(f"{fn}: float32 formula off by {worst:.3g} ({mode})")
        assert worst < 2.0 ** -20


# (what, x offset, y offset, out dims, in strides, takes the 16-byte path):
# the transposes of the GPU file and a few neighbours of its slices; the
# strided copies themselves come from mk.SLICE_CASES
_GATE_EXTRA = [
    ("head split", 0, 0, [2, 4, 3, 8], [96, 8, 32, 1], True),
    ("last dim 12", 0, 0, [2, 4, 3, 12], [144, 12, 48, 1], False),
    ("last dim moves", 0, 0, [2, 8, 3, 4], [96, 1, 32, 8], False),
    ("row stride 20 alone", 0, 0, [4, 8], [20, 1], False),
    ("x[:, 4:20] of [4,32]", 4, 0, [4, 16], [32, 1], False),
    ("unaligned destination", 0, 1, [4, 16], [32, 1], False),
    ("rank 1", 0, 0, [64], [1], False),
]

_GATE_HEAD = r"""
#include <cstdio>
#include <cstdint>
#include "transpose_gate.h"
int main() {
  using tfsc::transpose_takes_v8;
  alignas(16) static unsigned short x[4096], y[4096];
  int bad = 0;
  auto expect = [&](const char* what, bool got, bool want) {
    if (got != want) { std::printf("%s: got %d want %d\n", what, got, want); ++bad; }
  };
"""


def _gate_program():
    cases = [(f"slice {name}", off, 0, out, st, v8)
             for name, (_shape, _idx, off, out, st, v8)
             in mk.SLICE_CASES.items()] + _GATE_EXTRA
    body = []
    for what, xo, yo, dims, st, v8 in cases:
        body.append(
            "  { int64_t d[] = {%s}, s[] = {%s};\n"
            "    expect(\"%s\", transpose_takes_v8(x + %d, y + %d, %d, d, s),"
            " %s); }\n" % (", ".join(map(str, dims)),
                           ", ".join(map(str, st)), what, xo, yo, len(dims),
                           "true" if v8 else "false"))
    return _GATE_HEAD + "".join(body) + "  return bad;\n}\n"


def _host_compiler():
    """g++, else another host C++ compiler; the last one is the clang++
    that ships with ROCm, which the extension's own build needs."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for cc in ("g++", "c++", "clang++",
               os.path.join(rocm, "lib", "llvm", "bin", "clang++")):
        path = shutil.which(cc)
        if path:
            return path
    return None


def test_transpose_vector_gate_on_the_host(tmp_path):
    """transpose_gate.h as a stand-alone host program under ASan/UBSan:
    every strided-copy case of the GPU file takes the kernel its table
    entry says, and so do the transposes."""
    cxx = _host_compiler()
    assert cxx is not None, "no host C++ compiler, not even ROCm's clang++"
    src = tmp_path / "gate.cpp"
    src.write_text(_gate_program())
    exe = tmp_path / "gate"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", f"-I{CSRC}", str(src),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_slice_cases_describe_their_slices():
    """offset, strides and output shape of each strided-copy case are the
    slice they name."""
    for name, (shape, idx, off, out, st, _v8) in mk.SLICE_CASES.items():
        n = int(np.prod(shape))
        flat = np.arange(n)
        want = flat.reshape(shape)[idx]
        assert list(want.shape) == out, name
        got = np.lib.stride_tricks.as_strided(
            flat[off:], out, [s * flat.itemsize for s in st])
        np.testing.assert_array_equal(got, want, err_msg=name)
