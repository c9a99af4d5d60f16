// Which kernel launch_transpose picks. Plain C++ with no HIP types, so a
// host program can include and check it.
#pragma once

#include <cstdint>

namespace tfsc {

// k_transpose_v8 moves 16-byte chunks: out[..., 8g..8g+7] comes from
// x + (sum of outer coords * in_strides) + 8g. Every such address is
// 16-byte aligned iff the last dim stays innermost (stride 1) and is a
// multiple of 8 elements, both base pointers are 16-byte aligned, and
// every other input stride is a multiple of 8 elements. A strided_copy
// arrives here with an offset source pointer and the sliced tensor's
// outer strides (x[:, 3:11] of [4, 20]: 6 bytes off, row stride 20), so
// the shape alone does not decide.
inline bool transpose_takes_v8(const void* x, const void* y, int ndim,
                               const int64_t* out_dims,
                               const int64_t* in_strides) {
  if (ndim < 2 || in_strides[ndim - 1] != 1 || out_dims[ndim - 1] % 8 != 0)
    return false;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15u)
    return false;
  for (int d = 0; d < ndim - 1; ++d)
    if (in_strides[d] % 8 != 0) return false;
  return true;
}

}  // namespace tfsc
