// Memory-bound serving kernels for gfx950: elementwise, fused BN+act,
// softmax, layernorm, reductions, pooling, transpose, gather, pad.
//
// All are HBM-bandwidth-bound: bf16 I/O is vectorized as ushort4/8 where
// the layout permits (cdna_hip_programming.md G13), grids are capped and
// grid-stride (G11), accumulation is f32.
#include "../common.h"
#include "../kernels.h"
#include "../transpose_gate.h"

#include <stdexcept>
#include <string>

namespace tfsc {

constexpr int TPB = 256;
constexpr int MAX_BLOCKS = 2048;   // 256 CU * 8 blocks/CU

static inline int grid_for(int64_t n, int per_thread = 1) {
  int64_t blocks = ceil_div(n, int64_t(TPB) * per_thread);
  return int(blocks < MAX_BLOCKS ? (blocks > 0 ? blocks : 1) : MAX_BLOCKS);
}

// ---------------------------------------------------------------------------
// elementwise
// ---------------------------------------------------------------------------
TFSC_DEV float apply_unary(float v, int fn) {
  switch (fn) {
    case ELT_RELU: return v > 0.f ? v : 0.f;
    case ELT_TANH: return tanhf(v);
    case ELT_SIGMOID: return 1.f / (1.f + __expf(-v));
    case ELT_ERF: return erff(v);
    case ELT_SQRT: return sqrtf(v);
    case ELT_RSQRT: return rsqrtf(v);
    case ELT_EXP: return __expf(v);
    case ELT_NEG: return -v;
    case ELT_SQUARE: return v * v;
    case ELT_GELU: return 0.5f * v * (1.f + erff(v * 0.70710678f));
    case ELT_RELU6: return v < 0.f ? 0.f : (v > 6.f ? 6.f : v);
    default: return v;
  }
}

TFSC_DEV float apply_binary(float a, float b, int fn) {
  switch (fn) {
    case ELT_ADD: return a + b;
    case ELT_SUB: return a - b;
    case ELT_MUL: return a * b;
    case ELT_DIV: return a / b;
    case ELT_MAX: return fmaxf(a, b);
    case ELT_MIN: return fminf(a, b);
    case ELT_SQDIFF: { float d = a - b; return d * d; }
    default: return a;
  }
}

__global__ void k_unary(const ushort* __restrict__ x, ushort* __restrict__ y,
                        int64_t n, int fn) {
  int64_t i0 = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TPB;
  // vectorized over 4 bf16 per thread
  int64_t n4 = n / 4;
  for (int64_t i = i0; i < n4; i += stride) {
    short4_t v = reinterpret_cast<const short4_t*>(x)[i];
    short4_t r;
    #pragma unroll
    for (int j = 0; j < 4; ++j)
      r[j] = (short)f2bf(apply_unary(bf2f((ushort)v[j]), fn));
    reinterpret_cast<short4_t*>(y)[i] = r;
  }
  for (int64_t i = n4 * 4 + i0; i < n; i += stride)
    y[i] = f2bf(apply_unary(bf2f(x[i]), fn));
}

__global__ void k_binary_same(const ushort* __restrict__ a,
                              const ushort* __restrict__ b,
                              ushort* __restrict__ y, int64_t n, int fn) {
  int64_t i0 = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TPB;
  int64_t n4 = n / 4;
  for (int64_t i = i0; i < n4; i += stride) {
    short4_t va = reinterpret_cast<const short4_t*>(a)[i];
    short4_t vb = reinterpret_cast<const short4_t*>(b)[i];
    short4_t r;
    #pragma unroll
    for (int j = 0; j < 4; ++j)
      r[j] = (short)f2bf(apply_binary(bf2f((ushort)va[j]),
                                      bf2f((ushort)vb[j]), fn));
    reinterpret_cast<short4_t*>(y)[i] = r;
  }
  for (int64_t i = n4 * 4 + i0; i < n; i += stride)
    y[i] = f2bf(apply_binary(bf2f(a[i]), bf2f(b[i]), fn));
}

__global__ void k_binary_bcast(const ushort* __restrict__ a,
                               const ushort* __restrict__ b,
                               ushort* __restrict__ y, int64_t n,
                               BcastArgs bc, int fn) {
  int64_t i0 = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t i = i0; i < n; i += stride) {
    int64_t rem = i, ia = 0, ib = 0;
    #pragma unroll
    for (int d = MAX_DIMS - 1; d >= 0; --d) {
      if (d >= bc.ndim) continue;
      int64_t c = rem % bc.dims[d];
      rem /= bc.dims[d];
      ia += c * bc.sa[d];
      ib += c * bc.sb[d];
    }
    y[i] = f2bf(apply_binary(bf2f(a[ia]), bf2f(b[ib]), fn));
  }
}

void launch_eltwise_unary(hipStream_t s, const ushort* x, ushort* y,
                          int64_t n, int fn) {
  hipLaunchKernelGGL(k_unary, dim3(grid_for(n, 4)), dim3(TPB), 0, s,
                     x, y, n, fn);
}

void launch_eltwise_binary(hipStream_t s, const ushort* a, const ushort* b,
                           ushort* y, int64_t n_out, const BcastArgs& bc,
                           int fn) {
  bool same = true;
  for (int d = 0; d < bc.ndim; ++d) {
    // contiguous same-shape iff both stride patterns are the canonical
    // contiguous ones (marked by sa/sb equal to out strides; python sets
    // sa=sb=contig in that case and ndim=1)
  }
  if (bc.ndim == 1 && bc.sa[0] == 1 && bc.sb[0] == 1) {
    hipLaunchKernelGGL(k_binary_same, dim3(grid_for(n_out, 4)), dim3(TPB),
                       0, s, a, b, y, n_out, fn);
  } else {
    hipLaunchKernelGGL(k_binary_bcast, dim3(grid_for(n_out)), dim3(TPB),
                       0, s, a, b, y, n_out, bc, fn);
  }
  (void)same;
}

// ---------------------------------------------------------------------------
// fused scale/shift (+act): y = act(x * scale[c] + shift[c]) over [rows, C]
// ---------------------------------------------------------------------------
__global__ void k_bn_act(const ushort* __restrict__ x,
                         const ushort* __restrict__ scale,
                         const ushort* __restrict__ shift,
                         ushort* __restrict__ y, int64_t n, int64_t c,
                         int act) {
  int64_t i0 = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t i = i0; i < n; i += stride) {
    int64_t ch = i % c;
    float v = bf2f(x[i]) * bf2f(scale[ch]) + bf2f(shift[ch]);
    switch (act) {
      case ACT_RELU: v = v > 0.f ? v : 0.f; break;
      case ACT_TANH: v = tanhf(v); break;
      case ACT_SIGMOID: v = 1.f / (1.f + __expf(-v)); break;
      case ACT_GELU: v = 0.5f * v * (1.f + erff(v * 0.70710678f)); break;
      case ACT_RELU6: v = v < 0.f ? 0.f : (v > 6.f ? 6.f : v); break;
    }
    y[i] = f2bf(v);
  }
}

void launch_bn_act(hipStream_t s, const ushort* x, const ushort* scale,
                   const ushort* shift, ushort* y, int64_t rows, int64_t c,
                   int act) {
  int64_t n = rows * c;
  hipLaunchKernelGGL(k_bn_act, dim3(grid_for(n)), dim3(TPB), 0, s,
                     x, scale, shift, y, n, c, act);
}

// ---------------------------------------------------------------------------
// row softmax: one block per row (grid-stride over rows), online max+sum
// ---------------------------------------------------------------------------
template <typename Reduce>
TFSC_DEV float block_reduce(float v, Reduce red, float init) {
  __shared__ float smem[TPB / WAVE];
  #pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1)
    v = red(v, __shfl_down(v, off, WAVE));
  int wid = threadIdx.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) smem[wid] = v;
  __syncthreads();
  v = (threadIdx.x < TPB / WAVE) ? smem[threadIdx.x] : init;
  #pragma unroll
  for (int off = TPB / WAVE / 2; off > 0; off >>= 1)
    v = red(v, __shfl_down(v, off, WAVE));
  v = __shfl(v, 0, WAVE);
  if (threadIdx.x == 0) smem[0] = v;
  __syncthreads();
  v = smem[0];
  __syncthreads();
  return v;
}

struct MaxOp { TFSC_DEV float operator()(float a, float b) const { return fmaxf(a, b); } };
struct SumOp { TFSC_DEV float operator()(float a, float b) const { return a + b; } };

__global__ void k_softmax(const ushort* __restrict__ x,
                          ushort* __restrict__ y, int64_t rows,
                          int64_t cols) {
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const ushort* xr = x + row * cols;
    ushort* yr = y + row * cols;
    float mx = -INFINITY;
    for (int64_t i = threadIdx.x; i < cols; i += TPB)
      mx = fmaxf(mx, bf2f(xr[i]));
    mx = block_reduce(mx, MaxOp(), -INFINITY);
    float sum = 0.f;
    for (int64_t i = threadIdx.x; i < cols; i += TPB)
      sum += __expf(bf2f(xr[i]) - mx);
    sum = block_reduce(sum, SumOp(), 0.f);
    float inv = 1.f / sum;
    for (int64_t i = threadIdx.x; i < cols; i += TPB)
      yr[i] = f2bf(__expf(bf2f(xr[i]) - mx) * inv);
  }
}

// small-row softmax: one WAVE per row, the whole row in registers
// (cols <= 8*VEC*... handled for cols <= 512, 8 bf16 per lane), single
// read of x — the block-per-row kernel re-reads x three times and idles
// (256-cols) threads (attention S=128 rows ran at ~0.85 TB/s before).
template <int VPL>   // values per lane (8 -> cols<=512)
__global__ void k_softmax_wave(const ushort* __restrict__ x,
                               ushort* __restrict__ y, int64_t rows,
                               int cols) {
  int64_t row0 = (int64_t)blockIdx.x * (TPB / WAVE) + threadIdx.x / WAVE;
  int64_t wstride = (int64_t)gridDim.x * (TPB / WAVE);
  int lane = threadIdx.x % WAVE;
  for (int64_t row = row0; row < rows; row += wstride) {
    const ushort* xr = x + row * cols;
    ushort* yr = y + row * cols;
    float v[VPL];
    int n = (cols + WAVE - 1) / WAVE;   // elements this lane handles
    float mx = -INFINITY;
    #pragma unroll
    for (int j = 0; j < VPL; ++j) {
      int i = j * WAVE + lane;
      v[j] = (j < n && i < cols) ? bf2f(xr[i]) : -INFINITY;
      mx = fmaxf(mx, v[j]);
    }
    #pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1)
      mx = fmaxf(mx, __shfl_xor(mx, off, WAVE));
    float sum = 0.f;
    #pragma unroll
    for (int j = 0; j < VPL; ++j) {
      v[j] = __expf(v[j] - mx);
      sum += v[j];
    }
    #pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1)
      sum += __shfl_xor(sum, off, WAVE);
    float inv = 1.f / sum;
    #pragma unroll
    for (int j = 0; j < VPL; ++j) {
      int i = j * WAVE + lane;
      if (j < n && i < cols) yr[i] = f2bf(v[j] * inv);
    }
  }
}

void launch_softmax(hipStream_t s, const ushort* x, ushort* y,
                    int64_t rows, int64_t cols) {
  if (cols <= 512) {
    int64_t wgs = ceil_div(rows, (int64_t)(TPB / WAVE));
    int blocks = int(wgs < MAX_BLOCKS ? (wgs > 0 ? wgs : 1) : MAX_BLOCKS);
    if (cols <= 128)
      hipLaunchKernelGGL(k_softmax_wave<2>, dim3(blocks), dim3(TPB), 0, s,
                         x, y, rows, int(cols));
    else
      hipLaunchKernelGGL(k_softmax_wave<8>, dim3(blocks), dim3(TPB), 0, s,
                         x, y, rows, int(cols));
    return;
  }
  int blocks = int(rows < MAX_BLOCKS ? rows : MAX_BLOCKS);
  hipLaunchKernelGGL(k_softmax, dim3(blocks), dim3(TPB), 0, s,
                     x, y, rows, cols);
}

// ---------------------------------------------------------------------------
// layernorm (last dim): one block per row. Two passes for the statistics:
// the mean, then the mean of squared deviations from it (E[x^2] - mean^2
// cancels in f32 on rows whose mean is large against their spread); the
// second and third reads of the row hit the cache.
// ---------------------------------------------------------------------------
__global__ void k_layernorm(const ushort* __restrict__ x,
                            const ushort* __restrict__ gamma,
                            const ushort* __restrict__ beta,
                            ushort* __restrict__ y, int64_t rows,
                            int64_t cols, float eps) {
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const ushort* xr = x + row * cols;
    ushort* yr = y + row * cols;
    float sum = 0.f;
    for (int64_t i = threadIdx.x; i < cols; i += TPB)
      sum += bf2f(xr[i]);
    float mean = block_reduce(sum, SumOp(), 0.f) / cols;
    float sq = 0.f;
    for (int64_t i = threadIdx.x; i < cols; i += TPB) {
      float d = bf2f(xr[i]) - mean;
      sq += d * d;
    }
    float var = block_reduce(sq, SumOp(), 0.f) / cols;   // >= 0
    float rstd = rsqrtf(var + eps);
    for (int64_t i = threadIdx.x; i < cols; i += TPB) {
      float v = (bf2f(xr[i]) - mean) * rstd;
      yr[i] = f2bf(v * bf2f(gamma[i]) + bf2f(beta[i]));
    }
  }
}

void launch_layernorm(hipStream_t s, const ushort* x, const ushort* gamma,
                      const ushort* beta, ushort* y, int64_t rows,
                      int64_t cols, float eps) {
  int blocks = int(rows < MAX_BLOCKS ? rows : MAX_BLOCKS);
  hipLaunchKernelGGL(k_layernorm, dim3(blocks), dim3(TPB), 0, s,
                     x, gamma, beta, y, rows, cols, eps);
}

// ---------------------------------------------------------------------------
// reductions
// ---------------------------------------------------------------------------
__global__ void k_mean_last(const ushort* __restrict__ x,
                            ushort* __restrict__ y, int64_t rows,
                            int64_t cols) {
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const ushort* xr = x + row * cols;
    float sum = 0.f;
    for (int64_t i = threadIdx.x; i < cols; i += TPB)
      sum += bf2f(xr[i]);
    sum = block_reduce(sum, SumOp(), 0.f);
    if (threadIdx.x == 0) y[row] = f2bf(sum / cols);
  }
}

void launch_reduce_mean_last(hipStream_t s, const ushort* x, ushort* y,
                             int64_t rows, int64_t cols) {
  int blocks = int(rows < MAX_BLOCKS ? rows : MAX_BLOCKS);
  hipLaunchKernelGGL(k_mean_last, dim3(blocks), dim3(TPB), 0, s,
                     x, y, rows, cols);
}

// mean over axis 1 of [d0, d1, d2]: out[d0, d2]. Threads over (d0, d2) —
// coalesced on d2.
__global__ void k_mean_mid(const ushort* __restrict__ x,
                           ushort* __restrict__ y, int64_t d0, int64_t d1,
                           int64_t d2) {
  int64_t n = d0 * d2;
  int64_t i0 = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t i = i0; i < n; i += stride) {
    int64_t o = i / d2, c = i % d2;
    const ushort* xp = x + o * d1 * d2 + c;
    float sum = 0.f;
    for (int64_t j = 0; j < d1; ++j) sum += bf2f(xp[j * d2]);
    y[i] = f2bf(sum / d1);
  }
}

void launch_reduce_mean_mid(hipStream_t s, const ushort* x, ushort* y,
                            int64_t d0, int64_t d1, int64_t d2) {
  hipLaunchKernelGGL(k_mean_mid, dim3(grid_for(d0 * d2)), dim3(TPB), 0, s,
                     x, y, d0, d1, d2);
}

// ---------------------------------------------------------------------------
// pooling (NHWC; one thread per output element, coalesced over C)
// ---------------------------------------------------------------------------
__global__ void k_pool(const ushort* __restrict__ x, ushort* __restrict__ y,
                       bool is_max, int N, int H, int W, int C, int Ho,
                       int Wo, int kh, int kw, int sh, int sw, int pt,
                       int pl) {
  int64_t n_out = (int64_t)N * Ho * Wo * C;
  int64_t i0 = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t i = i0; i < n_out; i += stride) {
    int c = int(i % C);
    int64_t t = i / C;
    int wo = int(t % Wo); t /= Wo;
    int ho = int(t % Ho); int n = int(t / Ho);
    float acc = is_max ? -INFINITY : 0.f;
    int count = 0;
    for (int r = 0; r < kh; ++r) {
      int hi = ho * sh + r - pt;
      if (hi < 0 || hi >= H) continue;
      for (int q = 0; q < kw; ++q) {
        int wi = wo * sw + q - pl;
        if (wi < 0 || wi >= W) continue;
        float v = bf2f(x[(((int64_t)n * H + hi) * W + wi) * C + c]);
        if (is_max) acc = fmaxf(acc, v);
        else acc += v;
        ++count;
      }
    }
    y[i] = f2bf(is_max ? acc : (count ? acc / count : 0.f));
  }
}

// vectorized pool (C % 8 == 0): one thread per (n,ho,wo,c8-group),
// 16-byte loads/stores — 1/8 the index math of the scalar kernel
__global__ void k_pool_v8(const ushort* __restrict__ x,
                          ushort* __restrict__ y, bool is_max, int N,
                          int H, int W, int C, int Ho, int Wo, int kh,
                          int kw, int sh, int sw, int pt, int pl) {
  int c8 = C >> 3;
  int64_t n_grp = (int64_t)N * Ho * Wo * c8;
  int64_t i0 = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t i = i0; i < n_grp; i += stride) {
    int g = int(i % c8);
    int64_t t = i / c8;
    int wo = int(t % Wo); t /= Wo;
    int ho = int(t % Ho); int n = int(t / Ho);
    float acc[8];
    #pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = is_max ? -INFINITY : 0.f;
    int count = 0;
    for (int r = 0; r < kh; ++r) {
      int hi = ho * sh + r - pt;
      if (hi < 0 || hi >= H) continue;
      for (int q = 0; q < kw; ++q) {
        int wi = wo * sw + q - pl;
        if (wi < 0 || wi >= W) continue;
        short4_t lo = *reinterpret_cast<const short4_t*>(
            x + (((int64_t)n * H + hi) * W + wi) * C + g * 8);
        short4_t hi4 = *reinterpret_cast<const short4_t*>(
            x + (((int64_t)n * H + hi) * W + wi) * C + g * 8 + 4);
        #pragma unroll
        for (int j = 0; j < 4; ++j) {
          float a = bf2f((ushort)lo[j]);
          float b = bf2f((ushort)hi4[j]);
          if (is_max) {
            acc[j] = fmaxf(acc[j], a);
            acc[j + 4] = fmaxf(acc[j + 4], b);
          } else {
            acc[j] += a;
            acc[j + 4] += b;
          }
        }
        ++count;
      }
    }
    short4_t out_lo, out_hi;
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
      float a = is_max ? acc[j] : (count ? acc[j] / count : 0.f);
      float b = is_max ? acc[j + 4] : (count ? acc[j + 4] / count : 0.f);
      out_lo[j] = (short)f2bf(a);
      out_hi[j] = (short)f2bf(b);
    }
    ushort* dst = y + i * 8;
    *reinterpret_cast<short4_t*>(dst) = out_lo;
    *reinterpret_cast<short4_t*>(dst + 4) = out_hi;
  }
}

void launch_pool(hipStream_t s, const ushort* x, ushort* y, bool is_max,
                 int N, int H, int W, int C, int Ho, int Wo, int kh, int kw,
                 int sh, int sw, int pt, int pl) {
  if (C % 8 == 0) {
    int64_t n_grp = (int64_t)N * Ho * Wo * (C / 8);
    hipLaunchKernelGGL(k_pool_v8, dim3(grid_for(n_grp)), dim3(TPB), 0, s,
                       x, y, is_max, N, H, W, C, Ho, Wo, kh, kw, sh, sw,
                       pt, pl);
    return;
  }
  int64_t n_out = (int64_t)N * Ho * Wo * C;
  hipLaunchKernelGGL(k_pool, dim3(grid_for(n_out)), dim3(TPB), 0, s,
                     x, y, is_max, N, H, W, C, Ho, Wo, kh, kw, sh, sw,
                     pt, pl);
}

// ---------------------------------------------------------------------------
// transpose / gather / pad
// ---------------------------------------------------------------------------
struct TransArgs {
  int ndim;
  int64_t out_dims[MAX_DIMS];
  int64_t in_strides[MAX_DIMS];   // input element stride per OUTPUT dim
};

__global__ void k_transpose(const ushort* __restrict__ x,
                            ushort* __restrict__ y, TransArgs ta,
                            int64_t n) {
  int64_t i0 = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t i = i0; i < n; i += stride) {
    int64_t rem = i, src = 0;
    #pragma unroll
    for (int d = MAX_DIMS - 1; d >= 0; --d) {
      if (d >= ta.ndim) continue;
      int64_t c = rem % ta.out_dims[d];
      rem /= ta.out_dims[d];
      src += c * ta.in_strides[d];
    }
    y[i] = x[src];
  }
}

// fast path: the permutation keeps the LAST dim innermost (e.g. the
// attention head split/merge perm [0,2,1,3]) and it is a multiple of 8
// bf16 — move 16-byte chunks instead of scalars. transpose_takes_v8
// (transpose_gate.h) decides; it also looks at the pointers and the outer
// strides, since strided_copy comes through here with an offset source.
__global__ void k_transpose_v8(const ushort* __restrict__ x,
                               ushort* __restrict__ y, TransArgs ta,
                               int64_t n_grp, int last) {
  int grp_per_row = last >> 3;
  int64_t i0 = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t i = i0; i < n_grp; i += stride) {
    int g = int(i % grp_per_row);
    int64_t rem = i / grp_per_row;        // linear index over outer dims
    int64_t src = 0;
    #pragma unroll
    for (int d = MAX_DIMS - 1; d >= 0; --d) {
      if (d >= ta.ndim - 1) continue;     // skip last dim
      int64_t c = rem % ta.out_dims[d];
      rem /= ta.out_dims[d];
      src += c * ta.in_strides[d];
    }
    *reinterpret_cast<uint4*>(y + i * 8) =
        *reinterpret_cast<const uint4*>(x + src + g * 8);
  }
}

void launch_transpose(hipStream_t s, const ushort* x, ushort* y, int ndim,
                      const int64_t* out_dims, const int64_t* in_strides,
                      int64_t n_out) {
  TransArgs ta;
  ta.ndim = ndim;
  for (int d = 0; d < MAX_DIMS; ++d) {
    ta.out_dims[d] = d < ndim ? out_dims[d] : 1;
    ta.in_strides[d] = d < ndim ? in_strides[d] : 0;
  }
  int last = ndim > 0 ? int(out_dims[ndim - 1]) : 0;
  if (transpose_takes_v8(x, y, ndim, out_dims, in_strides)) {
    int64_t n_grp = n_out / 8;
    hipLaunchKernelGGL(k_transpose_v8, dim3(grid_for(n_grp)), dim3(TPB),
                       0, s, x, y, ta, n_grp, last);
    return;
  }
  hipLaunchKernelGGL(k_transpose, dim3(grid_for(n_out)), dim3(TPB), 0, s,
                     x, y, ta, n_out);
}

__global__ void k_gather_rows(const ushort* __restrict__ table,
                              const int* __restrict__ idx,
                              ushort* __restrict__ y, int64_t n_idx,
                              int64_t row) {
  int64_t n = n_idx * row;
  int64_t i0 = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t i = i0; i < n; i += stride) {
    int64_t r = i / row, c = i % row;
    y[i] = table[(int64_t)idx[r] * row + c];
  }
}

void launch_gather_rows(hipStream_t s, const ushort* table, const int* idx,
                        ushort* y, int64_t n_idx, int64_t row_elems) {
  hipLaunchKernelGGL(k_gather_rows, dim3(grid_for(n_idx * row_elems)),
                     dim3(TPB), 0, s, table, idx, y, n_idx, row_elems);
}

// dtype casts for the C++ fast predict path (f32 staging <-> bf16
// workspace; conversion on-GPU instead of host-side)
__global__ void k_f32_to_bf16(const float* __restrict__ x,
                              ushort* __restrict__ y, int64_t n) {
  int64_t i0 = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TPB;
  int64_t n4 = n / 4;
  for (int64_t i = i0; i < n4; i += stride) {
    float4 v = reinterpret_cast<const float4*>(x)[i];
    short4_t r;
    r[0] = (short)f2bf(v.x); r[1] = (short)f2bf(v.y);
    r[2] = (short)f2bf(v.z); r[3] = (short)f2bf(v.w);
    reinterpret_cast<short4_t*>(y)[i] = r;
  }
  for (int64_t i = n4 * 4 + i0; i < n; i += stride)
    y[i] = f2bf(x[i]);
}

__global__ void k_bf16_to_f32(const ushort* __restrict__ x,
                              float* __restrict__ y, int64_t n) {
  int64_t i0 = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TPB;
  int64_t n4 = n / 4;
  for (int64_t i = i0; i < n4; i += stride) {
    short4_t v = reinterpret_cast<const short4_t*>(x)[i];
    float4 r;
    r.x = bf2f((ushort)v[0]); r.y = bf2f((ushort)v[1]);
    r.z = bf2f((ushort)v[2]); r.w = bf2f((ushort)v[3]);
    reinterpret_cast<float4*>(y)[i] = r;
  }
  for (int64_t i = n4 * 4 + i0; i < n; i += stride)
    y[i] = bf2f(x[i]);
}

void launch_f32_to_bf16(hipStream_t s, const float* x, ushort* y,
                        int64_t n) {
  hipLaunchKernelGGL(k_f32_to_bf16, dim3(grid_for(n, 4)), dim3(TPB), 0, s,
                     x, y, n);
}

void launch_bf16_to_f32(hipStream_t s, const ushort* x, float* y,
                        int64_t n) {
  hipLaunchKernelGGL(k_bf16_to_f32, dim3(grid_for(n, 4)), dim3(TPB), 0, s,
                     x, y, n);
}

// widen the channel dim with zeros: [rows, c_in] -> [rows, c_out]
// (used to lift C%8!=0 conv inputs — e.g. RGB stems — onto the fused
// implicit-GEMM path)
__global__ void k_pad_last(const ushort* __restrict__ x,
                           ushort* __restrict__ y, int64_t rows, int c_in,
                           int c_out) {
  int64_t n = rows * c_out;
  int64_t i0 = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t i = i0; i < n; i += stride) {
    int c = int(i % c_out);
    int64_t r = i / c_out;
    y[i] = c < c_in ? x[r * c_in + c] : ushort(0);
  }
}

void launch_pad_last(hipStream_t s, const ushort* x, ushort* y,
                     int64_t rows, int c_in, int c_out) {
  hipLaunchKernelGGL(k_pad_last, dim3(grid_for(rows * c_out)), dim3(TPB),
                     0, s, x, y, rows, c_in, c_out);
}

__global__ void k_pad_nhwc(const ushort* __restrict__ x,
                           ushort* __restrict__ y, int N, int H, int W,
                           int C, int pt, int pl, int Ho, int Wo) {
  int64_t n_out = (int64_t)N * Ho * Wo * C;
  int64_t i0 = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t i = i0; i < n_out; i += stride) {
    int c = int(i % C);
    int64_t t = i / C;
    int wo = int(t % Wo); t /= Wo;
    int ho = int(t % Ho); int n = int(t / Ho);
    int hi = ho - pt, wi = wo - pl;
    ushort v = 0;
    if (hi >= 0 && hi < H && wi >= 0 && wi < W)
      v = x[(((int64_t)n * H + hi) * W + wi) * C + c];
    y[i] = v;
  }
}

void launch_pad_nhwc(hipStream_t s, const ushort* x, ushort* y,
                     int N, int H, int W, int C, int pt, int pb, int pl,
                     int pr) {
  int Ho = H + pt + pb, Wo = W + pl + pr;
  int64_t n_out = (int64_t)N * Ho * Wo * C;
  hipLaunchKernelGGL(k_pad_nhwc, dim3(grid_for(n_out)), dim3(TPB), 0, s,
                     x, y, N, H, W, C, pt, pl, Ho, Wo);
}

// ---------------------------------------------------------------------------
// depthwise NHWC conv: per-channel R x S taps,
// memory-bound — channels are contiguous in NHWC so the channel dim is
// the vector dim (4x bf16). w is [R,S,C] flat; per-tap weight loads hit
// L2 (w is tiny and every pixel of the image reuses it). These two
// kernels are depth_multiplier == 1; the multiplier kernels follow them.
// ---------------------------------------------------------------------------
TFSC_DEV float dw_act(float v, int act) {
  switch (act) {
    case ACT_RELU: return v > 0.f ? v : 0.f;
    case ACT_TANH: return tanhf(v);
    case ACT_SIGMOID: return 1.f / (1.f + __expf(-v));
    case ACT_GELU: return 0.5f * v * (1.f + erff(v * 0.70710678f));
    case ACT_RELU6: return v < 0.f ? 0.f : (v > 6.f ? 6.f : v);
    default: return v;
  }
}

__global__ void k_depthwise_v4(const ushort* __restrict__ x,
                               const ushort* __restrict__ w,
                               const ushort* __restrict__ bias,
                               ushort* __restrict__ y,
                               int N, int H, int W, int C, int R, int S,
                               int sh, int sw, int pt, int pl,
                               int Ho, int Wo, int act) {
  int c4 = C / 4;
  int64_t total = (int64_t)N * Ho * Wo * c4;
  int64_t i0 = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t i = i0; i < total; i += stride) {
    int64_t t = i;
    int cv = int(t % c4); t /= c4;
    int wo = int(t % Wo); t /= Wo;
    int ho = int(t % Ho); int n = int(t / Ho);
    int c = cv * 4;
    float acc[4];
    short4_t bv = reinterpret_cast<const short4_t*>(bias)[cv];
    #pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = bf2f((ushort)bv[j]);
    int hi0 = ho * sh - pt, wi0 = wo * sw - pl;
    for (int r = 0; r < R; ++r) {
      int hi = hi0 + r;
      if (hi < 0 || hi >= H) continue;
      for (int sx = 0; sx < S; ++sx) {
        int wi = wi0 + sx;
        if (wi < 0 || wi >= W) continue;
        short4_t xv = reinterpret_cast<const short4_t*>(
            x + ((((int64_t)n * H + hi) * W + wi) * C))[cv];
        short4_t wv = reinterpret_cast<const short4_t*>(
            w + ((r * S + sx) * C))[cv];
        #pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[j] += bf2f((ushort)xv[j]) * bf2f((ushort)wv[j]);
      }
    }
    short4_t out;
    #pragma unroll
    for (int j = 0; j < 4; ++j)
      out[j] = (short)f2bf(dw_act(acc[j], act));
    reinterpret_cast<short4_t*>(
        y + ((((int64_t)n * Ho + ho) * Wo + wo) * C))[cv] = out;
  }
}

__global__ void k_depthwise_scalar(const ushort* __restrict__ x,
                                   const ushort* __restrict__ w,
                                   const ushort* __restrict__ bias,
                                   ushort* __restrict__ y,
                                   int N, int H, int W, int C, int R, int S,
                                   int sh, int sw, int pt, int pl,
                                   int Ho, int Wo, int act) {
  int64_t total = (int64_t)N * Ho * Wo * C;
  int64_t i0 = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t i = i0; i < total; i += stride) {
    int64_t t = i;
    int c = int(t % C); t /= C;
    int wo = int(t % Wo); t /= Wo;
    int ho = int(t % Ho); int n = int(t / Ho);
    float acc = bf2f(bias[c]);
    int hi0 = ho * sh - pt, wi0 = wo * sw - pl;
    for (int r = 0; r < R; ++r) {
      int hi = hi0 + r;
      if (hi < 0 || hi >= H) continue;
      for (int sx = 0; sx < S; ++sx) {
        int wi = wi0 + sx;
        if (wi < 0 || wi >= W) continue;
        acc += bf2f(x[(((int64_t)n * H + hi) * W + wi) * C + c]) *
               bf2f(w[(r * S + sx) * C + c]);
      }
    }
    y[i] = f2bf(dw_act(acc, act));
  }
}

// Depth multiplier M > 1: output channel k = c*M + m reads input channel
// c = k / M; w [R,S,C*M], bias [C*M] and y [N,Ho,Wo,C*M] are contiguous
// in k (the TF [R,S,C,M] filter read flat). Still memory-bound: k is
// the vector dim, 8 bf16 = 16 bytes of w, bias and y per thread.
//
// XC = 8/M input channels feed one thread's 8 outputs: 4 (M = 2, one
// 8-byte x load per tap), 2 (M = 4, one 4-byte load) or 1 (M % 8 == 0,
// one bf16 shared by all 8). The launcher only comes here when
// (C*M) % 8 == 0 and M is 2, 4 or a multiple of 8, and that is what
// aligns the x loads: a pixel's row of C elements starts at a multiple
// of 8 bytes when C % 4 == 0 (M = 2) and of 4 bytes when C % 2 == 0
// (M = 4), and the thread's first channel kv*XC sits XC*2 bytes further
// per vector; for M % 8 == 0 the 8 outputs kv*8.. lie inside one block
// of M and share the single channel kv*8 / M.
template <int XC>
__global__ void k_depthwise_mult_v8(const ushort* __restrict__ x,
                                    const ushort* __restrict__ w,
                                    const ushort* __restrict__ bias,
                                    ushort* __restrict__ y,
                                    int N, int H, int W, int C, int M,
                                    int R, int S, int sh, int sw, int pt,
                                    int pl, int Ho, int Wo, int act) {
  int K = C * M;
  int k8 = K / 8;
  int64_t total = (int64_t)N * Ho * Wo * k8;
  int64_t i0 = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t i = i0; i < total; i += stride) {
    int64_t t = i;
    int kv = int(t % k8); t /= k8;
    int wo = int(t % Wo); t /= Wo;
    int ho = int(t % Ho); int n = int(t / Ho);
    int c0 = XC == 1 ? (kv * 8) / M : kv * XC;
    float acc[8];
    short8_t bv = reinterpret_cast<const short8_t*>(bias)[kv];
    #pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = bf2f((ushort)bv[j]);
    int hi0 = ho * sh - pt, wi0 = wo * sw - pl;
    for (int r = 0; r < R; ++r) {
      int hi = hi0 + r;
      if (hi < 0 || hi >= H) continue;
      for (int sx = 0; sx < S; ++sx) {
        int wi = wi0 + sx;
        if (wi < 0 || wi >= W) continue;
        const ushort* xp = x + ((((int64_t)n * H + hi) * W + wi) * C + c0);
        float xf[XC];
        if constexpr (XC == 4) {
          short4_t xv = *reinterpret_cast<const short4_t*>(xp);
          #pragma unroll
          for (int j = 0; j < 4; ++j) xf[j] = bf2f((ushort)xv[j]);
        } else if constexpr (XC == 2) {
          uint32_t xv = *reinterpret_cast<const uint32_t*>(xp);
          xf[0] = bf2f((ushort)(xv & 0xffffu));
          xf[1] = bf2f((ushort)(xv >> 16));
        } else {
          xf[0] = bf2f(*xp);
        }
        short8_t wv = reinterpret_cast<const short8_t*>(
            w + ((int64_t)(r * S + sx) * K))[kv];
        #pragma unroll
        for (int j = 0; j < 8; ++j)
          acc[j] += xf[j / (8 / XC)] * bf2f((ushort)wv[j]);
      }
    }
    short8_t out;
    #pragma unroll
    for (int j = 0; j < 8; ++j)
      out[j] = (short)f2bf(dw_act(acc[j], act));
    reinterpret_cast<short8_t*>(
        y + ((((int64_t)n * Ho + ho) * Wo + wo) * K))[kv] = out;
  }
}

// every other (C, M): one thread per output element
__global__ void k_depthwise_mult_scalar(const ushort* __restrict__ x,
                                        const ushort* __restrict__ w,
                                        const ushort* __restrict__ bias,
                                        ushort* __restrict__ y,
                                        int N, int H, int W, int C, int M,
                                        int R, int S, int sh, int sw,
                                        int pt, int pl, int Ho, int Wo,
                                        int act) {
  int K = C * M;
  int64_t total = (int64_t)N * Ho * Wo * K;
  int64_t i0 = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t i = i0; i < total; i += stride) {
    int64_t t = i;
    int k = int(t % K); t /= K;
    int wo = int(t % Wo); t /= Wo;
    int ho = int(t % Ho); int n = int(t / Ho);
    int c = k / M;
    float acc = bf2f(bias[k]);
    int hi0 = ho * sh - pt, wi0 = wo * sw - pl;
    for (int r = 0; r < R; ++r) {
      int hi = hi0 + r;
      if (hi < 0 || hi >= H) continue;
      for (int sx = 0; sx < S; ++sx) {
        int wi = wi0 + sx;
        if (wi < 0 || wi >= W) continue;
        acc += bf2f(x[(((int64_t)n * H + hi) * W + wi) * C + c]) *
               bf2f(w[(int64_t)(r * S + sx) * K + k]);
      }
    }
    y[i] = f2bf(dw_act(acc, act));
  }
}

void launch_depthwise_conv(hipStream_t s, const ushort* x, const ushort* w,
                           const ushort* bias, ushort* y,
                           int N, int H, int W, int C, int R, int S,
                           int sh, int sw, int pt, int pl, int Ho, int Wo,
                           int act, int mult) {
  if (mult < 1)
    throw std::runtime_error("depthwise conv: depth multiplier " +
                             std::to_string(mult) + " < 1");
  if (mult > 1) {
    int64_t K = (int64_t)C * mult;
    bool vec = K % 8 == 0 && (mult == 2 || mult == 4 || mult % 8 == 0);
    if (!vec) {
      hipLaunchKernelGGL(k_depthwise_mult_scalar,
                         dim3(grid_for((int64_t)N * Ho * Wo * K)),
                         dim3(TPB), 0, s, x, w, bias, y, N, H, W, C, mult,
                         R, S, sh, sw, pt, pl, Ho, Wo, act);
      return;
    }
    dim3 grid(grid_for((int64_t)N * Ho * Wo * (K / 8)));
    if (mult == 2)
      hipLaunchKernelGGL(k_depthwise_mult_v8<4>, grid, dim3(TPB), 0, s, x,
                         w, bias, y, N, H, W, C, mult, R, S, sh, sw, pt,
                         pl, Ho, Wo, act);
    else if (mult == 4)
      hipLaunchKernelGGL(k_depthwise_mult_v8<2>, grid, dim3(TPB), 0, s, x,
                         w, bias, y, N, H, W, C, mult, R, S, sh, sw, pt,
                         pl, Ho, Wo, act);
    else
      hipLaunchKernelGGL(k_depthwise_mult_v8<1>, grid, dim3(TPB), 0, s, x,
                         w, bias, y, N, H, W, C, mult, R, S, sh, sw, pt,
                         pl, Ho, Wo, act);
    return;
  }
  if (C % 4 == 0) {
    int64_t total = (int64_t)N * Ho * Wo * (C / 4);
    hipLaunchKernelGGL(k_depthwise_v4, dim3(grid_for(total)), dim3(TPB),
                       0, s, x, w, bias, y, N, H, W, C, R, S, sh, sw,
                       pt, pl, Ho, Wo, act);
  } else {
    int64_t total = (int64_t)N * Ho * Wo * C;
    hipLaunchKernelGGL(k_depthwise_scalar, dim3(grid_for(total)),
                       dim3(TPB), 0, s, x, w, bias, y, N, H, W, C, R, S,
                       sh, sw, pt, pl, Ho, Wo, act);
  }
}

// ---------------------------------------------------------------------------
// scatter (linear src -> strided dst): the concat building block; the
// exact inverse of k_transpose's gather
// ---------------------------------------------------------------------------
__global__ void k_scatter(const ushort* __restrict__ x,
                          ushort* __restrict__ y, TransArgs ta,
                          int64_t n) {
  int64_t i0 = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t i = i0; i < n; i += stride) {
    int64_t rem = i, dst = 0;
    #pragma unroll
    for (int d = MAX_DIMS - 1; d >= 0; --d) {
      if (d >= ta.ndim) continue;
      int64_t c = rem % ta.out_dims[d];     // here: INPUT dims
      rem /= ta.out_dims[d];
      dst += c * ta.in_strides[d];          // here: OUTPUT strides
    }
    y[dst] = x[i];
  }
}

void launch_scatter(hipStream_t s, const ushort* x, ushort* y, int ndim,
                    const int64_t* in_dims, const int64_t* out_strides,
                    int64_t n_in) {
  TransArgs ta;
  ta.ndim = ndim;
  for (int d = 0; d < MAX_DIMS; ++d) {
    ta.out_dims[d] = d < ndim ? in_dims[d] : 1;
    ta.in_strides[d] = d < ndim ? out_strides[d] : 0;
  }
  hipLaunchKernelGGL(k_scatter, dim3(grid_for(n_in)), dim3(TPB), 0, s,
                     x, y, ta, n_in);
}

// ---------------------------------------------------------------------------
// dtype casts + rowwise argmax (classification heads / index ops)
// ---------------------------------------------------------------------------
__global__ void k_cast_i2f(const int* __restrict__ x,
                           ushort* __restrict__ y, int64_t n) {
  int64_t i0 = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t i = i0; i < n; i += stride)
    y[i] = f2bf(float(x[i]));
}

__global__ void k_cast_f2i(const ushort* __restrict__ x,
                           int* __restrict__ y, int64_t n) {
  int64_t i0 = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t i = i0; i < n; i += stride)
    y[i] = int(bf2f(x[i]));      // trunc toward zero (TF Cast)
}

void launch_cast(hipStream_t s, const void* x, void* y, int64_t n,
                 int mode) {
  if (mode == 0)
    hipLaunchKernelGGL(k_cast_i2f, dim3(grid_for(n)), dim3(TPB), 0, s,
                       reinterpret_cast<const int*>(x),
                       reinterpret_cast<ushort*>(y), n);
  else
    hipLaunchKernelGGL(k_cast_f2i, dim3(grid_for(n)), dim3(TPB), 0, s,
                       reinterpret_cast<const ushort*>(x),
                       reinterpret_cast<int*>(y), n);
}

// one wave per row; first-max-wins: strict > within a lane, (value, lower
// index) across lanes
__global__ __launch_bounds__(256)
void k_argmax_last(const ushort* __restrict__ x, int* __restrict__ y,
                   int64_t rows, int64_t cols) {
  int wv = threadIdx.x / WAVE;
  int lane = threadIdx.x % WAVE;
  int64_t waves_total = (int64_t)gridDim.x * (256 / WAVE);
  for (int64_t row = (int64_t)blockIdx.x * (256 / WAVE) + wv;
       row < rows; row += waves_total) {
    const ushort* xr = x + row * cols;
    // seeded with (-inf, 0): a row with nothing above -inf answers 0,
    // as TF does, and a lane past the row's end loses every comparison
    // against a real element except an equal -inf, where 0 is right
    float best = -INFINITY;
    int besti = 0;
    for (int64_t i = lane; i < cols; i += WAVE) {
      float v = bf2f(xr[i]);
      if (v > best) {              // i ascends within a lane: first wins
        best = v;
        besti = int(i);
      }
    }
    #pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) {
      float ov = __shfl_xor(best, off, WAVE);
      int oi = __shfl_xor(besti, off, WAVE);
      if (ov > best || (ov == best && oi < besti)) {
        best = ov;
        besti = oi;
      }
    }
    if (lane == 0) y[row] = besti;
  }
}

void launch_argmax_last(hipStream_t s, const ushort* x, int* y,
                        int64_t rows, int64_t cols) {
  int64_t waves = rows;
  int blocks = int(ceil_div(waves, (int64_t)(256 / WAVE)));
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_argmax_last, dim3(blocks), dim3(256), 0, s, x, y,
                     rows, cols);
}

// ---------------------------------------------------------------------------
// image resize (NHWC; TF ResizeNearestNeighbor / ResizeBilinear) and
// zero-insertion (the input dilation of a transposed conv). Same design
// as pooling: one thread per 8 channels of one output pixel with 16-byte
// loads/stores when C % 8 == 0, one thread per element otherwise.
// Source coordinates are f32 and use the unfused *_rn forms so they
// round exactly like the CPU executor's (no fma contraction); every
// source index is clamped into the image.
// ---------------------------------------------------------------------------
struct ResizeGeom {
  int N, H, W, C, Ho, Wo;
  int align, half;        // align_corners / half_pixel_centers (0|1)
  float hscale, wscale;   // computed on the host in f32
};

TFSC_DEV int resize_nearest_idx(int d, float scale, int n_in, int align,
                                int half) {
  float src = half ? __fmul_rn(float(d) + 0.5f, scale)
                   : __fmul_rn(float(d), scale);
  int i = int(align ? roundf(src) : floorf(src));
  return min(max(i, 0), n_in - 1);
}

TFSC_DEV void resize_bilinear_coord(int d, float scale, int n_in, int half,
                                    int& lo, int& hi, float& lerp) {
  float src = half ? __fsub_rn(__fmul_rn(float(d) + 0.5f, scale), 0.5f)
                   : __fmul_rn(float(d), scale);
  float fl = floorf(src);
  lo = min(max(int(fl), 0), n_in - 1);
  hi = min(max(int(ceilf(src)), 0), n_in - 1);
  lerp = src - fl;
}

TFSC_DEV float resize_lerp2(float tl, float tr, float bl, float br,
                            float lx, float ly) {
  float top = tl + (tr - tl) * lx;
  float bot = bl + (br - bl) * lx;
  return top + (bot - top) * ly;
}

// low / high bf16 of a packed 32-bit word as f32
TFSC_DEV float bf_lo(uint32_t u) { return __uint_as_float(u << 16); }
TFSC_DEV float bf_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }

TFSC_DEV uint32_t resize_lerp_pair(uint32_t tl, uint32_t tr, uint32_t bl,
                                   uint32_t br, float lx, float ly) {
  return f2bf2(
      resize_lerp2(bf_lo(tl), bf_lo(tr), bf_lo(bl), bf_lo(br), lx, ly),
      resize_lerp2(bf_hi(tl), bf_hi(tr), bf_hi(bl), bf_hi(br), lx, ly));
}

template <bool BILINEAR>
__global__ void k_resize_v8(const ushort* __restrict__ x,
                            ushort* __restrict__ y, ResizeGeom g) {
  int c8 = g.C >> 3;
  int64_t n_grp = (int64_t)g.N * g.Ho * g.Wo * c8;
  int64_t i0 = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t i = i0; i < n_grp; i += stride) {
    int grp = int(i % c8);
    int64_t t = i / c8;
    int wo = int(t % g.Wo); t /= g.Wo;
    int ho = int(t % g.Ho); int n = int(t / g.Ho);
    const ushort* img = x + (int64_t)n * g.H * g.W * g.C + grp * 8;
    auto px = [&](int hi, int wi) {
      return *reinterpret_cast<const uint4*>(
          img + ((int64_t)hi * g.W + wi) * g.C);
    };
    uint4 out;
    if (BILINEAR) {
      int y0, y1, x0, x1;
      float ly, lx;
      resize_bilinear_coord(ho, g.hscale, g.H, g.half, y0, y1, ly);
      resize_bilinear_coord(wo, g.wscale, g.W, g.half, x0, x1, lx);
      uint4 tl = px(y0, x0), tr = px(y0, x1);
      uint4 bl = px(y1, x0), br = px(y1, x1);
      out.x = resize_lerp_pair(tl.x, tr.x, bl.x, br.x, lx, ly);
      out.y = resize_lerp_pair(tl.y, tr.y, bl.y, br.y, lx, ly);
      out.z = resize_lerp_pair(tl.z, tr.z, bl.z, br.z, lx, ly);
      out.w = resize_lerp_pair(tl.w, tr.w, bl.w, br.w, lx, ly);
    } else {
      out = px(resize_nearest_idx(ho, g.hscale, g.H, g.align, g.half),
               resize_nearest_idx(wo, g.wscale, g.W, g.align, g.half));
    }
    *reinterpret_cast<uint4*>(y + i * 8) = out;
  }
}

template <bool BILINEAR>
__global__ void k_resize(const ushort* __restrict__ x,
                         ushort* __restrict__ y, ResizeGeom g) {
  int64_t n_out = (int64_t)g.N * g.Ho * g.Wo * g.C;
  int64_t i0 = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t i = i0; i < n_out; i += stride) {
    int c = int(i % g.C);
    int64_t t = i / g.C;
    int wo = int(t % g.Wo); t /= g.Wo;
    int ho = int(t % g.Ho); int n = int(t / g.Ho);
    const ushort* img = x + (int64_t)n * g.H * g.W * g.C + c;
    auto px = [&](int hi, int wi) {
      return img[((int64_t)hi * g.W + wi) * g.C];
    };
    if (BILINEAR) {
      int y0, y1, x0, x1;
      float ly, lx;
      resize_bilinear_coord(ho, g.hscale, g.H, g.half, y0, y1, ly);
      resize_bilinear_coord(wo, g.wscale, g.W, g.half, x0, x1, lx);
      y[i] = f2bf(resize_lerp2(bf2f(px(y0, x0)), bf2f(px(y0, x1)),
                               bf2f(px(y1, x0)), bf2f(px(y1, x1)),
                               lx, ly));
    } else {
      y[i] = px(resize_nearest_idx(ho, g.hscale, g.H, g.align, g.half),
                resize_nearest_idx(wo, g.wscale, g.W, g.align, g.half));
    }
  }
}

static inline bool aligned16(const void* a, const void* b) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) &
          15u) == 0;
}

static inline float resize_scale(int n_in, int n_out, bool align_corners) {
  return (align_corners && n_out > 1)
             ? float(n_in - 1) / float(n_out - 1)
             : float(n_in) / float(n_out);
}

void launch_resize_nhwc(hipStream_t s, const ushort* x, ushort* y, int N,
                        int H, int W, int C, int Ho, int Wo, int mode,
                        bool align_corners, bool half_pixel_centers) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || Ho <= 0 || Wo <= 0)
    throw std::runtime_error("resize: every dimension must be positive");
  if (mode != 0 && mode != 1)
    throw std::runtime_error("resize: mode must be 0 (nearest) or 1 "
                             "(bilinear), got " + std::to_string(mode));
  if (align_corners && half_pixel_centers)
    throw std::runtime_error("resize: align_corners and "
                             "half_pixel_centers are mutually exclusive");
  ResizeGeom g{N, H, W, C, Ho, Wo, align_corners ? 1 : 0,
               half_pixel_centers ? 1 : 0,
               resize_scale(H, Ho, align_corners),
               resize_scale(W, Wo, align_corners)};
  if (C % 8 == 0 && aligned16(x, y)) {
    int64_t n_grp = (int64_t)N * Ho * Wo * (C / 8);
    if (mode == 1)
      hipLaunchKernelGGL(k_resize_v8<true>, dim3(grid_for(n_grp)),
                         dim3(TPB), 0, s, x, y, g);
    else
      hipLaunchKernelGGL(k_resize_v8<false>, dim3(grid_for(n_grp)),
                         dim3(TPB), 0, s, x, y, g);
    return;
  }
  int64_t n_out = (int64_t)N * Ho * Wo * C;
  if (mode == 1)
    hipLaunchKernelGGL(k_resize<true>, dim3(grid_for(n_out)), dim3(TPB), 0,
                       s, x, y, g);
  else
    hipLaunchKernelGGL(k_resize<false>, dim3(grid_for(n_out)), dim3(TPB), 0,
                       s, x, y, g);
}

// zero-insert: x [N,h,w,C] -> y [N,(h-1)*sh+1,(w-1)*sw+1,C] with x at the
// (sh, sw)-strided positions. EVERY output element is written (data or
// zero) in the one pass: y lives in the liveness-reused workspace arena,
// so it holds another tensor's bytes when the kernel starts.
__global__ void k_zero_insert_v8(const ushort* __restrict__ x,
                                 ushort* __restrict__ y, int N, int h,
                                 int w, int C, int sh, int sw, int Ho,
                                 int Wo) {
  int c8 = C >> 3;
  int64_t n_grp = (int64_t)N * Ho * Wo * c8;
  int64_t i0 = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t i = i0; i < n_grp; i += stride) {
    int grp = int(i % c8);
    int64_t t = i / c8;
    int wo = int(t % Wo); t /= Wo;
    int ho = int(t % Ho); int n = int(t / Ho);
    uint4 v = uint4{0, 0, 0, 0};
    if (ho % sh == 0 && wo % sw == 0)
      v = *reinterpret_cast<const uint4*>(
          x + (((int64_t)n * h + ho / sh) * w + wo / sw) * C + grp * 8);
    *reinterpret_cast<uint4*>(y + i * 8) = v;
  }
}

__global__ void k_zero_insert(const ushort* __restrict__ x,
                              ushort* __restrict__ y, int N, int h, int w,
                              int C, int sh, int sw, int Ho, int Wo) {
  int64_t n_out = (int64_t)N * Ho * Wo * C;
  int64_t i0 = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t i = i0; i < n_out; i += stride) {
    int c = int(i % C);
    int64_t t = i / C;
    int wo = int(t % Wo); t /= Wo;
    int ho = int(t % Ho); int n = int(t / Ho);
    ushort v = 0;
    if (ho % sh == 0 && wo % sw == 0)
      v = x[(((int64_t)n * h + ho / sh) * w + wo / sw) * C + c];
    y[i] = v;
  }
}

void launch_zero_insert_nhwc(hipStream_t s, const ushort* x, ushort* y,
                             int N, int h, int w, int C, int sh, int sw) {
  if (N <= 0 || h <= 0 || w <= 0 || C <= 0 || sh <= 0 || sw <= 0)
    throw std::runtime_error(
        "zero_insert: every dimension and stride must be positive");
  int64_t Ho64 = (int64_t)(h - 1) * sh + 1, Wo64 = (int64_t)(w - 1) * sw + 1;
  if (Ho64 > INT32_MAX || Wo64 > INT32_MAX)
    throw std::runtime_error("zero_insert: output image too large");
  int Ho = int(Ho64), Wo = int(Wo64);
  if (C % 8 == 0 && aligned16(x, y)) {
    int64_t n_grp = (int64_t)N * Ho * Wo * (C / 8);
    hipLaunchKernelGGL(k_zero_insert_v8, dim3(grid_for(n_grp)), dim3(TPB),
                       0, s, x, y, N, h, w, C, sh, sw, Ho, Wo);
    return;
  }
  int64_t n_out = (int64_t)N * Ho * Wo * C;
  hipLaunchKernelGGL(k_zero_insert, dim3(grid_for(n_out)), dim3(TPB), 0, s,
                     x, y, N, h, w, C, sh, sw, Ho, Wo);
}

}  // namespace tfsc
