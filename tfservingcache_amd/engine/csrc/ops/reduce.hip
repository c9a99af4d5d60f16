// Reductions (TF Sum / Max / Min / Prod / Mean) over one run of axes of a
// bf16 tensor seen as [outer, red, inner]; f32 accumulation, one rounding.
//
//   inner == 1   k_reduce_rows_wave   short rows: one wave per row, four
//                                     rows per workgroup, no LDS
//                k_reduce_rows_block  long rows: one 256-thread workgroup
//                                     per (row, segment)
//   inner  > 1   k_reduce_cols        a workgroup is TX lanes along inner
//                                     by TY = 256 / TX slices along red
//
// A reduced axis split into P segments (the emitter picks P, see
// emit.reduce_segments) writes one f32 partial per (output, segment) to
// scratch[out * P + seg]; a second launch of the row kernels, instantiated
// on f32 input, reduces the P partials and rounds once. Mean is a sum
// until that last step, which divides once.
//
// Data movement of the row kernels: a row (or segment) is addressed in a
// frame that starts at the 16-byte boundary at or below its first
// element, so every vector is one aligned 16-byte load; the first and
// last vector of an unaligned or ragged row are read element by element
// under a bounds mask, masked elements being the function's identity.
// The block form keeps four such loads in flight per thread on four
// accumulators; the wave form one, two or four, by the row's length. k_reduce_cols gives each lane 8 consecutive channels (one
// 16-byte load per slice, four slices in flight) when inner % 8 == 0 and
// the pointers allow, one channel otherwise; per-slice partials meet in
// LDS (8 KB), fold across TY and leave in one 16-byte store.
//
// Max and min skip NaN elements (fmaxf / fminf); a row of NaNs answers
// the identity (-inf / +inf). Sum, mean and prod propagate NaN.
#include "../common.h"
#include "../kernels.h"

#include <stdexcept>
#include <string>

// The float arithmetic of this file is compiled without packed f32
// instructions (v_pk_add_f32 and kin): the extension's flags are shared
// by every source, so the feature is switched off here, for the device
// pass only (the host pass does not know it).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                   \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace tfsc {

namespace {

constexpr int RED_TPB = 256;
constexpr int RED_WAVES = RED_TPB / WAVE;
constexpr int RED_MAX_BLOCKS = 1 << 20;   // grid-stride past this
constexpr int RED_UNROLL = 4;             // 16-byte loads in flight / thread

enum RedFn : int { RED_MEAN = 0, RED_SUM, RED_MAX, RED_MIN, RED_PROD };

// measured on the MI355X, profiles/reductions.md; scripts/reduce_probe.py
// moves them to time both sides
int g_wave_max_cols = 2048;   // rows up to this go one wave per row
int g_cols_tx_max = 64;       // lanes along inner of one k_reduce_cols tile
int g_cols_wg_target = 512;   // narrow the tile while fewer workgroups
constexpr int COLS_TX_MIN = 8;   // 8 lanes of 16 bytes: one 128-byte line

template <int FN> TFSC_DEV float red_identity() {
  if constexpr (FN == RED_MAX) return -INFINITY;
  else if constexpr (FN == RED_MIN) return INFINITY;
  else if constexpr (FN == RED_PROD) return 1.f;
  else return 0.f;
}

template <int FN> TFSC_DEV float red_op(float a, float b) {
  if constexpr (FN == RED_MAX) return fmaxf(a, b);
  else if constexpr (FN == RED_MIN) return fminf(a, b);
  else if constexpr (FN == RED_PROD) return a * b;
  else return a + b;
}

// the 8 bf16 of one 16-byte vector as f32
TFSC_DEV void widen8(uint4 r, float f[8]) {
  uint32_t w[4] = {r.x, r.y, r.z, r.w};
  #pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[2 * j] = __uint_as_float(w[j] << 16);
    f[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
  }
}

TFSC_DEV float to_f32(ushort v) { return bf2f(v); }
TFSC_DEV float to_f32(float v) { return v; }

// all elements of one 16-byte vector folded into one value
template <int FN> TFSC_DEV float fold(uint4 r, ushort) {
  float f[8];
  widen8(r, f);
  return red_op<FN>(
      red_op<FN>(red_op<FN>(f[0], f[1]), red_op<FN>(f[2], f[3])),
      red_op<FN>(red_op<FN>(f[4], f[5]), red_op<FN>(f[6], f[7])));
}
template <int FN> TFSC_DEV float fold(uint4 r, float) {
  return red_op<FN>(
      red_op<FN>(__uint_as_float(r.x), __uint_as_float(r.y)),
      red_op<FN>(__uint_as_float(r.z), __uint_as_float(r.w)));
}

// n elements starting at p, seen from the 16-byte boundary at or below p.
// Vectors [v_lo, v_hi) lie whole inside the elements; vector 0 and vector
// v_hi can be partial.
template <int FN, typename T>
struct Frame {
  static constexpr int V = 16 / int(sizeof(T));
  const T* base;   // 16-byte aligned
  int64_t lo, hi;  // frame positions [lo, hi) hold the elements

  TFSC_DEV Frame(const T* p, int64_t n) {
    int shift = int((reinterpret_cast<uintptr_t>(p) & 15u) / sizeof(T));
    base = p - shift;
    lo = shift;
    hi = shift + n;
  }
  TFSC_DEV int64_t v_lo() const { return lo > 0 ? 1 : 0; }
  TFSC_DEV int64_t v_hi() const { return hi / V; }
  TFSC_DEV uint4 raw(int64_t v) const {
    return *reinterpret_cast<const uint4*>(base + v * V);
  }
  // a partial vector: element by element, the rest is the identity
  TFSC_DEV float edge(int64_t v) const {
    float a = red_identity<FN>();
    #pragma unroll
    for (int j = 0; j < V; ++j) {
      int64_t q = v * V + j;
      if (q >= lo && q < hi) a = red_op<FN>(a, to_f32(base[q]));
    }
    return a;
  }
  // thread 0 takes the partial first vector, thread 1 the partial last
  // one (the same vector when everything lies inside vector 0)
  TFSC_DEV float edges(int t) const {
    const bool head = lo > 0, tail = hi % V != 0 && !(head && hi < V);
    if (t == 0 && head) return edge(0);
    if (t == 1 && tail) return edge(hi / V);
    return red_identity<FN>();
  }
};

// Thread t of STRIDE folds its share of the frame. The whole vectors go
// U at a time: the loads are issued together, without a branch (a vector
// past the end re-reads the last whole one and is dropped), and land on
// accumulators of their own.
template <int FN, typename T, int STRIDE, int U>
TFSC_DEV float sweep(const Frame<FN, T>& fr, int t) {
  float acc[U];
  #pragma unroll
  for (int u = 0; u < U; ++u) acc[u] = red_identity<FN>();
  const int64_t v_hi = fr.v_hi();
  for (int64_t v0 = fr.v_lo() + t; v0 < v_hi; v0 += U * STRIDE) {
    uint4 r[U];
    #pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t v = v0 + u * STRIDE;
      r[u] = fr.raw(v < v_hi ? v : v_hi - 1);
    }
    #pragma unroll
    for (int u = 0; u < U; ++u) {
      const float f = fold<FN>(r[u], T());
      acc[u] = red_op<FN>(acc[u],
                          v0 + u * STRIDE < v_hi ? f : red_identity<FN>());
    }
  }
  float a = fr.edges(t);
  #pragma unroll
  for (int u = 0; u < U; ++u) a = red_op<FN>(a, acc[u]);
  return a;
}

template <int FN> TFSC_DEV float wave_reduce(float a) {
  #pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1)
    a = red_op<FN>(a, __shfl_xor(a, off, WAVE));
  return a;
}

// the value that leaves: an f32 partial, or the rounded result
template <int FN, bool PARTIAL>
TFSC_DEV void store_result(void* y, int64_t i, float a, float div) {
  if constexpr (PARTIAL) {
    static_cast<float*>(y)[i] = a;
  } else {
    if constexpr (FN == RED_MEAN) a = a / div;
    static_cast<ushort*>(y)[i] = f2bf(a);
  }
}

// ---------------------------------------------------------------------------
// inner == 1, short rows: one wave per row, cross-lane shuffles only. U
// loads in flight per lane: 1 when 64 lanes cover the row in one step
// ---------------------------------------------------------------------------
template <int FN, typename T, int U>
__global__ __launch_bounds__(RED_TPB)
void k_reduce_rows_wave(const T* __restrict__ x, void* __restrict__ y,
                        int64_t rows, int64_t cols, float div) {
  const int lane = threadIdx.x % WAVE;
  const int64_t w0 = int64_t(blockIdx.x) * RED_WAVES + threadIdx.x / WAVE;
  for (int64_t row = w0; row < rows;
       row += int64_t(gridDim.x) * RED_WAVES) {
    Frame<FN, T> fr(x + row * cols, cols);
    float a = wave_reduce<FN>(sweep<FN, T, WAVE, U>(fr, lane));
    if (lane == 0) store_result<FN, false>(y, row, a, div);
  }
}

// ---------------------------------------------------------------------------
// inner == 1, long rows: one workgroup per (row, segment); segment `seg`
// of a row is columns [seg * seglen, min(cols, (seg + 1) * seglen))
// ---------------------------------------------------------------------------
template <int FN, typename T, bool PARTIAL>
__global__ __launch_bounds__(RED_TPB)
void k_reduce_rows_block(const T* __restrict__ x, void* __restrict__ y,
                         int64_t rows, int64_t cols, int64_t P,
                         int64_t seglen, float div) {
  __shared__ float wave_s[RED_WAVES];
  const int tid = threadIdx.x;
  for (int64_t w = blockIdx.x; w < rows * P; w += gridDim.x) {
    const int64_t row = P == 1 ? w : w / P, seg = w - row * P;
    const int64_t c0 = seg * seglen;
    const int64_t n = (cols - c0 < seglen ? cols - c0 : seglen);
    Frame<FN, T> fr(x + row * cols + c0, n > 0 ? n : 0);
    float a = wave_reduce<FN>(sweep<FN, T, RED_TPB, RED_UNROLL>(fr, tid));
    if (tid % WAVE == 0) wave_s[tid / WAVE] = a;
    __syncthreads();
    if (tid == 0) {
      a = red_op<FN>(red_op<FN>(wave_s[0], wave_s[1]),
                     red_op<FN>(wave_s[2], wave_s[3]));
      store_result<FN, PARTIAL>(y, w, a, div);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// inner > 1: [outer, red, inner] -> [outer, inner]. Work item = (outer
// index, tile of TX * VEC channels, segment of red); tx walks the tile's
// channels, ty the segment's slices at stride TY.
// ---------------------------------------------------------------------------
template <int FN, int VEC, bool PARTIAL>
__global__ __launch_bounds__(RED_TPB)
void k_reduce_cols(const ushort* __restrict__ x, void* __restrict__ y,
                   int64_t outer, int64_t red, int64_t inner, int64_t P,
                   int64_t seglen, int lg_tx, float div) {
  __shared__ float part_s[RED_TPB * VEC];
  const int TX = 1 << lg_tx, TY = RED_TPB >> lg_tx;
  const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> lg_tx;
  const int64_t tiles = (inner + int64_t(TX) * VEC - 1) / (int64_t(TX) * VEC);
  float* mine = part_s + threadIdx.x * VEC;
  for (int64_t w = blockIdx.x; w < outer * tiles * P; w += gridDim.x) {
    const int64_t seg = w % P, tile = (w / P) % tiles, o = w / (P * tiles);
    const int64_t c0 = (tile * TX + tx) * VEC;
    const int64_t j0 = seg * seglen;
    const int64_t j1 = red - j0 < seglen ? red : j0 + seglen;
    float acc[VEC];
    #pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = red_identity<FN>();
    if (c0 < inner) {
      const ushort* xp = x + o * red * inner + c0;
      int64_t j = j0 + ty;
      if constexpr (VEC == 8) {
        for (; j + int64_t(RED_UNROLL - 1) * TY < j1;
             j += int64_t(RED_UNROLL) * TY) {
          uint4 r[RED_UNROLL];
          #pragma unroll
          for (int u = 0; u < RED_UNROLL; ++u)
            r[u] = *reinterpret_cast<const uint4*>(
                xp + (j + int64_t(u) * TY) * inner);
          #pragma unroll
          for (int u = 0; u < RED_UNROLL; ++u) {
            float f[8];
            widen8(r[u], f);
            #pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = red_op<FN>(acc[e], f[e]);
          }
        }
        for (; j < j1; j += TY) {
          float f[8];
          widen8(*reinterpret_cast<const uint4*>(xp + j * inner), f);
          #pragma unroll
          for (int e = 0; e < 8; ++e) acc[e] = red_op<FN>(acc[e], f[e]);
        }
      } else {
        float b[RED_UNROLL];
        for (; j + int64_t(RED_UNROLL - 1) * TY < j1;
             j += int64_t(RED_UNROLL) * TY) {
          #pragma unroll
          for (int u = 0; u < RED_UNROLL; ++u)
            b[u] = bf2f(xp[(j + int64_t(u) * TY) * inner]);
          #pragma unroll
          for (int u = 0; u < RED_UNROLL; ++u)
            acc[0] = red_op<FN>(acc[0], b[u]);
        }
        for (; j < j1; j += TY) acc[0] = red_op<FN>(acc[0], bf2f(xp[j * inner]));
      }
    }
    #pragma unroll
    for (int e = 0; e < VEC; ++e) mine[e] = acc[e];
    __syncthreads();
    // fold the TY slices: row ty takes row ty + s
    for (int s = TY >> 1; s > 0; s >>= 1) {
      if (ty < s) {
        const float* other = mine + s * TX * VEC;
        #pragma unroll
        for (int e = 0; e < VEC; ++e) mine[e] = red_op<FN>(mine[e], other[e]);
      }
      __syncthreads();
    }
    if (ty == 0 && c0 < inner) {
      const int64_t out = o * inner + c0;
      if constexpr (PARTIAL) {
        #pragma unroll
        for (int e = 0; e < VEC; ++e)
          static_cast<float*>(y)[(out + e) * P + seg] = mine[e];
      } else if constexpr (VEC == 8) {
        float f[8];
        #pragma unroll
        for (int e = 0; e < 8; ++e)
          f[e] = FN == RED_MEAN ? mine[e] / div : mine[e];
        *reinterpret_cast<uint4*>(static_cast<ushort*>(y) + out) =
            make_uint4(f2bf2(f[0], f[1]), f2bf2(f[2], f[3]),
                       f2bf2(f[4], f[5]), f2bf2(f[6], f[7]));
      } else {
        store_result<FN, false>(y, out, mine[0], div);
      }
    }
    __syncthreads();
  }
}

int grid_of(int64_t items) {
  return int(items < RED_MAX_BLOCKS ? (items > 0 ? items : 1)
                                    : RED_MAX_BLOCKS);
}

// rows of `cols` elements of T -> one value each (P == 1), or P partials
template <int FN, typename T, bool PARTIAL>
void rows_launch(hipStream_t s, const T* x, void* y, int64_t rows,
                 int64_t cols, int64_t P, float div) {
  if constexpr (!PARTIAL) {
    if (P == 1 && cols <= g_wave_max_cols) {
      const dim3 grid(grid_of(ceil_div(rows, RED_WAVES)));
      const int64_t nv = ceil_div(cols * int64_t(sizeof(T)), 16);
      if (nv <= WAVE)
        hipLaunchKernelGGL((k_reduce_rows_wave<FN, T, 1>), grid,
                           dim3(RED_TPB), 0, s, x, y, rows, cols, div);
      else if (nv <= 2 * WAVE)
        hipLaunchKernelGGL((k_reduce_rows_wave<FN, T, 2>), grid,
                           dim3(RED_TPB), 0, s, x, y, rows, cols, div);
      else
        hipLaunchKernelGGL((k_reduce_rows_wave<FN, T, RED_UNROLL>), grid,
                           dim3(RED_TPB), 0, s, x, y, rows, cols, div);
      return;
    }
  }
  hipLaunchKernelGGL((k_reduce_rows_block<FN, T, PARTIAL>),
                     dim3(grid_of(rows * P)), dim3(RED_TPB), 0, s, x, y,
                     rows, cols, P, ceil_div(cols, P), div);
}

template <int FN, bool PARTIAL>
void cols_launch(hipStream_t s, const ushort* x, void* y, int64_t outer,
                 int64_t red, int64_t inner, int64_t P, float div) {
  // 16-byte loads and stores need every slice to start on a boundary
  const bool vec = inner % 8 == 0 &&
                   reinterpret_cast<uintptr_t>(x) % 16 == 0 &&
                   (PARTIAL || reinterpret_cast<uintptr_t>(y) % 16 == 0);
  const int lg_tx = reduce_cols_lg_tx(outer, inner, P, vec);
  const int64_t per_tile = (int64_t(1) << lg_tx) * (vec ? 8 : 1);
  const int grid = grid_of(outer * ceil_div(inner, per_tile) * P);
  const int64_t seglen = ceil_div(red, P);
  if (vec)
    hipLaunchKernelGGL((k_reduce_cols<FN, 8, PARTIAL>), dim3(grid),
                       dim3(RED_TPB), 0, s, x, y, outer, red, inner, P,
                       seglen, lg_tx, div);
  else
    hipLaunchKernelGGL((k_reduce_cols<FN, 1, PARTIAL>), dim3(grid),
                       dim3(RED_TPB), 0, s, x, y, outer, red, inner, P,
                       seglen, lg_tx, div);
}

template <int FN>
void reduce_fn(hipStream_t s, const ushort* x, ushort* y, float* scratch,
               int64_t outer, int64_t red, int64_t inner, int64_t P) {
  const float div = float(red);
  if (P == 1) {
    if (inner == 1)
      rows_launch<FN, ushort, false>(s, x, y, outer, red, 1, div);
    else
      cols_launch<FN, false>(s, x, y, outer, red, inner, 1, div);
    return;
  }
  if (inner == 1)
    rows_launch<FN, ushort, true>(s, x, scratch, outer, red, P, div);
  else
    cols_launch<FN, true>(s, x, scratch, outer, red, inner, P, div);
  rows_launch<FN, float, false>(s, scratch, y, outer * inner, P, 1, div);
}

}  // namespace

int reduce_cols_lg_tx(int64_t outer, int64_t inner, int64_t P, bool vec) {
  // no wider than inner needs, so a narrow tensor keeps all 256 threads
  // busy along red; then, with 16-byte lanes, halved down to one cache
  // line while the launch has fewer workgroups than the target: a
  // narrower tile is more workgroups, each with more slices in flight
  const int64_t lanes = vec ? inner / 8 : inner;
  int lg = 0;
  while ((int64_t(1) << lg) < lanes && (1 << lg) < g_cols_tx_max) ++lg;
  while (vec && (1 << lg) > COLS_TX_MIN &&
         outer * ceil_div(lanes, int64_t(1) << lg) * P < g_cols_wg_target)
    --lg;
  return lg;
}

int reduce_wave_max_cols() { return g_wave_max_cols; }
int reduce_cols_tx_max() { return g_cols_tx_max; }
int reduce_cols_wg_target() { return g_cols_wg_target; }

void set_reduce_thresholds(int wave_max_cols, int cols_tx_max,
                           int cols_wg_target) {
  if (wave_max_cols < 0 || cols_tx_max < 1 || cols_tx_max > RED_TPB ||
      (cols_tx_max & (cols_tx_max - 1)) != 0 || cols_wg_target < 0)
    throw std::runtime_error("reduce: bad thresholds");
  g_wave_max_cols = wave_max_cols;
  g_cols_tx_max = cols_tx_max;
  g_cols_wg_target = cols_wg_target;
}

void launch_reduce(hipStream_t s, const ushort* x, ushort* y, void* scratch,
                   int64_t outer, int64_t red, int64_t inner, int fn,
                   int64_t P) {
  if (outer < 1 || red < 1 || inner < 1)
    throw std::runtime_error("reduce: bad view [" + std::to_string(outer) +
                             ", " + std::to_string(red) + ", " +
                             std::to_string(inner) + "]");
  if (P < 1 || P > red || P > 4096)
    throw std::runtime_error("reduce: P = " + std::to_string(P) +
                             " outside [1, min(red, 4096)]");
  if (P > 1 && (scratch == nullptr ||
                reinterpret_cast<uintptr_t>(scratch) % 4 != 0))
    throw std::runtime_error("reduce: a split needs 4-byte aligned scratch");
  float* scr = static_cast<float*>(scratch);
  switch (fn) {
    case RED_MEAN: reduce_fn<RED_MEAN>(s, x, y, scr, outer, red, inner, P); break;
    case RED_SUM: reduce_fn<RED_SUM>(s, x, y, scr, outer, red, inner, P); break;
    case RED_MAX: reduce_fn<RED_MAX>(s, x, y, scr, outer, red, inner, P); break;
    case RED_MIN: reduce_fn<RED_MIN>(s, x, y, scr, outer, red, inner, P); break;
    case RED_PROD: reduce_fn<RED_PROD>(s, x, y, scr, outer, red, inner, P); break;
    default:
      throw std::runtime_error("reduce: unknown fn " + std::to_string(fn));
  }
}

}  // namespace tfsc

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
