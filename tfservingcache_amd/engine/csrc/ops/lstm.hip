// Fused LSTM (TF BlockLSTM / BlockLSTMV2) for gfx950: the recurrence
//
//   pre = x_t W_x + b  +  h_{t-1} W_h         (x W_x + b comes in as `pre`)
//   i = s(pre_i + c wci)   f = s(pre_f + c wcf)   g = tanh(pre_ci)
//   c' = g i + c f, clamped to +-clip when clip > 0
//   o = s(pre_o + c' wco)  h = o tanh(c')
//
// The per-step GEMM is tiny (M = batch <= 32, K = H, N = 4H) and its
// weight is reused T times, so neither kernel here uses the 128x128 tile
// pipeline of gemm.hip. Both put the batch on the M side of
// v_mfma_f32_16x16x32_bf16 (16-row batch tiles, the last one partial) and
// a tile of 16 hidden units with all four of their gates on the N side.
//
// Column order. W_h is [N][Kp] bf16 (the GEMM weight transform of the
// planner's [H, N] master), N = 64 * ceil(H / 16), Kp = pad64(H), and
// `pre` is [rows][N]. Column n = (j / 16) * 64 + (j % 16) * 4 + gate holds
// gate (0 i, 1 ci, 2 f, 3 o) of unit j. Four MFMA accumulators, one per
// gate, then leave lane l with the four gates of unit j = tile * 16 +
// (l & 15) for batch rows (l >> 4) * 4 + r: the gate maths is lane-local,
// and a lane's four `pre` values are one 8-byte load.
//
// Units j >= H inside the last tile are padding: their W_x, b and W_h
// columns are zero, so pre = 0, c stays 0 and h = o * tanh(0) = 0. The
// kernels store j < H only and read h columns k >= H as zero.
//
// lstm_resident_kernel: one workgroup per batch tile runs all T steps.
//   W_h lives in LDS for the whole sequence (XOR-swizzled 16-byte chunks);
//   wave w owns unit tile w (at most 8 tiles, H <= 128, whatever the LDS
//   size); c stays in f32 registers; h_t is rounded to bf16 once, stored,
//   and written to the other of two LDS h buffers as the next step's A
//   operand. One barrier per step.
// lstm_step_kernel: one launch per step, grid = unit tiles x batch tiles.
//   K is split over the block's four waves and the partial accumulators
//   meet in LDS; wave w then finishes accumulator row r = w, so all 256
//   threads share the epilogue. W_h streams from L2; h_{t-1} is read from
//   the output tensor (h0 at t = 0); c lives in the f32 scratch, which
//   step 0 initialises from c0 (or zero) without reading it.
// No workgroup ever waits for another one.
#include "../common.h"
#include "../kernels.h"

#include <stdexcept>
#include <string>
#include <utility>

// The float arithmetic of this file is compiled without packed f32
// instructions (v_pk_add_f32 and kin): the extension's flags are shared
// by every source, so the feature is switched off here, for the device
// pass only (the host pass does not know it).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                   \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace tfsc {

using bf16x8_t = __attribute__((ext_vector_type(8))) __bf16;
using f32x4_t = __attribute__((ext_vector_type(4))) float;

struct LstmArgs {
  const ushort* pre;      // [rows][N]
  const ushort* wh;       // [N][Kp]
  const ushort* wci;      // [H] or null (all three or none)
  const ushort* wcf;
  const ushort* wco;
  const ushort* h0;       // [B][H] or null
  const ushort* c0;       // [B][H] or null
  float* cstate;          // [B][H], stepped kernel only
  ushort* h;              // row (t, b) at t * st_t + b * st_b
  ushort* cs;             // same addressing, or null
  int T, B, H, N, Kp;
  int64_t st_t, st_b;     // elements
  int64_t pre_t, pre_b;   // rows of `pre`
  float clip;
};

TFSC_DEV float sigmoid_fast(float v) { return 1.f / (1.f + __expf(-v)); }
// exact at both tails: exp -> inf gives 1, exp -> 0 gives -1
TFSC_DEV float tanh_fast(float v) { return 1.f - 2.f / (1.f + __expf(2.f * v)); }

// One (unit, batch row) cell update from the four gate pre-activations.
// Returns h as bf16; c is updated in place.
TFSC_DEV ushort lstm_cell(float pi, float pg, float pf, float po, float& c,
                          float wci, float wcf, float wco, float clip) {
  float i = sigmoid_fast(pi + c * wci);
  float f = sigmoid_fast(pf + c * wcf);
  float g = tanh_fast(pg);
  float cn = g * i + c * f;
  if (clip > 0.f) cn = fminf(fmaxf(cn, -clip), clip);
  float o = sigmoid_fast(po + cn * wco);
  c = cn;
  return f2bf(o * tanh_fast(cn));
}

// Functions of the HIP headers keep the packed-f32 feature, and a function
// with a feature its caller lacks is called, not inlined: a call per step
// costs the resident kernel 1 us of its 1.5. So the barrier is spelt with
// builtins (what __syncthreads() expands to) and the 8-byte load uses a
// plain struct, not uint2 and its constructors.
TFSC_DEV void block_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

struct alignas(8) Gates4 { uint32_t x, y; };    // bf16 i, ci | f, o

// the four bf16 gates of one (row, unit): 8 bytes, 8-byte aligned
TFSC_DEV Gates4 load_pre(const ushort* pre, int64_t row, int N, int col) {
  return *reinterpret_cast<const Gates4*>(pre + row * N + col);
}

TFSC_DEV float lo_bf(uint32_t w) { return bf2f(ushort(w & 0xffffu)); }
TFSC_DEV float hi_bf(uint32_t w) { return bf2f(ushort(w >> 16)); }

// byte offset of 16-byte chunk `chunk` of row `row` in an LDS image whose
// rows are Kp bf16; chunks are XOR-swizzled inside each group of 8 (128
// bytes) so the 16 rows of a fragment read hit different banks
TFSC_DEV int lds_chunk(int row, int chunk, int Kp, int key) {
  return row * Kp * 2 + (((chunk & ~7) | ((chunk & 7) ^ (key & 7))) << 4);
}

constexpr int LSTM_RES_MAX_WAVES = 8;        // one unit tile per wave

__global__ __launch_bounds__(LSTM_RES_MAX_WAVES * WAVE)
void lstm_resident_kernel(LstmArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Kp = a.Kp, H = a.H, N = a.N;
  const int b0 = blockIdx.x * 16;
  char* w_lds = smem;                           // [N][Kp]
  char* h_lds = smem + (size_t)N * Kp * 2;      // 2 x [16][Kp]
  const int h_bytes = 16 * Kp * 2;

  // W_h -> LDS, swizzled by the row's unit (row >> 2)
  const int cpr = Kp >> 3;                      // chunks per row
  for (int idx = tid; idx < N * cpr; idx += blockDim.x) {
    int n = idx / cpr, ch = idx - n * cpr;
    bf16x8 v = *reinterpret_cast<const bf16x8*>(a.wh + (size_t)n * Kp + ch * 8);
    *reinterpret_cast<bf16x8*>(w_lds + lds_chunk(n, ch, Kp, n >> 2)) = v;
  }
  // both h buffers zero (columns >= H and rows >= B stay zero), then h0
  for (int idx = tid; idx < 2 * 16 * cpr; idx += blockDim.x)
    reinterpret_cast<bf16x8*>(h_lds)[idx] = bf16x8{};
  block_sync();
  if (a.h0) {
    for (int idx = tid; idx < 16 * H; idx += blockDim.x) {
      int r = idx / H, j = idx - r * H;
      if (b0 + r < a.B)
        *reinterpret_cast<ushort*>(h_lds + lds_chunk(r, j >> 3, Kp, r) +
                                   (j & 7) * 2) =
            a.h0[(int64_t)(b0 + r) * H + j];
    }
  }

  const int u = lane & 15;                      // unit in tile / A row
  const int kgrp = lane >> 4;                   // K chunk in a 32-step
  const int rb = kgrp * 4;                      // first batch row of acc
  const int tile = wave;                        // blockDim.x = n_tiles * 64
  const int j = tile * 16 + u;
  const bool live = j < H;
  const float wci = live && a.wci ? bf2f(a.wci[j]) : 0.f;
  const float wcf = live && a.wcf ? bf2f(a.wcf[j]) : 0.f;
  const float wco = live && a.wco ? bf2f(a.wco[j]) : 0.f;
  float c[4];
  #pragma unroll
  for (int r = 0; r < 4; ++r) {
    int b = b0 + rb + r;
    c[r] = live && a.c0 && b < a.B ? bf2f(a.c0[(int64_t)b * H + j]) : 0.f;
  }
  block_sync();

  int cur = 0;
  for (int t = 0; t < a.T; ++t) {
    const char* hin = h_lds + cur * h_bytes;
    char* hout = h_lds + (cur ^ 1) * h_bytes;
    {
      // this step's pre-activations: issued before the MFMA loop so the
      // loads fly under it
      Gates4 pv[4];
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        int b = b0 + rb + r;
        pv[r] = b < a.B
            ? load_pre(a.pre, t * a.pre_t + b * a.pre_b, N, tile * 64 + u * 4)
            : Gates4{0u, 0u};
      }
      f32x4_t acc[4] = {};
      for (int ks = 0; ks < (Kp >> 5); ++ks) {
        const int ch = ks * 4 + kgrp;
        bf16x8_t af = *reinterpret_cast<const bf16x8_t*>(
            hin + lds_chunk(u, ch, Kp, u));
        #pragma unroll
        for (int g = 0; g < 4; ++g) {
          bf16x8_t bfrag = *reinterpret_cast<const bf16x8_t*>(
              w_lds + lds_chunk(tile * 64 + u * 4 + g, ch, Kp, tile * 16 + u));
          acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfrag, acc[g],
                                                           0, 0, 0);
        }
      }
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rb + r, b = b0 + row;
        ushort hv = lstm_cell(acc[0][r] + lo_bf(pv[r].x),
                              acc[1][r] + hi_bf(pv[r].x),
                              acc[2][r] + lo_bf(pv[r].y),
                              acc[3][r] + hi_bf(pv[r].y), c[r], wci, wcf,
                              wco, a.clip);
        *reinterpret_cast<ushort*>(hout + lds_chunk(row, j >> 3, Kp, row) +
                                   (j & 7) * 2) = hv;
        if (b < a.B && j < H) {
          int64_t off = t * a.st_t + b * a.st_b + j;
          a.h[off] = hv;
          if (a.cs) a.cs[off] = f2bf(c[r]);
        }
      }
    }
    block_sync();
    cur ^= 1;
  }
}

constexpr int LSTM_STEP_WAVES = 4;

// hp: h_{t-1} rows at hp + b * hp_sb (null: zero state, no MFMA); cin:
// f32 c_{t-1} (cstate), or null at t == 0 where c0 (bf16, may be null too)
// is read instead. vec: 16-byte loads of hp are legal.
__global__ __launch_bounds__(LSTM_STEP_WAVES * WAVE)
void lstm_step_kernel(LstmArgs a, int t, const ushort* hp, int64_t hp_sb,
                      bool first, bool vec) {
  __shared__ float red[LSTM_STEP_WAVES * 16 * WAVE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Kp = a.Kp, H = a.H, N = a.N;
  const int tile = blockIdx.x, b0 = blockIdx.y * 16;
  const int u = lane & 15, kgrp = lane >> 4;

  // epilogue coordinates: wave w finishes accumulator row r = w
  const int row = kgrp * 4 + wave, b = b0 + row, j = tile * 16 + u;
  Gates4 pv = b < a.B
      ? load_pre(a.pre, t * a.pre_t + b * a.pre_b, N, tile * 64 + u * 4)
      : Gates4{0u, 0u};

  f32x4_t acc[4] = {};
  if (hp) {
    int ab = b0 + u;                            // A row = batch row
    ab = ab < a.B ? ab : a.B - 1;               // clamped; rows >= B unused
    const ushort* arow = hp + ab * hp_sb;
    for (int ks = wave; ks < (Kp >> 5); ks += LSTM_STEP_WAVES) {
      const int k = ks * 32 + kgrp * 8;
      bf16x8 av = {};
      if (vec) {
        if (k < H) av = *reinterpret_cast<const bf16x8*>(arow + k);
      } else {
        #pragma unroll
        for (int e = 0; e < 8; ++e)
          if (k + e < H) av[e] = (short)arow[k + e];
      }
      bf16x8_t af = __builtin_bit_cast(bf16x8_t, av);
      #pragma unroll
      for (int g = 0; g < 4; ++g) {
        bf16x8_t bfrag = *reinterpret_cast<const bf16x8_t*>(
            a.wh + (size_t)(tile * 64 + u * 4 + g) * Kp + k);
        acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfrag, acc[g],
                                                         0, 0, 0);
      }
    }
  }
  #pragma unroll
  for (int g = 0; g < 4; ++g)
    #pragma unroll
    for (int r = 0; r < 4; ++r)
      red[((wave * 4 + g) * 4 + r) * WAVE + lane] = acc[g][r];
  block_sync();
  float p[4];
  #pragma unroll
  for (int g = 0; g < 4; ++g) {
    float sum = 0.f;
    #pragma unroll
    for (int w = 0; w < LSTM_STEP_WAVES; ++w)
      sum += red[((w * 4 + g) * 4 + wave) * WAVE + lane];
    p[g] = sum;
  }
  if (b >= a.B || j >= H) return;
  const int64_t ci = (int64_t)b * H + j;
  float c = first ? (a.c0 ? bf2f(a.c0[ci]) : 0.f) : a.cstate[ci];
  ushort hv = lstm_cell(p[0] + lo_bf(pv.x), p[1] + hi_bf(pv.x),
                        p[2] + lo_bf(pv.y), p[3] + hi_bf(pv.y), c,
                        a.wci ? bf2f(a.wci[j]) : 0.f,
                        a.wcf ? bf2f(a.wcf[j]) : 0.f,
                        a.wco ? bf2f(a.wco[j]) : 0.f, a.clip);
  a.cstate[ci] = c;
  const int64_t off = t * a.st_t + b * a.st_b + j;
  a.h[off] = hv;
  if (a.cs) a.cs[off] = f2bf(c);
}

// ---------------------------------------------------------------------------
// launcher

static int64_t lstm_resident_lds_bytes(int64_t H) {
  int64_t N = 64 * ceil_div(H, 16), Kp = 64 * ceil_div(H, 64);
  return N * Kp * 2 + 2 * 16 * Kp * 2;
}

static int64_t lstm_lds_limit() {
  static int64_t limit = [] {
    int dev = 0, v = 0;
    HIP_CHECK(hipGetDevice(&dev));
    HIP_CHECK(hipDeviceGetAttribute(
        &v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    return int64_t(v);
  }();
  return limit;
}

// largest H the resident kernel can hold: W_h and two h buffers inside the
// LDS one workgroup may allocate, one unit tile per wave
static int lstm_resident_fit_h() {
  static int fit = [] {
    int h = 0;
    const int cap = LSTM_RES_MAX_WAVES * 16;
    while (h < cap && lstm_resident_lds_bytes(h + 1) <= lstm_lds_limit()) ++h;
    return h;
  }();
  return fit;
}

static int g_lstm_resident_max_h = -1;          // -1: the LDS-derived limit

int lstm_resident_max_h() {
  return g_lstm_resident_max_h < 0 ? lstm_resident_fit_h()
                                   : g_lstm_resident_max_h;
}

void set_lstm_resident_max_h(int h) {
  if (h < 0)
    g_lstm_resident_max_h = -1;
  else
    g_lstm_resident_max_h = h < lstm_resident_fit_h() ? h
                                                      : lstm_resident_fit_h();
}

// rows of `len` elements at t * st_t + b * st_b must not overlap. A
// sufficient test: the axis with the smaller stride must fit inside one
// step of the other, which holds for both layouts the emitter makes and
// refuses interleavings that would also be disjoint
static bool lstm_rows_disjoint(int64_t T, int64_t B, int64_t st_t,
                               int64_t st_b, int64_t len) {
  if (st_t < 0 || st_b < 0) return false;
  int64_t ns = T, ss = st_t, nl = B, sl = st_b;   // small / large stride
  if (nl == 1 || (ns > 1 && ss > sl)) {
    std::swap(ns, nl);
    std::swap(ss, sl);
  }
  if (ns > 1 && ss < len) return false;
  if (nl > 1 && sl < (ns - 1) * ss + len) return false;
  return true;
}

void launch_lstm(hipStream_t s, const ushort* pre, const ushort* wh,
                 const ushort* wci, const ushort* wcf, const ushort* wco,
                 const ushort* h0, const ushort* c0, float* cstate,
                 ushort* h, ushort* cs, int64_t T, int64_t B, int64_t H,
                 int64_t st_t, int64_t st_b, int64_t pre_t, int64_t pre_b,
                 float clip) {
  if (T < 1 || B < 1 || H < 1)
    throw std::runtime_error("lstm: T, B and H must be >= 1 (got " +
                             std::to_string(T) + ", " + std::to_string(B) +
                             ", " + std::to_string(H) + ")");
  if (!pre || !wh || !h || !cstate)
    throw std::runtime_error("lstm: pre, W_h, h and the cell scratch must "
                             "be set");
  if ((wci != nullptr) != (wcf != nullptr) ||
      (wci != nullptr) != (wco != nullptr))
    throw std::runtime_error("lstm: peephole needs wci, wcf and wco");
  if (!lstm_rows_disjoint(T, B, st_t, st_b, H) ||
      !lstm_rows_disjoint(T, B, pre_t, pre_b, 1))
    throw std::runtime_error("lstm: rows overlap under the given strides");
  if (H > (1 << 20) || T * B > INT32_MAX / 2)
    throw std::runtime_error("lstm: extent out of range");
  if (!(clip >= 0.f)) throw std::runtime_error("lstm: cell_clip < 0");

  LstmArgs a;
  a.pre = pre; a.wh = wh; a.wci = wci; a.wcf = wcf; a.wco = wco;
  a.h0 = h0; a.c0 = c0; a.cstate = cstate; a.h = h; a.cs = cs;
  a.T = int(T); a.B = int(B); a.H = int(H);
  a.N = int(64 * ceil_div(H, 16));
  a.Kp = int(64 * ceil_div(H, 64));
  a.st_t = st_t; a.st_b = st_b; a.pre_t = pre_t; a.pre_b = pre_b;
  a.clip = clip;
  const unsigned btiles = unsigned(ceil_div(B, 16));
  const int n_tiles = a.N / 64;

  if (H <= lstm_resident_max_h()) {
    const size_t lds = size_t(lstm_resident_lds_bytes(H));
    // once per process: the engine drives one device per process
    static const bool attr_set = [] {
      HIP_CHECK(hipFuncSetAttribute(
          reinterpret_cast<const void*>(lstm_resident_kernel),
          hipFuncAttributeMaxDynamicSharedMemorySize, int(lstm_lds_limit())));
      return true;
    }();
    (void)attr_set;
    hipLaunchKernelGGL(lstm_resident_kernel, dim3(btiles),
                       dim3(n_tiles * WAVE), lds, s, a);
    HIP_CHECK(hipGetLastError());
    return;
  }
  const bool vec_ok = H % 8 == 0 && st_b % 8 == 0 && st_t % 8 == 0 &&
                      reinterpret_cast<uintptr_t>(h) % 16 == 0;
  for (int t = 0; t < a.T; ++t) {
    const ushort* hp = t == 0 ? h0 : h + (t - 1) * st_t;
    const int64_t hp_sb = t == 0 ? H : st_b;
    const bool vec = t == 0
        ? H % 8 == 0 && reinterpret_cast<uintptr_t>(h0) % 16 == 0
        : vec_ok;
    hipLaunchKernelGGL(lstm_step_kernel, dim3(n_tiles, btiles),
                       dim3(LSTM_STEP_WAVES * WAVE), 0, s, a, t, hp, hp_sb,
                       t == 0, vec);
  }
  HIP_CHECK(hipGetLastError());
}

}  // namespace tfsc

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
