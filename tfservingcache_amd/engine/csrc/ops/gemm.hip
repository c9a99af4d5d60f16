// bf16 MFMA GEMM for gfx950 — the serving hot path.
//
// C[M,N] = act(alpha * A[M,K] @ B^T[N,K] + bias [+ residual])
//
// Structure follows the CDNA4 canonical GEMM anatomy
// (/opt/skills/guides/cdna_hip_programming.md §5): 128x128 block tile,
// BK=64, 4 waves (one 64x64 wave tile each), double-buffered LDS filled
// with 16-byte `global_load_lds` (lane-linear dest, XOR-swizzled SOURCE
// address + matching XOR on the ds_read — §5.4 rule 21 / T2), MFMA
// v_mfma_f32_16x16x32_bf16 accumulating f32, fused
// bias/activation/residual epilogue.
//
// B is expected TRANSPOSED ([N][K] row-major): the planner pre-transposes
// weights at model-load time so both A and B fragments read contiguously
// along K. A variant with B in [K][N] (register-staged transpose on the
// fly) serves the batched attention P@V case.
//
// Row indices are clamped at the staging loads (no out-of-bounds reads on
// partial tiles); stores are masked by (row < M && col < N). K must be a
// multiple of 64 — the planner zero-pads weights and im2col buffers.
#include "../common.h"
#include "../kernels.h"

#include <algorithm>
#include <stdexcept>

namespace tfsc {

using bf16x8_t = __attribute__((ext_vector_type(8))) __bf16;
using f32x4_t = __attribute__((ext_vector_type(4))) float;

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int N_WAVES = 4;                // 2x2 wave grid of 64x64 tiles
constexpr int THREADS = N_WAVES * WAVE;   // 256

// XCD-aware blockIdx remap (guide T1, bijective variant): the dispatcher
// places block b on XCD b % 8, so consecutive tile ids (which share A/B
// panels) land on different per-XCD L2s; remapping gives each XCD a
// contiguous chunk of the grid. Applies when the kernel is HBM-bound
// (+10% on large GEMMs); bijective for any grid size.
TFSC_DEV int xcd_swizzle(int bid, int nblocks) {
  constexpr int NXCD = 8;
  if (nblocks < 2 * NXCD) return bid;
  int q = nblocks / NXCD, r = nblocks % NXCD;
  int xcd = bid % NXCD, idx = bid / NXCD;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// LDS tile: [128 rows][64 cols] bf16, 128-byte rows = 8 chunks of 16B.
// XOR swizzle: chunk' = chunk ^ (row & 7)  (T2: <=2-way conflicts).
TFSC_DEV int lds_off(int row, int chunk) {   // byte offset into a tile
  return row * 128 + ((chunk ^ (row & 7)) << 4);
}

template <int ROWS, int NWAVES>
TFSC_DEV void stage_tile_glds(const ushort* __restrict__ src, int64_t ld,
                              int row_limit, int row0, int k0,
                              char* lds_tile, int wave, int lane) {
  // the block's NWAVES waves stage ROWS rows together (each glds covers
  // 8 rows x 64 cols = 1 KiB); lane l covers (row = 8*i + l/8,
  // chunk = l%8) of its wave's slice. The glds LDS destination is
  // wave-uniform-base + lane*16 (lane-linear), which matches the
  // [row][chunk] image exactly.
  constexpr int ROWS_PER_WAVE = ROWS / NWAVES;
  constexpr int N_GLDS = ROWS_PER_WAVE / 8;
  int r_in = (lane >> 3);           // 0..7
  int chunk = lane & 7;             // 0..7
  #pragma unroll
  for (int i = 0; i < N_GLDS; ++i) {
    int row = wave * ROWS_PER_WAVE + i * 8 + r_in;
    int grow = row0 + row;
    grow = grow < row_limit ? grow : row_limit;
    // source chunk is pre-swizzled so the LINEAR lds image holds the
    // swizzled layout (rule 21: swizzle source + read, never the dest)
    int chunk_src = chunk ^ (row & 7);
    const ushort* gptr = src + (int64_t)grow * ld + k0 + chunk_src * 8;
    // wave-uniform base for this glds: start of the wave's 8-row slice
    char* lds_base = lds_tile + (wave * ROWS_PER_WAVE + i * 8) * 128;
    __builtin_amdgcn_global_load_lds(
        reinterpret_cast<const uint32_t*>(gptr),
        reinterpret_cast<uint32_t*>(lds_base), 16, 0, 0);
  }
}

// register-staged transpose path for B given as [K][N] (attention P@V):
// each lane loads 8 bf16 along N (coalesced) and scatters them into the
// [N][K]-image LDS tile with the same XOR swizzle.
template <int ROWS, int NWAVES>
TFSC_DEV void stage_tile_transposed(const ushort* __restrict__ src,
                                    int64_t ld, int k_limit, int n0, int k0,
                                    ushort* lds_tile, int wave, int lane,
                                    int n_limit) {
  // tile wanted: rows = n (ROWS), cols = k (64). Source element (k, n).
  constexpr int NG = ROWS / 8;            // n-groups of 8
  constexpr int THREADS_ = NWAVES * WAVE;
  constexpr int PASSES = (ROWS * 64) / (THREADS_ * 8);
  int tid = wave * WAVE + lane;
  #pragma unroll
  for (int pass = 0; pass < PASSES; ++pass) {
    int idx = pass * THREADS_ + tid;      // covers k-major: 64 k x NG groups
    int k = idx / NG;                     // 0..63
    int ng = idx % NG;                    // n-group of 8
    int gk = k0 + k;
    gk = gk < k_limit ? gk : k_limit;
    const ushort* gptr = src + (int64_t)gk * ld + n0 + ng * 8;
    ushort vals[8];
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      int gn = n0 + ng * 8 + j;
      vals[j] = (gn < n_limit) ? gptr[j] : ushort(0);
    }
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      int n = ng * 8 + j;
      int byte_off = lds_off(n, k >> 3) + (k & 7) * 2;
      *reinterpret_cast<ushort*>(
          reinterpret_cast<char*>(lds_tile) + byte_off) = vals[j];
    }
  }
}

TFSC_DEV float act_apply(float v, int act) {
  switch (act) {
    case ACT_RELU: return v > 0.f ? v : 0.f;
    case ACT_TANH: return tanhf(v);
    case ACT_SIGMOID: return 1.f / (1.f + __expf(-v));
    case ACT_GELU: return 0.5f * v * (1.f + erff(v * 0.70710678f));
    case ACT_RELU6: return v < 0.f ? 0.f : (v > 6.f ? 6.f : v);
    default: return v;
  }
}

// Coalesced epilogue: the MFMA C/D fragment layout scatters a lane's
// values over 2-byte strides, so direct stores are scalar ushort
// (32-byte wave segments — issue- and coalescing-poor, cf. guide T21).
// Instead each wave restages its 64x64 tile (acc*alpha + bias, bf16)
// through its own 8 KB LDS region, then streams it out row-major with
// 16-byte lanes — and reads the optional residual coalesced in the same
// pass. One __syncthreads() guards the LDS reuse of the staging tiles.
template <bool HAS_BIAS, bool HAS_RES>
TFSC_DEV void epilogue_store(f32x4_t (&acc)[4][4], char* smem,
                             const ushort* __restrict__ bias,
                             const ushort* __restrict__ residual,
                             ushort* __restrict__ Cb,
                             int M, int N, int m0, int n0, int wave,
                             int lane, int wm, int wn, int act,
                             float alpha) {
  __syncthreads();              // tiles are dead; reuse as staging
  ushort* stage = reinterpret_cast<ushort*>(smem + wave * 8192);
  const int col_in = lane & 15;
  const int row_base = (lane >> 4) * 4;
  #pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    #pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      int col = ni * 16 + col_in;
      float bv = HAS_BIAS ? bf2f(bias[n0 + wn * 64 + col]) : 0.f;
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = mi * 16 + row_base + r;
        // pad column stride by 0 (64 cols x 2B = 128 B rows; lanes of a
        // 16-lane group write 2B at 2B stride -> conflict-free halves)
        stage[row * 64 + col] = f2bf(acc[mi][ni][r] * alpha + bv);
      }
    }
  }
  __syncthreads();
  // stream out: iteration i, lane l -> linear 16B chunk i*64+l of the
  // wave's 64x64 tile (8 chunks per row) — consecutive lanes write
  // consecutive chunks (coalesced 1 KB per wave-instruction)
  #pragma unroll
  for (int i = 0; i < 8; ++i) {
    int chunk_id = i * 64 + lane;
    int row = chunk_id >> 3;
    int chunk = chunk_id & 7;
    int grow = m0 + wm * 64 + row;
    int gcol0 = n0 + wn * 64 + chunk * 8;
    if (grow >= M) continue;
    bf16x8 v = *reinterpret_cast<const bf16x8*>(stage + row * 64 +
                                                chunk * 8);
    int64_t goff = (int64_t)grow * N + gcol0;
    if (HAS_RES || act != ACT_NONE) {
      bf16x8 rv = {};
      if (HAS_RES && gcol0 + 7 < N)
        rv = *reinterpret_cast<const bf16x8*>(residual + goff);
      #pragma unroll
      for (int j = 0; j < 8; ++j) {
        float x = bf2f((ushort)v[j]);
        if (HAS_RES) {
          if (gcol0 + 7 < N) x += bf2f((ushort)rv[j]);
          else if (gcol0 + j < N) x += bf2f(residual[goff + j]);
        }
        v[j] = (short)f2bf(act_apply(x, act));
      }
    }
    if (gcol0 + 7 < N) {
      *reinterpret_cast<bf16x8*>(Cb + goff) = v;
    } else {
      for (int j = 0; j < 8 && gcol0 + j < N; ++j)
        Cb[goff + j] = (ushort)v[j];
    }
  }
}

// Geometry: WMW x WNW waves, each owning a 64x64 output tile
// (BM = WMW*64, BN = WNW*64). (2,2) = the full 128x128 tile; (1,2) and
// (1,1) keep medium shapes (e.g. BERT dense layers, attention batched
// GEMMs) from under-filling the 256-CU chip.
template <int WMW, int WNW, bool TRANS_B, bool HAS_BIAS, bool HAS_RES>
__global__ __launch_bounds__(WMW * WNW * WAVE)
void gemm_bf16_kernel(const ushort* __restrict__ A,
                      const ushort* __restrict__ B,
                      const ushort* __restrict__ bias,
                      const ushort* __restrict__ residual,
                      ushort* __restrict__ C,
                      int M, int N, int K, int act, float alpha,
                      int64_t strideA, int64_t strideB, int64_t strideC,
                      int n_tiles_m) {
  constexpr int BM_ = WMW * 64, BN_ = WNW * 64;
  constexpr int NW = WMW * WNW;
  constexpr int A_BYTES = BM_ * BK * 2, B_BYTES = BN_ * BK * 2;
  __shared__ __attribute__((aligned(16))) char smem[2 * (A_BYTES + B_BYTES)];
  auto lds_a = [&](int buf) -> char* {
    return smem + buf * (A_BYTES + B_BYTES); };
  auto lds_b = [&](int buf) -> char* {
    return smem + buf * (A_BYTES + B_BYTES) + A_BYTES; };

  const int bat = blockIdx.y;
  const ushort* Ab = A + bat * strideA;
  const ushort* Bb = B + bat * strideB;
  ushort* Cb = C + bat * strideC;

  const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
  const int tile_m = bid % n_tiles_m;
  const int tile_n = bid / n_tiles_m;
  const int m0 = tile_m * BM_;
  const int n0 = tile_n * BN_;

  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int wm = wave / WNW, wn = wave % WNW;

  f32x4_t acc[4][4] = {};

  const int n_ktiles = K / BK;

  // prologue: stage tile 0 into buf 0
  {
    stage_tile_glds<BM_, NW>(Ab, K, M - 1, m0, 0, lds_a(0), wave, lane);
    if (TRANS_B) {
      stage_tile_glds<BN_, NW>(Bb, K, N - 1, n0, 0, lds_b(0), wave, lane);
    } else {
      stage_tile_transposed<BN_, NW>(
          Bb, N, K - 1, n0, 0, reinterpret_cast<ushort*>(lds_b(0)), wave,
          lane, N);
    }
  }

  // 2-phase schedule (T3 minimum form, cdna_hip_programming.md §5.5):
  // one barrier per K-tile; the next tile's staging loads are issued
  // BEFORE this tile's ds_read+MFMA so the glds overlaps the compute.
  // __syncthreads() emits the vmcnt(0) drain for the in-flight glds.
  int cur = 0;
  for (int kt = 0; kt < n_ktiles; ++kt) {
    __syncthreads();
    if (kt + 1 < n_ktiles) {
      int k0 = (kt + 1) * BK;
      stage_tile_glds<BM_, NW>(Ab, K, M - 1, m0, k0, lds_a(cur ^ 1),
                               wave, lane);
      if (TRANS_B) {
        stage_tile_glds<BN_, NW>(Bb, K, N - 1, n0, k0, lds_b(cur ^ 1),
                                 wave, lane);
      } else {
        stage_tile_transposed<BN_, NW>(
            Bb, N, K - 1, n0, k0,
            reinterpret_cast<ushort*>(lds_b(cur ^ 1)), wave, lane, N);
      }
    }

    const char* at = lds_a(cur);
    const char* bt = lds_b(cur);
    const int frow = lane & 15;           // fragment row/col within 16
    const int kgrp = lane >> 4;           // 0..3

    #pragma unroll
    for (int ks = 0; ks < 2; ++ks) {      // two K=32 steps per 64-tile
      bf16x8_t a_frag[4], b_frag[4];
      const int chunk = ks * 4 + kgrp;
      #pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        int row = wm * 64 + mi * 16 + frow;
        a_frag[mi] = *reinterpret_cast<const bf16x8_t*>(
            at + lds_off(row, chunk));
      }
      #pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        int row = wn * 64 + ni * 16 + frow;
        b_frag[ni] = *reinterpret_cast<const bf16x8_t*>(
            bt + lds_off(row, chunk));
      }
      __builtin_amdgcn_s_setprio(1);
      #pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a_frag[mi], b_frag[ni], acc[mi][ni], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    cur ^= 1;
  }

  epilogue_store<HAS_BIAS, HAS_RES>(acc, smem, bias, residual, Cb, M, N,
                                    m0, n0, wave, lane, wm, wn, act,
                                    alpha);
}

template <int WMW, int WNW, bool TRANS_B>
static void gemm_launch_geom(hipStream_t s, const ushort* A,
                             const ushort* B, const ushort* bias,
                             const ushort* residual, ushort* C,
                             int64_t bat, int64_t M, int64_t N, int64_t K,
                             int act, float alpha, int64_t sA, int64_t sB,
                             int64_t sC) {
  int ntm = int(ceil_div(M, WMW * 64)), ntn = int(ceil_div(N, WNW * 64));
  dim3 grid(ntm * ntn, (unsigned)bat);
  dim3 block(WMW * WNW * WAVE);
  bool hb = bias != nullptr, hr = residual != nullptr;
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, block, 0, s, A, B, bias, residual, C,
                       (int)M, (int)N, (int)K, act, alpha, sA, sB, sC, ntm);
  };
  if (hb && hr)  launch(gemm_bf16_kernel<WMW, WNW, TRANS_B, true, true>);
  else if (hb)   launch(gemm_bf16_kernel<WMW, WNW, TRANS_B, true, false>);
  else if (hr)   launch(gemm_bf16_kernel<WMW, WNW, TRANS_B, false, true>);
  else           launch(gemm_bf16_kernel<WMW, WNW, TRANS_B, false, false>);
}

template <bool TRANS_B>
static void gemm_dispatch(hipStream_t s, const ushort* A, const ushort* B,
                          const ushort* bias, const ushort* residual,
                          ushort* C, int64_t bat, int64_t M, int64_t N,
                          int64_t K, int act, float alpha, int64_t sA,
                          int64_t sB, int64_t sC) {
  if (K % BK != 0)
    throw std::runtime_error("gemm: K must be a multiple of 64 (got " +
                             std::to_string(K) + ")");
  // geometry by fill: prefer 128x128 tiles; shrink while the grid
  // under-fills the chip (2 blocks/CU at 64KB LDS -> target >=512,
  // accept >=232 = ~1 block/CU)
  auto blocks = [&](int bm, int bn) {
    return bat * ceil_div(M, bm) * ceil_div(N, bn);
  };
  if (blocks(128, 128) >= 232) {
    gemm_launch_geom<2, 2, TRANS_B>(s, A, B, bias, residual, C, bat, M, N,
                                    K, act, alpha, sA, sB, sC);
  } else if (blocks(64, 128) >= 232) {
    gemm_launch_geom<1, 2, TRANS_B>(s, A, B, bias, residual, C, bat, M, N,
                                    K, act, alpha, sA, sB, sC);
  } else {
    gemm_launch_geom<1, 1, TRANS_B>(s, A, B, bias, residual, C, bat, M, N,
                                    K, act, alpha, sA, sB, sC);
  }
}

void launch_gemm(hipStream_t s, const ushort* A, const ushort* B,
                 const ushort* bias, const ushort* residual, ushort* C,
                 int64_t M, int64_t N, int64_t K, int act, float alpha) {
  gemm_dispatch<true>(s, A, B, bias, residual, C, 1, M, N, K, act, alpha,
                      0, 0, 0);
}

// ---------------------------------------------------------------------------
// Fused implicit-GEMM conv: same 128x128xBK=64 MFMA structure, but the
// A tile is GATHERED from the NHWC input during glds staging — each
// lane's 16-byte chunk maps to 8 contiguous channels of one patch
// element (requires C % 8 == 0 so chunks never straddle an (r,s)
// boundary); out-of-image/-range chunks read from a zeroed buffer so
// the glds issues unconditionally. Removes the im2col memory pass that
// was 43-50% of ResNet-50 kernel time.
// ---------------------------------------------------------------------------
struct ConvGeom {
  int H, W, C, R, S, sh, sw, pt, pl, Ho, Wo, rsc;
};

TFSC_DEV void stage_tile_conv_a(const ushort* __restrict__ x,
                                const ushort* __restrict__ zeros,
                                const ConvGeom g, int M, int m0, int k0,
                                char* lds_tile, int wave, int lane) {
  int r_in = (lane >> 3);
  int chunk = lane & 7;
  #pragma unroll
  for (int i = 0; i < 4; ++i) {
    int row = wave * 32 + i * 8 + r_in;
    int m = m0 + row;
    m = m < M - 1 ? m : M - 1;
    int chunk_src = chunk ^ (row & 7);
    int k = k0 + chunk_src * 8;           // start of the 8-channel chunk
    // decompose m -> (n, ho, wo) and k -> (r, s, c)
    int wo = m % g.Wo;
    int t = m / g.Wo;
    int ho = t % g.Ho;
    int n = t / g.Ho;
    int c = k % g.C;
    int t2 = k / g.C;
    int s = t2 % g.S;
    int r = t2 / g.S;
    int hi = ho * g.sh + r - g.pt;
    int wi = wo * g.sw + s - g.pl;
    bool ok = (k < g.rsc) & (hi >= 0) & (hi < g.H) & (wi >= 0) & (wi < g.W);
    const ushort* gptr = ok
        ? x + (((int64_t)n * g.H + hi) * g.W + wi) * g.C + c
        : zeros;
    char* lds_base = lds_tile + (wave * 32 + i * 8) * 128;
    __builtin_amdgcn_global_load_lds(
        reinterpret_cast<const uint32_t*>(gptr),
        reinterpret_cast<uint32_t*>(lds_base), 16, 0, 0);
  }
}

template <bool HAS_RES>
__global__ __launch_bounds__(THREADS)
void conv_igemm_kernel(const ushort* __restrict__ x,
                       const ushort* __restrict__ B,
                       const ushort* __restrict__ bias,
                       const ushort* __restrict__ residual,
                       const ushort* __restrict__ zeros,
                       ushort* __restrict__ Cout,
                       int M, int N, int K, int act, ConvGeom g,
                       int n_tiles_m) {
  __shared__ __attribute__((aligned(16))) char smem[4 * BM * BK * 2];
  auto lds_a = [&](int buf) -> char* { return smem + buf * 32768; };
  auto lds_b = [&](int buf) -> char* { return smem + 16384 + buf * 32768; };

  const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
  const int tile_m = bid % n_tiles_m;
  const int tile_n = bid / n_tiles_m;
  const int m0 = tile_m * BM;
  const int n0 = tile_n * BN;
  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int wm = wave >> 1, wn = wave & 1;

  f32x4_t acc[4][4] = {};
  const int n_ktiles = K / BK;

  stage_tile_conv_a(x, zeros, g, M, m0, 0, lds_a(0), wave, lane);
  stage_tile_glds<128, 4>(B, K, N - 1, n0, 0, lds_b(0), wave, lane);

  int cur = 0;
  for (int kt = 0; kt < n_ktiles; ++kt) {
    __syncthreads();
    if (kt + 1 < n_ktiles) {
      int k0 = (kt + 1) * BK;
      stage_tile_conv_a(x, zeros, g, M, m0, k0, lds_a(cur ^ 1), wave, lane);
      stage_tile_glds<128, 4>(B, K, N - 1, n0, k0, lds_b(cur ^ 1), wave,
                              lane);
    }
    const char* at = lds_a(cur);
    const char* bt = lds_b(cur);
    const int frow = lane & 15;
    const int kgrp = lane >> 4;
    #pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_t a_frag[4], b_frag[4];
      const int chunk = ks * 4 + kgrp;
      #pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        a_frag[mi] = *reinterpret_cast<const bf16x8_t*>(
            at + lds_off(wm * 64 + mi * 16 + frow, chunk));
      #pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        b_frag[ni] = *reinterpret_cast<const bf16x8_t*>(
            bt + lds_off(wn * 64 + ni * 16 + frow, chunk));
      __builtin_amdgcn_s_setprio(1);
      #pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a_frag[mi], b_frag[ni], acc[mi][ni], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    cur ^= 1;
  }

  epilogue_store<true, HAS_RES>(acc, smem, bias, residual, Cout, M, N,
                                m0, n0, wave, lane, wm, wn, act, 1.0f);
}

// ---------------------------------------------------------------------------
// Grouped implicit-GEMM conv (ResNeXt / RegNet): per group g the GEMM is
//   y[M, g*Ng .. g*Ng+Ng) = x_g[M, pad64(R*S*Cg)] x w[g*Ng .., :]^T
// with x_g the im2col of input channels g*Cg .. g*Cg+Cg. One block owns
// (M tile, N tile inside the group, group). Ng is small (16..64 after
// the planner's merge), so the tile is 128 x (16*NT): the four waves
// stack along M, 32 rows x BN columns each. Same anatomy as the dense
// kernel: 16-byte glds staging with the XOR source swizzle, two LDS
// buffers, one barrier per K tile, 16x16x32 bf16 MFMA, LDS-restaged
// coalesced epilogue. With NT = 1 an A fragment feeds one MFMA, so the
// kernel is gather- and LDS-bound, not MFMA-bound.
// ---------------------------------------------------------------------------
struct GroupedConvGeom {
  int H, W, C, Cg, Ng, R, S, sh, sw, pt, pl, Ho, Wo, rsc;   // rsc = R*S*Cg
};

constexpr int GBM = 128;                  // grouped kernel's M tile

// B tile: rows n0 .. n0+BN_ of group g's filters ([Kc][ld] weight, rows
// g*Ng + n), clamped to the group's last row. BN_/8 glds of 8 rows each,
// dealt round-robin to the four waves (BN_ = 16: waves 0 and 1 only).
template <int BN_>
TFSC_DEV void stage_tile_grouped_b(const ushort* __restrict__ w, int ld,
                                   int row_base, int row_limit, int n0,
                                   int k0, char* lds_tile, int wave,
                                   int lane) {
  int r_in = lane >> 3;
  int chunk = lane & 7;
  #pragma unroll
  for (int i = 0; i < (BN_ / 8 + N_WAVES - 1) / N_WAVES; ++i) {
    int slab = i * N_WAVES + wave;        // wave-uniform
    if (slab * 8 >= BN_) break;
    int row = slab * 8 + r_in;
    int n = n0 + row;
    n = n < row_limit ? n : row_limit;
    int chunk_src = chunk ^ (row & 7);
    const ushort* gptr =
        w + (int64_t)(row_base + n) * ld + k0 + chunk_src * 8;
    __builtin_amdgcn_global_load_lds(
        reinterpret_cast<const uint32_t*>(gptr),
        reinterpret_cast<uint32_t*>(lds_tile + slab * 8 * 128), 16, 0, 0);
  }
}

template <int NT, bool HAS_RES>
__global__ __launch_bounds__(THREADS)
void conv_igemm_grouped_kernel(const ushort* __restrict__ x,
                               const ushort* __restrict__ B,
                               const ushort* __restrict__ bias,
                               const ushort* __restrict__ residual,
                               const ushort* __restrict__ zeros,
                               ushort* __restrict__ y,
                               int M, int Kc, int K, int act,
                               GroupedConvGeom g, int groups, int n_tiles_n) {
  constexpr int BN_ = 16 * NT;
  constexpr int A_BYTES = GBM * BK * 2, B_BYTES = BN_ * BK * 2;
  __shared__ __attribute__((aligned(16))) char smem[2 * (A_BYTES + B_BYTES)];
  auto lds_a = [&](int buf) -> char* {
    return smem + buf * (A_BYTES + B_BYTES); };
  auto lds_b = [&](int buf) -> char* {
    return smem + buf * (A_BYTES + B_BYTES) + A_BYTES; };

  // group fastest: the groups of one M tile read the same pixels (a
  // 128-byte line holds several groups' channels), so they should run
  // together on one XCD's L2
  const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
  const int grp = bid % groups;
  const int t_ = bid / groups;
  const int n0 = (t_ % n_tiles_n) * BN_;  // within the group
  const int m0 = (t_ / n_tiles_n) * GBM;
  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int r_in = lane >> 3;
  const int chunk_src = (lane & 7) ^ r_in;    // row & 7 == r_in

  // the lane's four A rows never change: decompose m -> (n, ho, wo) once
  int hi0[4], wi0[4], nH[4];
  #pragma unroll
  for (int i = 0; i < 4; ++i) {
    int m = m0 + wave * 32 + i * 8 + r_in;
    m = m < M - 1 ? m : M - 1;
    int wo = m % g.Wo;
    int t = m / g.Wo;
    hi0[i] = (t % g.Ho) * g.sh - g.pt;
    wi0[i] = wo * g.sw - g.pl;
    nH[i] = (t / g.Ho) * g.H;
  }
  const ushort* xg = x + grp * g.Cg;

  auto stage_a = [&](int k0, char* lds_tile) {
    int k = k0 + chunk_src * 8;           // start of the 8-channel chunk
    int c = k % g.Cg;
    int t2 = k / g.Cg;
    int s = t2 % g.S;
    int r = t2 / g.S;
    bool k_ok = k < g.rsc;
    #pragma unroll
    for (int i = 0; i < 4; ++i) {
      int hi = hi0[i] + r, wi = wi0[i] + s;
      bool ok = k_ok & (hi >= 0) & (hi < g.H) & (wi >= 0) & (wi < g.W);
      const ushort* gptr = ok
          ? xg + ((int64_t)(nH[i] + hi) * g.W + wi) * g.C + c
          : zeros;
      __builtin_amdgcn_global_load_lds(
          reinterpret_cast<const uint32_t*>(gptr),
          reinterpret_cast<uint32_t*>(lds_tile + (wave * 32 + i * 8) * 128),
          16, 0, 0);
    }
  };

  f32x4_t acc[2][NT] = {};
  const int n_ktiles = K / BK;
  const int row_base = grp * g.Ng;

  stage_a(0, lds_a(0));
  stage_tile_grouped_b<BN_>(B, K, row_base, g.Ng - 1, n0, 0, lds_b(0), wave,
                            lane);

  int cur = 0;
  for (int kt = 0; kt < n_ktiles; ++kt) {
    __syncthreads();
    if (kt + 1 < n_ktiles) {
      int k0 = (kt + 1) * BK;
      stage_a(k0, lds_a(cur ^ 1));
      stage_tile_grouped_b<BN_>(B, K, row_base, g.Ng - 1, n0, k0,
                                lds_b(cur ^ 1), wave, lane);
    }
    const char* at = lds_a(cur);
    const char* bt = lds_b(cur);
    const int frow = lane & 15;
    const int kgrp = lane >> 4;
    #pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_t a_frag[2], b_frag[NT];
      const int chunk = ks * 4 + kgrp;
      #pragma unroll
      for (int mi = 0; mi < 2; ++mi)
        a_frag[mi] = *reinterpret_cast<const bf16x8_t*>(
            at + lds_off(wave * 32 + mi * 16 + frow, chunk));
      #pragma unroll
      for (int ni = 0; ni < NT; ++ni)
        b_frag[ni] = *reinterpret_cast<const bf16x8_t*>(
            bt + lds_off(ni * 16 + frow, chunk));
      __builtin_amdgcn_s_setprio(1);
      #pragma unroll
      for (int mi = 0; mi < 2; ++mi)
        #pragma unroll
        for (int ni = 0; ni < NT; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a_frag[mi], b_frag[ni], acc[mi][ni], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    cur ^= 1;
  }

  // epilogue: each wave restages its 32 x BN_ tile (acc + bias, f32: the
  // narrow tile leaves room, so the result is rounded to bf16 once,
  // after residual and activation) through its own LDS region and
  // streams it out in 16-byte chunks to y[row*Kc + grp*Ng + n0 + col];
  // the column bound is the group's Ng (whole chunks, Ng % 8 == 0), the
  // row bound M
  __syncthreads();              // tiles are dead; reuse as staging
  float* stage = reinterpret_cast<float*>(smem + wave * (32 * BN_ * 4));
  {
    const int col_in = lane & 15;
    const int row_b = (lane >> 4) * 4;
    #pragma unroll
    for (int ni = 0; ni < NT; ++ni) {
      int col = ni * 16 + col_in;
      int nc = n0 + col;
      nc = nc < g.Ng ? nc : g.Ng - 1;
      float bv = bf2f(bias[row_base + nc]);
      #pragma unroll
      for (int mi = 0; mi < 2; ++mi)
        #pragma unroll
        for (int r = 0; r < 4; ++r)
          stage[(mi * 16 + row_b + r) * BN_ + col] = acc[mi][ni][r] + bv;
    }
  }
  __syncthreads();
  constexpr int CPR = BN_ / 8;            // 16-byte chunks per row
  #pragma unroll
  for (int i = 0; i < NT; ++i) {          // 32*CPR chunks = NT x 64 lanes
    int chunk_id = i * 64 + lane;
    int row = chunk_id / CPR;
    int chunk = chunk_id % CPR;
    int grow = m0 + wave * 32 + row;
    int gcol = n0 + chunk * 8;
    if (grow >= M || gcol >= g.Ng) continue;
    const f32x4_t* sp =
        reinterpret_cast<const f32x4_t*>(stage + row * BN_ + chunk * 8);
    f32x4_t lo = sp[0], hi = sp[1];
    int64_t goff = (int64_t)grow * Kc + row_base + gcol;
    bf16x8 rv = {};
    if (HAS_RES) rv = *reinterpret_cast<const bf16x8*>(residual + goff);
    bf16x8 v;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      float xv = j < 4 ? lo[j] : hi[j - 4];
      if (HAS_RES) xv += bf2f((ushort)rv[j]);
      v[j] = (short)f2bf(act_apply(xv, act));
    }
    *reinterpret_cast<bf16x8*>(y + goff) = v;
  }
}

// ---------------------------------------------------------------------------
// Dilated (atrous) implicit-GEMM conv (DeepLab / dilated-ResNet / ASPP):
//   hi = ho*sh - pt + r*dh,  wi = wo*sw - pl + s*dw
// Same anatomy as conv_igemm_kernel (128x128x64 tiles, 16-byte glds
// staging with the XOR source swizzle, two LDS buffers, one barrier per K
// tile, 16x16x32 bf16 MFMA, epilogue_store, XCD swizzle), with the
// m -> (n, ho, wo) decomposition of a lane's four A rows hoisted out of
// the K loop as in the grouped kernel.
//
// Dead-tap skipping (SKIP): at ASPP rates on small maps a whole row or
// column of filter taps lies outside the image for every row of an M
// tile; a dense K loop would stage zeros and run MFMAs on them. With
// C % 64 == 0 a K tile lies inside one tap (r, s), and K = R*S*C has no
// pad tile. The prologue reduces min/max of hi0 and wi0 over the block's
// 128 rows (wave shuffles, then the four waves through LDS: one extra
// barrier), builds a bit mask of the taps that can touch the image for
// some row of the block - conservative: it may keep a dead tap and never
// drops a live one - and the K loop visits live K tiles only; "next tile"
// of the double-buffer pipeline is the next live one. All of it is
// block-uniform scalar code. No live tile at all (huge explicit pads) is
// legal: the accumulators stay zero and the epilogue writes
// act(bias [+ residual]) everywhere. The launcher picks SKIP only when
// C % 64 == 0 and R*S <= 64 (the mask's width).
// ---------------------------------------------------------------------------
// The new float arithmetic below is compiled without packed f32
// instructions (v_pk_add_f32 and kin), as in ops/reduce.hip: the
// extension's flags are shared by every source, so the feature is
// switched off here, for the device pass only, and back on after.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                   \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
struct DilatedConvGeom {
  int H, W, C, R, S, sh, sw, pt, pl, dh, dw, Ho, Wo, rsc;
};

TFSC_DEV int wave_min(int v) {
  #pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    int t = __shfl_xor(v, o, WAVE);
    v = t < v ? t : v;
  }
  return v;
}

TFSC_DEV int wave_max(int v) {
  #pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    int t = __shfl_xor(v, o, WAVE);
    v = t > v ? t : v;
  }
  return v;
}

template <bool HAS_RES, bool SKIP>
__global__ __launch_bounds__(THREADS)
void conv_igemm_dilated_kernel(const ushort* __restrict__ x,
                               const ushort* __restrict__ B,
                               const ushort* __restrict__ bias,
                               const ushort* __restrict__ residual,
                               const ushort* __restrict__ zeros,
                               ushort* __restrict__ Cout,
                               int M, int N, int K, int act,
                               DilatedConvGeom g, int n_tiles_m) {
  __shared__ __attribute__((aligned(16))) char smem[4 * BM * BK * 2];
  auto lds_a = [&](int buf) -> char* { return smem + buf * 32768; };
  auto lds_b = [&](int buf) -> char* { return smem + 16384 + buf * 32768; };

  const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
  const int tile_m = bid % n_tiles_m;
  const int tile_n = bid / n_tiles_m;
  const int m0 = tile_m * BM;
  const int n0 = tile_n * BN;
  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int wm = wave >> 1, wn = wave & 1;
  const int r_in = lane >> 3;
  const int chunk_src = (lane & 7) ^ r_in;    // row & 7 == r_in

  // the lane's four A rows never change: decompose m -> (n, ho, wo) once
  int hi0[4], wi0[4], nH[4];
  #pragma unroll
  for (int i = 0; i < 4; ++i) {
    int m = m0 + wave * 32 + i * 8 + r_in;
    m = m < M - 1 ? m : M - 1;
    int wo = m % g.Wo;
    int t = m / g.Wo;
    hi0[i] = (t % g.Ho) * g.sh - g.pt;
    wi0[i] = wo * g.sw - g.pl;
    nH[i] = (t / g.Ho) * g.H;
  }

  // live-tap mask: bit r*S + s is clear when tap (r, s) is out of the
  // image for every one of the block's rows
  unsigned long long live = ~0ull;
  const int tiles_per_tap = g.C / BK;         // SKIP: C % 64 == 0
  if (SKIP) {
    int lo_h = hi0[0], hi_h = hi0[0], lo_w = wi0[0], hi_w = wi0[0];
    #pragma unroll
    for (int i = 1; i < 4; ++i) {
      lo_h = hi0[i] < lo_h ? hi0[i] : lo_h;
      hi_h = hi0[i] > hi_h ? hi0[i] : hi_h;
      lo_w = wi0[i] < lo_w ? wi0[i] : lo_w;
      hi_w = wi0[i] > hi_w ? wi0[i] : hi_w;
    }
    lo_h = wave_min(lo_h); hi_h = wave_max(hi_h);
    lo_w = wave_min(lo_w); hi_w = wave_max(hi_w);
    // buffer 1 is first written after the K loop's first barrier, so its
    // head is free to carry the four waves' partials until then
    int* red = reinterpret_cast<int*>(lds_a(1));
    if (lane == 0) {
      red[wave * 4 + 0] = lo_h; red[wave * 4 + 1] = hi_h;
      red[wave * 4 + 2] = lo_w; red[wave * 4 + 3] = hi_w;
    }
    __syncthreads();
    #pragma unroll
    for (int w_ = 0; w_ < N_WAVES; ++w_) {
      int a = red[w_ * 4 + 0], b = red[w_ * 4 + 1];
      int c = red[w_ * 4 + 2], d = red[w_ * 4 + 3];
      lo_h = a < lo_h ? a : lo_h; hi_h = b > hi_h ? b : hi_h;
      lo_w = c < lo_w ? c : lo_w; hi_w = d > hi_w ? d : hi_w;
    }
    lo_h = __builtin_amdgcn_readfirstlane(lo_h);
    hi_h = __builtin_amdgcn_readfirstlane(hi_h);
    lo_w = __builtin_amdgcn_readfirstlane(lo_w);
    hi_w = __builtin_amdgcn_readfirstlane(hi_w);
    live = 0;
    for (int r = 0; r < g.R; ++r) {
      bool row_dead = (hi_h + r * g.dh < 0) | (lo_h + r * g.dh >= g.H);
      for (int s = 0; s < g.S; ++s) {
        bool dead = row_dead | (hi_w + s * g.dw < 0) |
                    (lo_w + s * g.dw >= g.W);
        if (!dead) live |= 1ull << (r * g.S + s);
      }
    }
  }

  // The K loop runs over live tiles only. SKIP: `rest` holds the live taps
  // not yet staged, its lowest set bit the tap being staged, `j` the tile
  // inside that tap; the tap's (r*dh, s*dw) are scalars recomputed only
  // when the tap changes, so the per-tile k -> (r, s, c) divisions of the
  // dense kernel go away too. !SKIP: tile i is K tile i.
  const int n_live = SKIP ? __builtin_popcountll(live) * tiles_per_tap
                          : K / BK;
  unsigned long long rest = live;
  int j = 0, tap = 0, dr = 0, ds = 0;
  auto enter_tap = [&]() {
    tap = __builtin_ctzll(rest);
    dr = (tap / g.S) * g.dh;
    ds = (tap % g.S) * g.dw;
  };
  if (SKIP && n_live) enter_tap();

  // stage live tile `i` (SKIP: the tile the cursor stands on, then step)
  auto stage = [&](int i, int buf) {
    int k0, c, r_dh, s_dw;
    bool k_ok = true;
    if (SKIP) {
      k0 = (tap * tiles_per_tap + j) * BK;
      c = j * BK + chunk_src * 8;
      r_dh = dr; s_dw = ds;
      if (++j == tiles_per_tap) {
        j = 0;
        rest &= rest - 1;
        if (rest) enter_tap();
      }
    } else {
      k0 = i * BK;
      int k = k0 + chunk_src * 8;         // start of the 8-channel chunk
      c = k % g.C;
      int t2 = k / g.C;
      s_dw = (t2 % g.S) * g.dw;
      r_dh = (t2 / g.S) * g.dh;
      k_ok = k < g.rsc;
    }
    char* lds_tile = lds_a(buf);
    #pragma unroll
    for (int q = 0; q < 4; ++q) {
      int hi = hi0[q] + r_dh, wi = wi0[q] + s_dw;
      bool ok = k_ok & (hi >= 0) & (hi < g.H) & (wi >= 0) & (wi < g.W);
      const ushort* gptr = ok
          ? x + ((int64_t)(nH[q] + hi) * g.W + wi) * g.C + c
          : zeros;
      __builtin_amdgcn_global_load_lds(
          reinterpret_cast<const uint32_t*>(gptr),
          reinterpret_cast<uint32_t*>(lds_tile + (wave * 32 + q * 8) * 128),
          16, 0, 0);
    }
    stage_tile_glds<128, 4>(B, K, N - 1, n0, k0, lds_b(buf), wave, lane);
  };

  f32x4_t acc[4][4] = {};

  if (n_live) stage(0, 0);

  int cur = 0;
  for (int i = 0; i < n_live; ++i) {
    __syncthreads();
    if (i + 1 < n_live) stage(i + 1, cur ^ 1);
    const char* at = lds_a(cur);
    const char* bt = lds_b(cur);
    const int frow = lane & 15;
    const int kgrp = lane >> 4;
    #pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_t a_frag[4], b_frag[4];
      const int chunk = ks * 4 + kgrp;
      #pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        a_frag[mi] = *reinterpret_cast<const bf16x8_t*>(
            at + lds_off(wm * 64 + mi * 16 + frow, chunk));
      #pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        b_frag[ni] = *reinterpret_cast<const bf16x8_t*>(
            bt + lds_off(wn * 64 + ni * 16 + frow, chunk));
      __builtin_amdgcn_s_setprio(1);
      #pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a_frag[mi], b_frag[ni], acc[mi][ni], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    cur ^= 1;
  }

  epilogue_store<true, HAS_RES>(acc, smem, bias, residual, Cout, M, N,
                                m0, n0, wave, lane, wm, wn, act, 1.0f);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// Dead-tap skipping: 0 never, 1 where it pays (default), 2 wherever the
// kernel can (C % 64 == 0, R*S <= 64). A measurement switch
// (scripts/dilated_conv_probe.py). Measured on an MI355X
// (profiles/dilated_conv.md), the skipping kernel is 12-23% faster than
// the same kernel without it at [8,65,65,512] rates 12-36 and 2-4% slower
// where nothing can be gained: when the grid has at most one block per
// CU, the kernel lasts as long as its slowest block, which sits in the
// middle of the image and skips nothing; and when the dilated filter
// reaches over less than an eighth of the image, hardly a block lies
// wholly in the border where taps die. Mode 1 skips outside those cases.
static int g_dilated_skip = 1;
int conv_dilated_skip() { return g_dilated_skip; }
void set_conv_dilated_skip(int mode) { g_dilated_skip = mode; }

static void conv_dilated_launch(hipStream_t s, const ushort* x,
                                const ushort* w, const ushort* bias,
                                const ushort* residual, const ushort* zeros,
                                ushort* y, int M, int Kc, int k_pad, int act,
                                const DilatedConvGeom& g) {
  int ntm = int(ceil_div(M, BM)), ntn = int(ceil_div(Kc, BN));
  dim3 grid(ntm * ntn);
  bool skip = g_dilated_skip && g.C % BK == 0 && g.R * g.S <= 64;
  if (skip && g_dilated_skip == 1)
    skip = grid.x > 256 && ((g.R - 1) * g.dh * 8 >= g.H ||
                            (g.S - 1) * g.dw * 8 >= g.W);
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(THREADS), 0, s, x, w, bias, residual,
                       zeros, y, M, Kc, k_pad, act, g, ntm);
  };
  if (residual && skip) launch(conv_igemm_dilated_kernel<true, true>);
  else if (residual)    launch(conv_igemm_dilated_kernel<true, false>);
  else if (skip)        launch(conv_igemm_dilated_kernel<false, true>);
  else                  launch(conv_igemm_dilated_kernel<false, false>);
}

template <int NT>
static void conv_grouped_launch(hipStream_t s, const ushort* x,
                                const ushort* w, const ushort* bias,
                                const ushort* residual, const ushort* zeros,
                                ushort* y, int M, int Kc, int k_pad, int act,
                                const GroupedConvGeom& g, int groups) {
  int ntm = int(ceil_div(M, GBM)), ntn = int(ceil_div(g.Ng, 16 * NT));
  dim3 grid(ntm * ntn * groups);
  if (residual)
    hipLaunchKernelGGL((conv_igemm_grouped_kernel<NT, true>), grid,
                       dim3(THREADS), 0, s, x, w, bias, residual, zeros, y,
                       M, Kc, k_pad, act, g, groups, ntn);
  else
    hipLaunchKernelGGL((conv_igemm_grouped_kernel<NT, false>), grid,
                       dim3(THREADS), 0, s, x, w, bias, nullptr, zeros, y,
                       M, Kc, k_pad, act, g, groups, ntn);
}

void launch_conv_igemm(hipStream_t s, const ushort* x, const ushort* w,
                       const ushort* bias, const ushort* residual,
                       const ushort* zeros, ushort* y,
                       int N_img, int H, int W, int C, int Kc, int R,
                       int S, int sh, int sw, int pt, int pl, int Ho,
                       int Wo, int k_pad, int act, int groups, int dh,
                       int dw) {
  if (groups < 1)
    throw std::runtime_error("conv_igemm groups must be >= 1");
  if (dh < 1 || dw < 1)
    throw std::runtime_error("conv_igemm dilation must be >= 1");
  if (dh != 1 || dw != 1) {
    if (groups > 1)
      throw std::runtime_error("dilated grouped conv_igemm unsupported");
    if (C % 8 != 0)
      throw std::runtime_error("dilated conv_igemm requires C % 8 == 0");
    if (k_pad != (R * S * C + BK - 1) / BK * BK)
      throw std::runtime_error(
          "dilated conv_igemm k_pad must be pad64(R*S*C)");
    if ((int64_t)(R - 1) * dh >= (1 << 30) ||
        (int64_t)(S - 1) * dw >= (1 << 30))
      throw std::runtime_error("dilated conv_igemm: filter extent too large");
    DilatedConvGeom g{H, W, C, R, S, sh, sw, pt, pl, dh, dw, Ho, Wo,
                      R * S * C};
    conv_dilated_launch(s, x, w, bias, residual, zeros, y, N_img * Ho * Wo,
                        Kc, k_pad, act, g);
    return;
  }
  if (groups > 1) {
    if (C % groups != 0 || Kc % groups != 0)
      throw std::runtime_error(
          "grouped conv_igemm: groups must divide C and Kc");
    int Cg = C / groups, Ng = Kc / groups;
    if (Cg % 8 != 0 || Ng % 8 != 0)
      throw std::runtime_error(
          "grouped conv_igemm requires (C/groups) % 8 == 0 and "
          "(Kc/groups) % 8 == 0");
    if (k_pad != (R * S * Cg + BK - 1) / BK * BK)
      throw std::runtime_error(
          "grouped conv_igemm k_pad must be pad64(R*S*C/groups)");
    GroupedConvGeom g{H, W, C, Cg, Ng, R, S, sh, sw, pt, pl, Ho, Wo,
                      R * S * Cg};
    int M = N_img * Ho * Wo;
    // narrowest N tile that covers the group; Ng > 64 takes several
    if (Ng <= 16)
      conv_grouped_launch<1>(s, x, w, bias, residual, zeros, y, M, Kc,
                             k_pad, act, g, groups);
    else if (Ng <= 32)
      conv_grouped_launch<2>(s, x, w, bias, residual, zeros, y, M, Kc,
                             k_pad, act, g, groups);
    else
      conv_grouped_launch<4>(s, x, w, bias, residual, zeros, y, M, Kc,
                             k_pad, act, g, groups);
    return;
  }
  if (C % 8 != 0)
    throw std::runtime_error("conv_igemm requires C % 8 == 0");
  if (k_pad % BK != 0)
    throw std::runtime_error("conv_igemm k_pad must be 64-aligned");
  ConvGeom g{H, W, C, R, S, sh, sw, pt, pl, Ho, Wo, R * S * C};
  int M = N_img * Ho * Wo;
  int ntm = int(ceil_div(M, BM)), ntn = int(ceil_div(Kc, BN));
  dim3 grid(ntm * ntn);
  if (residual)
    hipLaunchKernelGGL((conv_igemm_kernel<true>), grid, dim3(THREADS), 0,
                       s, x, w, bias, residual, zeros, y, M, Kc, k_pad,
                       act, g, ntm);
  else
    hipLaunchKernelGGL((conv_igemm_kernel<false>), grid, dim3(THREADS), 0,
                       s, x, w, bias, nullptr, zeros, y, M, Kc, k_pad,
                       act, g, ntm);
}

// ---------------------------------------------------------------------------
// 3-D implicit-GEMM conv (C3D / I3D / R(2+1)D video nets, 3-D U-Net):
//   M = N*Do*Ho*Wo,  N = Kc,  K = pad64(T*R*S*C),  k = ((t*R + r)*S + s)*C + c
//   di = do*sd - pf + t,  hi = ho*sh - pt + r,  wi = wo*sw - pl + s
// Same anatomy as conv_igemm_kernel (128x128x64 tiles, four waves, 16-byte
// glds staging with the XOR source swizzle, two LDS buffers, one barrier
// per K tile, 16x16x32 bf16 MFMA inside s_setprio, an LDS-restaged
// coalesced epilogue (epilogue_store_f32 below), XCD swizzle). The A
// gather over three spatial axes has no division in the K loop:
//  - rows: a lane stages the same four A rows in every K tile, so
//    m -> (n, do, ho, wo) is decomposed once. A row keeps the corner of
//    its receptive field (di0, hi0, wi0) and `org`, the 64-bit element
//    offset of that corner in x (it may lie in the padding and be
//    negative; it is only ever added to an in-volume tap).
//  - k: a lane's 8-channel chunk advances by exactly 64 in k per tile, so
//    its (t, r, s, c) is a cursor advanced by add-and-carry. `koff`, the
//    chunk's element offset from a row's corner, ((t*H + r)*W + s)*C + c,
//    is the same for every row; it moves by 64 per tile plus a jump of
//    (W - S)*C when s wraps into r and (H - R)*W*C when r wraps into t.
//    A chunk's address is org + koff: one 64-bit add per row.
//  - TAP_UNIFORM (C % 64 == 0): a K tile lies inside one tap, so
//    (t, r, s), the tile's channel base and koff are block-uniform and
//    live in scalar registers; the lane adds its chunk's 8*chunk_src. K
//    has no pad tile then.
// Chunks outside the volume, and the k >= T*R*S*C tail (t >= T), read the
// zero page, so the four glds of a tile issue unconditionally.
// ---------------------------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                   \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
struct Conv3dGeom {
  int D, H, W, C, T, R, S, sd, sh, sw, pf, pt, pl, Do, Ho, Wo;
};

// epilogue_store rounds acc + bias to bf16 in its staging tile and rounds
// again after the residual add and the activation: with a residual the
// error reaches two bf16 roundings of the pre-residual value, which can
// exceed 2^-8 * max|y|. This variant of it rounds once. The 128x128 tile's
// four waves restage their 64x64 tiles as f32 - 16 KB each, exactly the
// 64 KB of tile buffers, dead by now - and the stream-out pass (the same
// 16-byte lanes, residual read coalesced) adds the residual, applies the
// activation and rounds.
template <bool HAS_RES>
TFSC_DEV void epilogue_store_f32(f32x4_t (&acc)[4][4], char* smem,
                                 const ushort* __restrict__ bias,
                                 const ushort* __restrict__ residual,
                                 ushort* __restrict__ Cb,
                                 int M, int N, int m0, int n0, int wave,
                                 int lane, int wm, int wn, int act) {
  __syncthreads();              // tiles are dead; reuse as staging
  float* stage = reinterpret_cast<float*>(smem + wave * 16384);
  const int col_in = lane & 15;
  const int row_base = (lane >> 4) * 4;
  #pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    #pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      int col = ni * 16 + col_in;
      float bv = bf2f(bias[n0 + wn * 64 + col]);
      #pragma unroll
      for (int r = 0; r < 4; ++r)
        stage[(mi * 16 + row_base + r) * 64 + col] = acc[mi][ni][r] + bv;
    }
  }
  __syncthreads();
  #pragma unroll
  for (int i = 0; i < 8; ++i) {
    int chunk_id = i * 64 + lane;
    int row = chunk_id >> 3;
    int chunk = chunk_id & 7;
    int grow = m0 + wm * 64 + row;
    int gcol0 = n0 + wn * 64 + chunk * 8;
    if (grow >= M) continue;
    const f32x4_t* sp =
        reinterpret_cast<const f32x4_t*>(stage + row * 64 + chunk * 8);
    f32x4_t lo = sp[0], hi = sp[1];
    float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    int64_t goff = (int64_t)grow * N + gcol0;
    const bool full = gcol0 + 7 < N;
    if (HAS_RES) {
      if (full) {
        bf16x8 rv = *reinterpret_cast<const bf16x8*>(residual + goff);
        #pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += bf2f((ushort)rv[j]);
      } else {
        for (int j = 0; j < 8 && gcol0 + j < N; ++j)
          v[j] += bf2f(residual[goff + j]);
      }
    }
    bf16x8 o;
    #pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (short)f2bf(act_apply(v[j], act));
    if (full) {
      *reinterpret_cast<bf16x8*>(Cb + goff) = o;
    } else {
      for (int j = 0; j < 8 && gcol0 + j < N; ++j)
        Cb[goff + j] = (ushort)o[j];
    }
  }
}

template <bool HAS_RES, bool TAP_UNIFORM>
__global__ __launch_bounds__(THREADS)
void conv3d_igemm_kernel(const ushort* __restrict__ x,
                         const ushort* __restrict__ B,
                         const ushort* __restrict__ bias,
                         const ushort* __restrict__ residual,
                         const ushort* __restrict__ zeros,
                         ushort* __restrict__ Cout,
                         int M, int N, int K, int act, Conv3dGeom g,
                         int n_tiles_m) {
  __shared__ __attribute__((aligned(16))) char smem[4 * BM * BK * 2];
  auto lds_a = [&](int buf) -> char* { return smem + buf * 32768; };
  auto lds_b = [&](int buf) -> char* { return smem + 16384 + buf * 32768; };

  const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
  const int tile_m = bid % n_tiles_m;
  const int tile_n = bid / n_tiles_m;
  const int m0 = tile_m * BM;
  const int n0 = tile_n * BN;
  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int wm = wave >> 1, wn = wave & 1;
  const int r_in = lane >> 3;
  const int chunk_src = (lane & 7) ^ r_in;    // row & 7 == r_in

  // the lane's four A rows: receptive-field corner and its offset in x
  int di0[4], hi0[4], wi0[4];
  int64_t org[4];
  #pragma unroll
  for (int i = 0; i < 4; ++i) {
    int m = m0 + wave * 32 + i * 8 + r_in;
    m = m < M - 1 ? m : M - 1;
    int wo = m % g.Wo;
    int q = m / g.Wo;
    int ho = q % g.Ho;
    q /= g.Ho;
    int n = q / g.Do;
    di0[i] = (q % g.Do) * g.sd - g.pf;
    hi0[i] = ho * g.sh - g.pt;
    wi0[i] = wo * g.sw - g.pl;
    org[i] = ((((int64_t)n * g.D + di0[i]) * g.H + hi0[i]) * g.W + wi0[i]) *
             g.C;
  }

  // the k cursor: tap (kt, kr, ks) and channel kc of the lane's chunk
  // (TAP_UNIFORM: of the tile's first chunk), koff as above
  int kt = 0, kr = 0, ks = 0, kc = 0;
  if (!TAP_UNIFORM) {
    int k = chunk_src * 8;
    kc = k % g.C;
    int q = k / g.C;
    ks = q % g.S;
    q /= g.S;
    kr = q % g.R;
    kt = q / g.R;
  }
  int64_t koff = (((int64_t)kt * g.H + kr) * g.W + ks) * g.C + kc;
  const int64_t r_jump = (int64_t)(g.W - g.S) * g.C;
  const int64_t t_jump = (int64_t)(g.H - g.R) * g.W * g.C;

  // stage the K tile the cursor stands on (k0 is its first k), then step
  auto stage = [&](int k0, int buf) {
    const int64_t off = TAP_UNIFORM ? koff + chunk_src * 8 : koff;
    const bool k_ok = TAP_UNIFORM || kt < g.T;
    char* lds_tile = lds_a(buf);
    #pragma unroll
    for (int q = 0; q < 4; ++q) {
      unsigned di = unsigned(di0[q] + kt);    // negative wraps above D
      unsigned hi = unsigned(hi0[q] + kr);
      unsigned wi = unsigned(wi0[q] + ks);
      bool ok = k_ok & (di < unsigned(g.D)) & (hi < unsigned(g.H)) &
                (wi < unsigned(g.W));
      const ushort* gptr = ok ? x + (org[q] + off) : zeros;
      __builtin_amdgcn_global_load_lds(
          reinterpret_cast<const uint32_t*>(gptr),
          reinterpret_cast<uint32_t*>(lds_tile + (wave * 32 + q * 8) * 128),
          16, 0, 0);
    }
    stage_tile_glds<128, 4>(B, K, N - 1, n0, k0, lds_b(buf), wave, lane);
    kc += BK;
    koff += BK;
    while (kc >= g.C) {                       // C >= 64: at most once
      kc -= g.C;
      if (++ks == g.S) {
        ks = 0;
        koff += r_jump;
        if (++kr == g.R) {
          kr = 0;
          koff += t_jump;
          ++kt;
        }
      }
    }
  };

  f32x4_t acc[4][4] = {};
  const int n_ktiles = K / BK;

  stage(0, 0);

  int cur = 0;
  for (int i = 0; i < n_ktiles; ++i) {
    __syncthreads();
    if (i + 1 < n_ktiles) stage((i + 1) * BK, cur ^ 1);
    const char* at = lds_a(cur);
    const char* bt = lds_b(cur);
    const int frow = lane & 15;
    const int kgrp = lane >> 4;
    #pragma unroll
    for (int kstep = 0; kstep < 2; ++kstep) {
      bf16x8_t a_frag[4], b_frag[4];
      const int chunk = kstep * 4 + kgrp;
      #pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        a_frag[mi] = *reinterpret_cast<const bf16x8_t*>(
            at + lds_off(wm * 64 + mi * 16 + frow, chunk));
      #pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        b_frag[ni] = *reinterpret_cast<const bf16x8_t*>(
            bt + lds_off(wn * 64 + ni * 16 + frow, chunk));
      __builtin_amdgcn_s_setprio(1);
      #pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a_frag[mi], b_frag[ni], acc[mi][ni], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    cur ^= 1;
  }

  epilogue_store_f32<HAS_RES>(acc, smem, bias, residual, Cout, M, N, m0, n0,
                              wave, lane, wm, wn, act);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

void launch_conv3d_igemm(hipStream_t s, const ushort* x, const ushort* w,
                         const ushort* bias, const ushort* residual,
                         const ushort* zeros, ushort* y,
                         int N_img, int D, int H, int W, int C, int Kc,
                         int T, int R, int S, int sd, int sh, int sw,
                         int pf, int pt, int pl, int Do, int Ho, int Wo,
                         int k_pad, int act, int groups, int dh, int dw) {
  if (groups != 1)
    throw std::runtime_error("grouped conv3d_igemm unsupported");
  if (dh != 1 || dw != 1)
    throw std::runtime_error("dilated conv3d_igemm unsupported");
  if (D < 1 || T < 1 || sd < 1 || Do < 1)
    throw std::runtime_error("conv3d_igemm: D, T, sd and Do must be >= 1");
  if (N_img < 1 || H < 1 || W < 1 || C < 1 || Kc < 1 || R < 1 || S < 1 ||
      sh < 1 || sw < 1 || Ho < 1 || Wo < 1)
    throw std::runtime_error(
        "conv3d_igemm: every extent and stride must be >= 1");
  if (C % 8 != 0)
    throw std::runtime_error("conv3d_igemm requires C % 8 == 0");
  int64_t trsc = (int64_t)T * R * S * C;
  if (trsc > INT32_MAX - BK || k_pad != (trsc + BK - 1) / BK * BK)
    throw std::runtime_error("conv3d_igemm k_pad must be pad64(T*R*S*C)");
  int64_t M = (int64_t)N_img * Do * Ho * Wo;
  if (M > INT32_MAX - BM)
    throw std::runtime_error("conv3d_igemm: more than 2^31 output voxels");
  Conv3dGeom g{D, H, W, C, T, R, S, sd, sh, sw, pf, pt, pl, Do, Ho, Wo};
  int ntm = int(ceil_div(M, BM)), ntn = int(ceil_div(Kc, BN));
  dim3 grid(ntm * ntn);
  bool uni = C % BK == 0;
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(THREADS), 0, s, x, w, bias, residual,
                       zeros, y, int(M), Kc, k_pad, act, g, ntm);
  };
  if (residual && uni) launch(conv3d_igemm_kernel<true, true>);
  else if (residual)   launch(conv3d_igemm_kernel<true, false>);
  else if (uni)        launch(conv3d_igemm_kernel<false, true>);
  else                 launch(conv3d_igemm_kernel<false, false>);
}

// ---------------------------------------------------------------------------
// 3-D transposed conv (Conv3DBackpropInputV2; 3-D U-Net / V-Net decoders),
// phase-split ("sub-pixel") implicit GEMM, one launch:
//   y[n,od,oh,ow,co] = sum x[n,i,j,l,ci] * w[t,r,s,co,ci],  od = i*sd - pf + t
// Per axis an output coordinate od has phase pd = (od + pf) mod sd and only
// meets taps t = pd + sd*a, a in [0, A(pd)), A(pd) = ceil((T - pd)/sd) (0
// when pd >= T), at input i = q - a with q = (od + pf) div sd. So each of
// the sd*sh*sw phases is a stride-1 conv over the un-dilated x with an
// A x B x Cc sub-filter that writes one strided sub-lattice of y; no tap
// multiplies an inserted zero.
//  - grid: phases x M tiles x N tiles. A block decodes (pd, ph, pw) from
//    its id and derives, per axis, A, the phase's first q (q0), its count
//    of q (Q) and the taps of the phases before it, all block-uniform
//    (phase_axis below; no device-side table). M_phase = N*Qd*Qh*Qw; Q
//    differs by at most 1 between phases, the M-tile count is sized by the
//    largest and a block with m0 >= M_phase returns before any barrier.
//  - weights: [Kc][k_pad], taps phase-major ((pd,ph,pw) row-major), inside
//    a phase in (a',b',c') order with a' = A-1-a (reversed), k = (taps
//    before + (a'*B + b')*Cc + c')*C + ci. Reversed taps make the cursor
//    walk forward through x from the corner (qd-(A-1), qh-(B-1),
//    qw-(Cc-1)): conv3d_igemm_kernel's org + koff gather with (T,R,S)
//    replaced by (A,B,Cc), TAP_UNIFORM included.
//  - a phase's k range starts at a multiple of C, not of 64: with
//    C % 64 != 0 its last K tile runs past its last tap. A reads the zero
//    page there (a' >= A), so whatever finite weights B holds there do not
//    count, but the tile must lie inside the row: the row carries all-zero
//    taps after the real ones until it does (conv3d_transpose_taps).
//  - a phase with no tap (filter smaller than the stride) has zero K
//    tiles: nothing is staged and the epilogue writes act(bias [+ res]).
//  - epilogue: epilogue_store_f32's staging with the global row offset
//    replaced by the voxel's, (((n*Do + od)*Ho + oh)*Wo + ow)*Kc, for the
//    store and the residual read alike.
// ---------------------------------------------------------------------------
struct Conv3dTGeom {
  int N, D, H, W, C, T, R, S, sd, sh, sw, pf, pt, pl, Do, Ho, Wo, ntm, ntn;
};

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                   \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
// one axis of a phase: taps A, first q, count of q, taps of earlier phases
struct PhaseAxis {
  int A, q0, Q, pref;
};

__host__ __device__ inline PhaseAxis phase_axis(int p, int T, int s, int pad,
                                                int out) {
  PhaseAxis a;
  a.A = p < T ? (T - p + s - 1) / s : 0;
  a.q0 = p >= pad ? 0 : (pad - p + s - 1) / s;
  int last = out - 1 + pad - p;           // largest od + pad - p
  a.Q = last < 0 ? 0 : last / s - a.q0 + 1;
  a.Q = a.Q < 0 ? 0 : a.Q;
  a.pref = (T / s) * p + (T % s < p ? T % s : p);   // |{t < T: t mod s < p}|
  return a;
}

// epilogue_store_f32 with the output row scattered: row_off(grow) is the
// element offset of row grow's Kc contiguous channels in y and residual
template <bool HAS_RES, class RowOff>
TFSC_DEV void epilogue_scatter_f32(f32x4_t (&acc)[4][4], char* smem,
                                   const ushort* __restrict__ bias,
                                   const ushort* __restrict__ residual,
                                   ushort* __restrict__ Cb, RowOff row_off,
                                   int M, int N, int m0, int n0, int wave,
                                   int lane, int wm, int wn, int act) {
  __syncthreads();              // tiles are dead; reuse as staging
  float* stage = reinterpret_cast<float*>(smem + wave * 16384);
  const int col_in = lane & 15;
  const int row_base = (lane >> 4) * 4;
  #pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    #pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      int col = ni * 16 + col_in;
      float bv = bf2f(bias[n0 + wn * 64 + col]);
      #pragma unroll
      for (int r = 0; r < 4; ++r)
        stage[(mi * 16 + row_base + r) * 64 + col] = acc[mi][ni][r] + bv;
    }
  }
  __syncthreads();
  #pragma unroll
  for (int i = 0; i < 8; ++i) {
    int chunk_id = i * 64 + lane;
    int row = chunk_id >> 3;
    int chunk = chunk_id & 7;
    int grow = m0 + wm * 64 + row;
    int gcol0 = n0 + wn * 64 + chunk * 8;
    if (grow >= M || gcol0 >= N) continue;
    const f32x4_t* sp =
        reinterpret_cast<const f32x4_t*>(stage + row * 64 + chunk * 8);
    f32x4_t lo = sp[0], hi = sp[1];
    float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    int64_t goff = row_off(grow) + gcol0;
    const bool full = gcol0 + 7 < N;
    if (HAS_RES) {
      if (full) {
        bf16x8 rv = *reinterpret_cast<const bf16x8*>(residual + goff);
        #pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += bf2f((ushort)rv[j]);
      } else {
        for (int j = 0; j < 8 && gcol0 + j < N; ++j)
          v[j] += bf2f(residual[goff + j]);
      }
    }
    bf16x8 o;
    #pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (short)f2bf(act_apply(v[j], act));
    if (full) {
      *reinterpret_cast<bf16x8*>(Cb + goff) = o;
    } else {
      for (int j = 0; j < 8 && gcol0 + j < N; ++j)
        Cb[goff + j] = (ushort)o[j];
    }
  }
}

template <bool HAS_RES, bool TAP_UNIFORM>
__global__ __launch_bounds__(THREADS)
void conv3d_transpose_igemm_kernel(const ushort* __restrict__ x,
                                   const ushort* __restrict__ B,
                                   const ushort* __restrict__ bias,
                                   const ushort* __restrict__ residual,
                                   const ushort* __restrict__ zeros,
                                   ushort* __restrict__ Cout,
                                   int N, int K, int act, Conv3dTGeom g) {
  __shared__ __attribute__((aligned(16))) char smem[4 * BM * BK * 2];
  auto lds_a = [&](int buf) -> char* { return smem + buf * 32768; };
  auto lds_b = [&](int buf) -> char* { return smem + 16384 + buf * 32768; };

  // block -> (phase, N tile, M tile), M fastest; all of it block-uniform
  const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
  const int tile_m = bid % g.ntm;
  int rest = bid / g.ntm;
  const int tile_n = rest % g.ntn;
  rest /= g.ntn;
  const int pw = rest % g.sw;
  rest /= g.sw;
  const int ph = rest % g.sh;
  const int pd = rest / g.sh;
  const PhaseAxis ad = phase_axis(pd, g.T, g.sd, g.pf, g.Do);
  const PhaseAxis ah = phase_axis(ph, g.R, g.sh, g.pt, g.Ho);
  const PhaseAxis aw = phase_axis(pw, g.S, g.sw, g.pl, g.Wo);
  const int M = g.N * ad.Q * ah.Q * aw.Q;     // the launcher bounds it
  const int m0 = tile_m * BM;
  if (m0 >= M) return;                        // before the first barrier
  const int n0 = tile_n * BN;
  const int n_taps = ad.A * ah.A * aw.A;
  const int n_ktiles = (n_taps * g.C + BK - 1) / BK;
  const int k_base =
      (ad.pref * g.R * g.S + ad.A * (ah.pref * g.S + ah.A * aw.pref)) * g.C;

  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int wm = wave >> 1, wn = wave & 1;
  const int r_in = lane >> 3;
  const int chunk_src = (lane & 7) ^ r_in;    // row & 7 == r_in

  // the lane's four A rows: m -> (n, qd, qh, qw), the corner
  // (qd-(A-1), qh-(B-1), qw-(Cc-1)) of the sub-filter's reach and its
  // offset in x (negative in the padding; only added to in-volume taps)
  int di0[4], hi0[4], wi0[4];
  int64_t org[4];
  if (n_ktiles > 0) {
    #pragma unroll
    for (int i = 0; i < 4; ++i) {
      int m = m0 + wave * 32 + i * 8 + r_in;
      m = m < M - 1 ? m : M - 1;
      int jw = m % aw.Q;
      int q = m / aw.Q;
      int jh = q % ah.Q;
      q /= ah.Q;
      int n = q / ad.Q;
      di0[i] = ad.q0 + q % ad.Q - (ad.A - 1);
      hi0[i] = ah.q0 + jh - (ah.A - 1);
      wi0[i] = aw.q0 + jw - (aw.A - 1);
      org[i] = ((((int64_t)n * g.D + di0[i]) * g.H + hi0[i]) * g.W + wi0[i]) *
               g.C;
    }
  }

  // the k cursor inside the phase: reversed tap (kt, kr, ks) = (a', b', c')
  // and channel kc of the lane's chunk (TAP_UNIFORM: of the tile's first
  // chunk); koff = ((kt*H + kr)*W + ks)*C + kc, the chunk's offset from a
  // row's corner
  int kt = 0, kr = 0, ks = 0, kc = 0;
  if (!TAP_UNIFORM && n_ktiles > 0) {
    int k = chunk_src * 8;
    kc = k % g.C;
    int q = k / g.C;
    ks = q % aw.A;
    q /= aw.A;
    kr = q % ah.A;
    kt = q / ah.A;
  }
  int64_t koff = (((int64_t)kt * g.H + kr) * g.W + ks) * g.C + kc;
  const int64_t r_jump = (int64_t)(g.W - aw.A) * g.C;
  const int64_t t_jump = (int64_t)(g.H - ah.A) * g.W * g.C;

  // stage the K tile the cursor stands on (k0 is its first k in the
  // phase), then step
  auto stage = [&](int k0, int buf) {
    const int64_t off = TAP_UNIFORM ? koff + chunk_src * 8 : koff;
    const bool k_ok = TAP_UNIFORM || kt < ad.A;
    char* lds_tile = lds_a(buf);
    #pragma unroll
    for (int q = 0; q < 4; ++q) {
      unsigned di = unsigned(di0[q] + kt);    // negative wraps above D
      unsigned hi = unsigned(hi0[q] + kr);
      unsigned wi = unsigned(wi0[q] + ks);
      bool ok = k_ok & (di < unsigned(g.D)) & (hi < unsigned(g.H)) &
                (wi < unsigned(g.W));
      const ushort* gptr = ok ? x + (org[q] + off) : zeros;
      __builtin_amdgcn_global_load_lds(
          reinterpret_cast<const uint32_t*>(gptr),
          reinterpret_cast<uint32_t*>(lds_tile + (wave * 32 + q * 8) * 128),
          16, 0, 0);
    }
    stage_tile_glds<128, 4>(B, K, N - 1, n0, k_base + k0, lds_b(buf), wave,
                            lane);
    kc += BK;
    koff += BK;
    while (kc >= g.C) {                       // C >= 64: at most once
      kc -= g.C;
      if (++ks == aw.A) {
        ks = 0;
        koff += r_jump;
        if (++kr == ah.A) {
          kr = 0;
          koff += t_jump;
          ++kt;
        }
      }
    }
  };

  f32x4_t acc[4][4] = {};

  if (n_ktiles > 0) stage(0, 0);

  int cur = 0;
  for (int i = 0; i < n_ktiles; ++i) {
    __syncthreads();
    if (i + 1 < n_ktiles) stage((i + 1) * BK, cur ^ 1);
    const char* at = lds_a(cur);
    const char* bt = lds_b(cur);
    const int frow = lane & 15;
    const int kgrp = lane >> 4;
    #pragma unroll
    for (int kstep = 0; kstep < 2; ++kstep) {
      bf16x8_t a_frag[4], b_frag[4];
      const int chunk = kstep * 4 + kgrp;
      #pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        a_frag[mi] = *reinterpret_cast<const bf16x8_t*>(
            at + lds_off(wm * 64 + mi * 16 + frow, chunk));
      #pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        b_frag[ni] = *reinterpret_cast<const bf16x8_t*>(
            bt + lds_off(wn * 64 + ni * 16 + frow, chunk));
      __builtin_amdgcn_s_setprio(1);
      #pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a_frag[mi], b_frag[ni], acc[mi][ni], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    cur ^= 1;
  }

  // row of the phase -> its voxel of y: od = qd*sd + pd - pf, likewise h, w
  auto row_off = [&](int m) -> int64_t {
    int jw = m % aw.Q;
    int q = m / aw.Q;
    int jh = q % ah.Q;
    q /= ah.Q;
    int n = q / ad.Q;
    int od = (ad.q0 + q % ad.Q) * g.sd + pd - g.pf;
    int oh = (ah.q0 + jh) * g.sh + ph - g.pt;
    int ow = (aw.q0 + jw) * g.sw + pw - g.pl;
    return ((((int64_t)n * g.Do + od) * g.Ho + oh) * g.Wo + ow) * N;
  };
  epilogue_scatter_f32<HAS_RES>(acc, smem, bias, residual, Cout, row_off, M,
                                N, m0, n0, wave, lane, wm, wn, act);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// taps of the weight row: T*R*S real ones, then zero taps until the last K
// tile of every non-empty phase ends inside the row
static int64_t conv3d_transpose_taps(int C, int T, int R, int S, int sd,
                                     int sh, int sw) {
  int64_t need = 0;
  for (int pd = 0; pd < sd && pd < T; ++pd)
    for (int ph = 0; ph < sh && ph < R; ++ph)
      for (int pw = 0; pw < sw && pw < S; ++pw) {
        PhaseAxis a = phase_axis(pd, T, sd, 0, 1);   // A and pref only
        PhaseAxis b = phase_axis(ph, R, sh, 0, 1);
        PhaseAxis c = phase_axis(pw, S, sw, 0, 1);
        int64_t before = (int64_t)a.pref * R * S +
                         (int64_t)a.A * (b.pref * S + b.A * c.pref);
        int64_t kp = (int64_t)a.A * b.A * c.A * C;
        int64_t end = before * C + (kp + BK - 1) / BK * BK;
        need = end > need ? end : need;
      }
  return (need + C - 1) / C;
}

void launch_conv3d_transpose_igemm(hipStream_t s, const ushort* x,
                                   const ushort* w, const ushort* bias,
                                   const ushort* residual,
                                   const ushort* zeros, ushort* y,
                                   int N_img, int D, int H, int W, int C,
                                   int Kc, int T, int R, int S, int sd,
                                   int sh, int sw, int pf, int pt, int pl,
                                   int Do, int Ho, int Wo, int k_pad,
                                   int act) {
  if (N_img < 1 || D < 1 || H < 1 || W < 1 || C < 1 || Kc < 1 || T < 1 ||
      R < 1 || S < 1 || sd < 1 || sh < 1 || sw < 1 || Do < 1 || Ho < 1 ||
      Wo < 1)
    throw std::runtime_error(
        "conv3d_transpose_igemm: every extent and stride must be >= 1");
  if (pf < 0 || pt < 0 || pl < 0)
    throw std::runtime_error("conv3d_transpose_igemm: negative pad");
  if (C % 8 != 0)
    throw std::runtime_error("conv3d_transpose_igemm requires C % 8 == 0");
  if ((int64_t)T * R * S * C > INT32_MAX / 4)
    throw std::runtime_error("conv3d_transpose_igemm: T*R*S*C beyond int32");
  // the weight row: see conv3d_transpose_taps
  int64_t row = conv3d_transpose_taps(C, T, R, S, sd, sh, sw) * C;
  if (k_pad != (row + BK - 1) / BK * BK)
    throw std::runtime_error(
        "conv3d_transpose_igemm k_pad must be pad64(taps * C), taps being "
        "T*R*S plus the zero taps that keep every phase's last K tile in "
        "the row");
  // the largest phase: the per-axis maxima of Q
  int64_t qmax[3] = {0, 0, 0};
  for (int p = 0; p < sd; ++p)
    qmax[0] = std::max<int64_t>(qmax[0], phase_axis(p, T, sd, pf, Do).Q);
  for (int p = 0; p < sh; ++p)
    qmax[1] = std::max<int64_t>(qmax[1], phase_axis(p, R, sh, pt, Ho).Q);
  for (int p = 0; p < sw; ++p)
    qmax[2] = std::max<int64_t>(qmax[2], phase_axis(p, S, sw, pl, Wo).Q);
  int64_t M = N_img * qmax[0] * qmax[1] * qmax[2];
  if (M > INT32_MAX - BM || (int64_t)N_img * Do * Ho * Wo > INT32_MAX - BM)
    throw std::runtime_error(
        "conv3d_transpose_igemm: more than 2^31 output voxels");
  int ntm = int(ceil_div(M, BM)), ntn = int(ceil_div(Kc, BN));
  int64_t blocks = (int64_t)sd * sh * sw * ntm * ntn;
  if (blocks > INT32_MAX)
    throw std::runtime_error("conv3d_transpose_igemm: grid beyond int32");
  Conv3dTGeom g{N_img, D, H, W, C, T, R, S, sd, sh, sw, pf, pt, pl,
                Do, Ho, Wo, ntm, ntn};
  dim3 grid((unsigned)blocks);
  bool uni = C % BK == 0;
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(THREADS), 0, s, x, w, bias, residual,
                       zeros, y, Kc, k_pad, act, g);
  };
  if (residual && uni) launch(conv3d_transpose_igemm_kernel<true, true>);
  else if (residual)   launch(conv3d_transpose_igemm_kernel<true, false>);
  else if (uni)        launch(conv3d_transpose_igemm_kernel<false, true>);
  else                 launch(conv3d_transpose_igemm_kernel<false, false>);
}

void launch_batched_gemm(hipStream_t s, const ushort* A, const ushort* B,
                         ushort* C, int64_t bat, int64_t M, int64_t N,
                         int64_t K, int64_t strideA, int64_t strideB,
                         int64_t strideC, bool trans_b, float alpha) {
  if (trans_b)
    gemm_dispatch<true>(s, A, B, nullptr, nullptr, C, bat, M, N, K,
                        ACT_NONE, alpha, strideA, strideB, strideC);
  else
    gemm_dispatch<false>(s, A, B, nullptr, nullptr, C, bat, M, N, K,
                         ACT_NONE, alpha, strideA, strideB, strideC);
}

}  // namespace tfsc
