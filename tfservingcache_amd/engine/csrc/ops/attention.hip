// Fused multi-head attention (flash-style, online softmax) for gfx950.
//
//   out[b,s,h,:] = softmax(scale * Q[b,s,h,:] . K[b,:,h,:]^T) @ V[b,:,h,:]
//
// Consumes Q/K/V in their NATURAL layout [B*S, H*D] (the output of the
// QKV projection GEMMs) and writes out in the same layout — replacing
// the unfused plan (4 transposes + 2 batched GEMMs + standalone softmax
// per layer, ~31% of BERT kernel time) with ONE kernel and no S x S
// score materialization.
//
// Geometry: one workgroup (4 waves) per (b, h, 64-row q-block). Q block
// kept in registers (2 A-fragments per wave). Round-2 revision (the
// round-1 kernel measured 11% MFMA-busy / 44% wave-parked — barrier-
// and staging-latency bound): kv tiles are processed TWO per barrier
// from a 4-deep LDS ring (K and V^T 4 x 8 KB each), so each
// __syncthreads covers 128 kv columns of MFMA work and the online
// softmax runs once per 128 columns instead of per 64; the P bounce
// region overlaps the (dead after the prologue) Q tile. 80 KB LDS ->
// 2 workgroups/CU.
//
// The head dim HD is a template parameter: 64 (BERT-base class) or 128
// (decoder-style heads); the planner keeps the unfused path otherwise.
// HD=128 doubles the row of the Q and K tiles (256 B, 16 chunks: the
// P-bounce image), the rows of the V^T tile (128), the K=32 steps of
// QK^T (4) and the O fragments (8); a kv tile is 32 KB instead of 16,
// the Q tile exactly fills the 16 KB Q/P overlay. Its RING=2 variant
// (80 KB, 2 workgroups/CU) serves every S: past one tile pair it
// restages the two slots between pairs instead of prefetching into a
// second pair of slots (a ring of 4 is 144 KB, one workgroup/CU).
//
// Optional additive bias (HAS_BIAS): the attention-mask term real
// exports add to the scaled scores before the softmax,
//
//   score[b,h,q,kv] = scale * q.k + bias[b*sb + h*sh + q*sq + kv]
//
// bf16, strides in elements, stride 0 = broadcast: [B,1,1,S] key
// padding (sb=S), [1,1,S,S] causal constant (sq=S), [B,1,S,S],
// [B,H,S,S]. The bias is read straight from global memory into the
// score-fragment lanes (kv column = lane&15, q rows = (lane>>4)*4+r)
// BEFORE the QK^T MFMA block so the load latency hides under it; no
// LDS. Indices are clamped to S-1 on both axes, so no read leaves the
// operand. -inf entries behave exactly like absent keys; a row with
// every key at -inf yields zeros. The HAS_BIAS=false instantiations are
// the unmasked kernels, unchanged.
#include "../common.h"
#include "../kernels.h"

#include <climits>
#include <stdexcept>
#include <string>

namespace tfsc {

namespace attn {

using bf16x8_t = __attribute__((ext_vector_type(8))) __bf16;
using f32x4_t = __attribute__((ext_vector_type(4))) float;
using ushort2_t = __attribute__((ext_vector_type(2))) ushort;

constexpr int QBLK = 64;       // q rows per workgroup (16 per wave)
constexpr int KVBLK = 64;      // kv rows per staged tile
constexpr int NW = 4;          // waves
constexpr int THREADS = NW * WAVE;
// kv-tile slots of the HD=128 geometry: 2 (80 KB, 2 WG/CU, restage
// between pairs) measured 63.7 us against 92.8 us for 4 (144 KB, 1
// WG/CU, pair prefetch) at B=16, H=8, S=512; equal at S=128
// (profiles/attention_hd128.md)
constexpr int RING_HD128 = 2;

// shared 64x64 bf16 tile image with the gemm.hip chunk-XOR swizzle
TFSC_DEV int t_off(int row, int chunk) {
  return row * 128 + ((chunk ^ (row & 7)) << 4);
}

// [16][128] bf16 image (P bounce): row stride 256 B, 16 chunks
TFSC_DEV int p_off(int row, int chunk) {
  return row * 256 + ((chunk ^ (row & 7)) << 4);
}

// Q / K tile image [64][HD]: t_off rows for HD=64, p_off rows for 128
template <int HD>
TFSC_DEV int qk_off(int row, int chunk) {
  return HD == 64 ? t_off(row, chunk) : p_off(row, chunk);
}

// stage a [64][HD] tile from rows of a [rows_total, H*D] matrix
// (row = s index, stride ld elements, cols = one head's D slice); one
// wave instruction fills 1 KB of LDS = 8 rows (HD=64) or 4 (HD=128)
template <int HD>
TFSC_DEV void stage_rows_glds(const ushort* __restrict__ src, int64_t ld,
                              int row0, int row_limit, char* lds_tile,
                              int wave, int lane) {
  constexpr int LPR = HD / 8;          // lanes (16 B chunks) per row
  constexpr int RPI = WAVE / LPR;      // rows per instruction
  int r_in = lane / LPR, chunk = lane % LPR;
  #pragma unroll
  for (int i = 0; i < 16 / RPI; ++i) {
    int row = wave * 16 + i * RPI + r_in;
    int grow = row0 + row;
    grow = grow < row_limit ? grow : row_limit;
    int chunk_src = chunk ^ (row & 7);
    const ushort* gptr = src + (int64_t)grow * ld + chunk_src * 8;
    char* lds_base = lds_tile + (wave * 16 + i * RPI) * (HD * 2);
    __builtin_amdgcn_global_load_lds(
        reinterpret_cast<const uint32_t*>(gptr),
        reinterpret_cast<uint32_t*>(lds_base), 16, 0, 0);
  }
}

// stage V^T: [d][kv] image from V rows [kv, H*D] (one vectorized 16 B
// global read per group, 8 scattered 2 B LDS writes)
TFSC_DEV void stage_vt(const ushort* __restrict__ src, int64_t ld,
                       int row0, int row_limit, ushort* lds_tile,
                       int wave, int lane) {
  int tid = wave * WAVE + lane;
  #pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    int idx = pass * THREADS + tid;       // 512 groups: kv(64) x dgrp(8)
    int kv = idx >> 3;
    int dg = idx & 7;
    int gkv = row0 + kv;
    gkv = gkv < row_limit ? gkv : row_limit;
    const ushort* gptr = src + (int64_t)gkv * ld + dg * 8;
    short8_t v = *reinterpret_cast<const short8_t*>(gptr);
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      int d = dg * 8 + j;
      int byte_off = t_off(d, kv >> 3) + (kv & 7) * 2;
      *reinterpret_cast<ushort*>(
          reinterpret_cast<char*>(lds_tile) + byte_off) = ushort(v[j]);
    }
  }
}

// stage V^T for HD=128: [128 d][64 kv] image (128 t_off rows) from V
// rows [kv, H*D]. A thread takes two adjacent kv rows of one 8-wide d
// group (two 16 B global reads) and writes 8 dwords, each the (kv,
// kv+1) pair of one d row: half the LDS writes of the 2-byte scatter.
// A wave covers 32 kv x 4 d groups per pass (64 B contiguous per row).
TFSC_DEV void stage_vt128(const ushort* __restrict__ src, int64_t ld,
                          int row0, int row_limit, char* lds_tile,
                          int wave, int lane) {
  int kv = (wave & 1) * 32 + (lane >> 2) * 2;       // even, 0..62
  int gkv0 = row0 + kv, gkv1 = row0 + kv + 1;
  gkv0 = gkv0 < row_limit ? gkv0 : row_limit;
  gkv1 = gkv1 < row_limit ? gkv1 : row_limit;
  #pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    int dg = (pass * 2 + (wave >> 1)) * 4 + (lane & 3);   // 0..15
    short8_t v0 = *reinterpret_cast<const short8_t*>(
        src + (int64_t)gkv0 * ld + dg * 8);
    short8_t v1 = *reinterpret_cast<const short8_t*>(
        src + (int64_t)gkv1 * ld + dg * 8);
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      int d = dg * 8 + j;
      int byte_off = t_off(d, kv >> 3) + (kv & 7) * 2;
      *reinterpret_cast<uint32_t*>(lds_tile + byte_off) =
          uint32_t(ushort(v0[j])) | (uint32_t(ushort(v1[j])) << 16);
    }
  }
}

template <int HD>
TFSC_DEV void stage_vt_hd(const ushort* __restrict__ src, int64_t ld,
                          int row0, int row_limit, char* lds_tile,
                          int wave, int lane) {
  if constexpr (HD == 64)
    stage_vt(src, ld, row0, row_limit,
             reinterpret_cast<ushort*>(lds_tile), wave, lane);
  else
    stage_vt128(src, ld, row0, row_limit, lds_tile, wave, lane);
}

// RING = staged kv-tile slots: 4 (pair prefetch, 80 KB LDS, 2 WG/CU)
// for long sequences; 2 (no prefetch needed when n_kv <= 2, 48 KB LDS,
// 3 WG/CU) for the S <= 128 serving shapes. HD=128 launches RING_HD128
// = 2 for every S (80 KB, 2 WG/CU), restaging its two slots between
// pairs when n_kv > 2; its RING=4 form (144 KB) prefetches like HD=64.
template <int HD, int RING, bool HAS_BIAS>
__global__ __launch_bounds__(THREADS)
void attention_kernel(const ushort* __restrict__ Q,
                      const ushort* __restrict__ K,
                      const ushort* __restrict__ V,
                      ushort* __restrict__ O,
                      int B, int S, int H, float scale, int n_qblk,
                      const ushort* __restrict__ bias, int64_t bias_sb,
                      int64_t bias_sh, int bias_sq) {
  static_assert(HD == 64 || HD == 128, "head dim geometries");
  constexpr int D = HD;
  constexpr int TILE = KVBLK * HD * 2;   // one K or V^T tile: 8 / 16 KB
  // LDS: K ring RINGxTILE | V^T ring RINGxTILE | q/p overlay 16 KB
  // (q tile uses the first 64*HD*2 B until its registers are loaded;
  // the per-wave [16][128] P bounce then reuses the whole 16 KB)
  __shared__ __attribute__((aligned(16))) char smem[TILE * 2 * RING + 16384];
  auto k_lds = [&](int buf) -> char* { return smem + buf * TILE; };
  auto vt_lds = [&](int buf) -> char* {
    return smem + RING * TILE + buf * TILE;
  };
  char* q_lds = smem + 2 * RING * TILE;
  char* p_lds = smem + 2 * RING * TILE;  // 4 waves x 4 KB (after Q)

  const int flat = blockIdx.x;
  const int qb = flat % n_qblk;
  const int h = (flat / n_qblk) % H;
  const int b = flat / (n_qblk * H);
  const int64_t ld = (int64_t)H * D;
  const ushort* Qb = Q + (int64_t)b * S * ld + h * D;
  const ushort* Kb = K + (int64_t)b * S * ld + h * D;
  const ushort* Vb = V + (int64_t)b * S * ld + h * D;
  ushort* Ob = O + (int64_t)b * S * ld + h * D;

  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int frow = lane & 15;
  const int kgrp = lane >> 4;
  const int q0 = qb * QBLK;

  // ---- stage Q AND the first kv tile pair concurrently (disjoint
  // LDS; one barrier covers all five tiles), then pull this wave's 16
  // q rows into registers
  stage_rows_glds<HD>(Qb, ld, q0, S - 1, q_lds, wave, lane);
  stage_rows_glds<HD>(Kb, ld, 0, S - 1, k_lds(0), wave, lane);
  stage_vt_hd<HD>(Vb, ld, 0, S - 1, vt_lds(0), wave, lane);
  stage_rows_glds<HD>(Kb, ld, KVBLK, S - 1, k_lds(1), wave, lane);
  stage_vt_hd<HD>(Vb, ld, KVBLK, S - 1, vt_lds(1), wave, lane);
  __syncthreads();
  bf16x8_t qf[D / 32];  // A-fragments for the K=32 steps over D
  #pragma unroll
  for (int ks = 0; ks < D / 32; ++ks) {
    int row = wave * 16 + frow;
    qf[ks] = *reinterpret_cast<const bf16x8_t*>(
        q_lds + qk_off<HD>(row, ks * 4 + kgrp));
  }
  __syncthreads();   // q_lds consumed; the region becomes the P bounce

  // ---- online softmax state: this lane covers rows wave*16 + kgrp*4+r
  // With a bias a whole tile pair of a row can sit at -inf (masked
  // keys) or -3.0e38 (kv tail); the running max then starts ABOVE the
  // tail sentinel so those columns exponentiate to 0, not exp(0).
  float m_run[4], l_run[4];
  f32x4_t o_acc[D / 16] = {}; // O fragments over d (16 cols each)
  #pragma unroll
  for (int r = 0; r < 4; ++r) {
    m_run[r] = HAS_BIAS ? -1.0e38f : -3.0e38f;
    l_run[r] = 0.f;
  }

  // bias rows of this lane: q rows past S clamp to S-1 (the epilogue
  // drops them); a 0 stride reads the one broadcast row
  // (32-bit unsigned byte offsets from the wave-uniform (b, h) plane:
  // one VGPR per address; the launcher bounds the plane to 2^31)
  const char* bias_bh = nullptr;
  uint32_t bias_roff[4] = {};
  if (HAS_BIAS) {
    bias_bh = reinterpret_cast<const char*>(
        bias + (int64_t)b * bias_sb + (int64_t)h * bias_sh);
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      int qrow = q0 + wave * 16 + kgrp * 4 + r;
      qrow = qrow < S ? qrow : S - 1;
      bias_roff[r] = uint32_t(qrow) * uint32_t(bias_sq) * 2u;
    }
  }

  const int n_kv = (S + KVBLK - 1) / KVBLK;
  const int n_pair = (n_kv + 1) / 2;

  for (int t = 0; t < n_pair; ++t) {
    // pair 0 was staged with Q (covered by the prologue barriers); a
    // barrier here covers the pair t prefetch issued in iteration t-1
    if (t > 0) __syncthreads();
    if (HD == 128 && RING < 4 && t > 0) {
      // ring of 2 past the first pair: every wave is done with pair
      // t-1 (barrier above); restage both slots, then a second barrier
      stage_rows_glds<HD>(Kb, ld, 2 * t * KVBLK, S - 1, k_lds(0), wave,
                          lane);
      stage_vt_hd<HD>(Vb, ld, 2 * t * KVBLK, S - 1, vt_lds(0), wave, lane);
      stage_rows_glds<HD>(Kb, ld, (2 * t + 1) * KVBLK, S - 1, k_lds(1),
                          wave, lane);
      stage_vt_hd<HD>(Vb, ld, (2 * t + 1) * KVBLK, S - 1, vt_lds(1), wave,
                      lane);
      __syncthreads();
    }
    const int base = RING >= 4 ? (t & 1) * 2 : 0;  // slots of this pair
    const int kv_base = t * 2 * KVBLK;
    // bias for this lane's 8 kv columns x 4 q rows, issued ahead of
    // the MFMA block so the latency hides under it — and ahead of the
    // next pair's prefetch: vector loads retire in order, so behind it
    // the first use of the bias would wait for the prefetch too. kv
    // columns past S clamp to S-1 (masked below). A per-key bias
    // (sq == 0) is one load per column, shared by the lane's 4 q rows;
    // a per-query bias is 32. Columns ni and ni+4 share a register as
    // two bf16 halves: 16 VGPRs, not 32, keeps the S <= 128 variant at
    // 3 workgroups per CU. The sq branch is wave-uniform.
    ushort2_t bv[4][4] = {};
    if (HAS_BIAS) {
      uint32_t off[8];
      #pragma unroll
      for (int ni = 0; ni < 8; ++ni) {
        int kv_col = kv_base + ni * 16 + frow;
        off[ni] = uint32_t(kv_col < S ? kv_col : S - 1) * 2u;
      }
      if (bias_sq == 0) {
        ushort bk[8];
        #pragma unroll
        for (int ni = 0; ni < 8; ++ni)
          bk[ni] = *reinterpret_cast<const ushort*>(bias_bh + off[ni]);
        #pragma unroll
        for (int ni = 0; ni < 8; ++ni)
          #pragma unroll
          for (int r = 0; r < 4; ++r) bv[ni & 3][r][ni >> 2] = bk[ni];
      } else {
        #pragma unroll
        for (int ni = 0; ni < 8; ++ni)
          #pragma unroll
          for (int r = 0; r < 4; ++r)
            bv[ni & 3][r][ni >> 2] = *reinterpret_cast<const ushort*>(
                bias_bh + (bias_roff[r] + off[ni]));
      }
    }
    if (RING >= 4 && t + 1 < n_pair) {
      const int nb = ((t + 1) & 1) * 2;
      stage_rows_glds<HD>(Kb, ld, (2 * t + 2) * KVBLK, S - 1, k_lds(nb),
                          wave, lane);
      stage_vt_hd<HD>(Vb, ld, (2 * t + 2) * KVBLK, S - 1, vt_lds(nb), wave,
                      lane);
      stage_rows_glds<HD>(Kb, ld, (2 * t + 3) * KVBLK, S - 1,
                          k_lds(nb + 1), wave, lane);
      stage_vt_hd<HD>(Vb, ld, (2 * t + 3) * KVBLK, S - 1, vt_lds(nb + 1),
                      wave, lane);
    }

    // ---- QK^T: scores[16 q rows][128 kv] = 8 x 1x4 fragments
    f32x4_t sc[8] = {};
    #pragma unroll
    for (int half = 0; half < 2; ++half) {
      const char* kt = k_lds(base + half);
      #pragma unroll
      for (int ks = 0; ks < D / 32; ++ks) {
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
          bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(
              kt + qk_off<HD>(ni * 16 + frow, ks * 4 + kgrp));
          sc[half * 4 + ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              qf[ks], kf, sc[half * 4 + ni], 0, 0, 0);
        }
      }
    }
    // scale (+ bias) + mask the kv tail
    #pragma unroll
    for (int ni = 0; ni < 8; ++ni) {
      int kv_col = kv_base + ni * 16 + frow;   // this lane's kv column
      bool valid = kv_col < S;
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = sc[ni][r] * scale;
        if (HAS_BIAS) v += bf2f(bv[ni & 3][r][ni >> 2]);
        sc[ni][r] = valid ? v : -3.0e38f;
      }
    }

    // ---- per-row max over the 128 kv columns (one pass per pair)
    float pmax[4];
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = sc[0][r];
      #pragma unroll
      for (int ni = 1; ni < 8; ++ni) v = fmaxf(v, sc[ni][r]);
      #pragma unroll
      for (int off = 8; off > 0; off >>= 1)
        v = fmaxf(v, __shfl_xor(v, off, 16));
      pmax[r] = v;
    }
    // online update
    float alpha[4];
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      float m_new = fmaxf(m_run[r], pmax[r]);
      alpha[r] = __expf(m_run[r] - m_new);
      m_run[r] = m_new;
    }
    // exponentiate P and row-sum
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      float sum = 0.f;
      #pragma unroll
      for (int ni = 0; ni < 8; ++ni) {
        sc[ni][r] = __expf(sc[ni][r] - m_run[r]);
        sum += sc[ni][r];
      }
      #pragma unroll
      for (int off = 8; off > 0; off >>= 1)
        sum += __shfl_xor(sum, off, 16);
      l_run[r] = l_run[r] * alpha[r] + sum;
    }
    // rescale O by alpha (rows of O fragments match reg index)
    #pragma unroll
    for (int ni = 0; ni < D / 16; ++ni)
      #pragma unroll
      for (int r = 0; r < 4; ++r)
        o_acc[ni][r] *= alpha[r];

    // ---- P (C-layout) -> LDS [16][128] -> A-fragment layout
    {
      ushort* pw = reinterpret_cast<ushort*>(p_lds + wave * 4096);
      #pragma unroll
      for (int ni = 0; ni < 8; ++ni) {
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          int row = kgrp * 4 + r;            // 0..15
          int col = ni * 16 + frow;          // 0..127
          *reinterpret_cast<ushort*>(
              reinterpret_cast<char*>(pw) + p_off(row, col >> 3) +
              (col & 7) * 2) = f2bf(sc[ni][r]);
        }
      }
      // wave-local write->read; compiler orders via lgkmcnt
      const char* pr = reinterpret_cast<const char*>(pw);
      #pragma unroll
      for (int ks = 0; ks < 4; ++ks) {       // contraction over 128 kv
        bf16x8_t pf = *reinterpret_cast<const bf16x8_t*>(
            pr + p_off(frow, ks * 4 + kgrp));
        const char* vt = vt_lds(base + (ks >> 1));
        int ksub = ks & 1;
        #pragma unroll
        for (int ni = 0; ni < D / 16; ++ni) {
          bf16x8_t vf = *reinterpret_cast<const bf16x8_t*>(
              vt + t_off(ni * 16 + frow, ksub * 4 + kgrp));
          o_acc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              pf, vf, o_acc[ni], 0, 0, 0);
        }
      }
    }
  }

  // ---- epilogue: O /= l, store rows q0 + wave*16 + kgrp*4 + r
  #pragma unroll
  for (int r = 0; r < 4; ++r) {
    int row = q0 + wave * 16 + kgrp * 4 + r;
    if (row >= S) continue;
    float inv = l_run[r] > 0.f ? 1.f / l_run[r] : 0.f;
    ushort* orow = Ob + (int64_t)row * ld;
    #pragma unroll
    for (int ni = 0; ni < D / 16; ++ni)
      orow[ni * 16 + frow] = f2bf(o_acc[ni][r] * inv);
  }
}

}  // namespace attn

template <int HD, int RING>
static void launch_geometry(hipStream_t s, dim3 grid, const ushort* Q,
                            const ushort* K, const ushort* V, ushort* O,
                            int B, int S, int H, float scale, int n_qblk,
                            const ushort* bias, int64_t bias_sb,
                            int64_t bias_sh, int bias_sq) {
  dim3 block(attn::THREADS);
  if (!bias)
    // unmasked models: the same instantiations as ever
    hipLaunchKernelGGL((attn::attention_kernel<HD, RING, false>), grid,
                       block, 0, s, Q, K, V, O, B, S, H, scale, n_qblk,
                       nullptr, 0, 0, 0);
  else
    hipLaunchKernelGGL((attn::attention_kernel<HD, RING, true>), grid,
                       block, 0, s, Q, K, V, O, B, S, H, scale, n_qblk,
                       bias, bias_sb, bias_sh, bias_sq);
}

void launch_attention(hipStream_t s, const ushort* Q, const ushort* K,
                      const ushort* V, ushort* O, int B, int S, int H,
                      int D_, float scale, const ushort* bias,
                      int64_t bias_sb, int64_t bias_sh, int64_t bias_sq) {
  if (D_ != 64 && D_ != 128)
    throw std::runtime_error(
        "fused attention requires head_dim 64 or 128, got " +
        std::to_string(D_));
  // the kernel indexes one (b, h) bias plane with 32-bit offsets
  if (bias && (bias_sb < 0 || bias_sh < 0 || bias_sq < 0 ||
               (int64_t)(S - 1) * bias_sq + S > INT32_MAX))
    throw std::runtime_error("fused attention: bad bias strides");
  int n_qblk = (S + attn::QBLK - 1) / attn::QBLK;
  dim3 grid(B * H * n_qblk);
  const int sq = int(bias_sq);
  if (D_ == 128)
    launch_geometry<128, attn::RING_HD128>(s, grid, Q, K, V, O, B, S, H, scale, n_qblk,
                            bias, bias_sb, bias_sh, sq);
  else if (S <= 2 * attn::KVBLK)
    launch_geometry<64, 2>(s, grid, Q, K, V, O, B, S, H, scale, n_qblk,
                           bias, bias_sb, bias_sh, sq);
  else
    launch_geometry<64, 4>(s, grid, Q, K, V, O, B, S, H, scale, n_qblk,
                           bias, bias_sb, bias_sh, sq);
}

}  // namespace tfsc
