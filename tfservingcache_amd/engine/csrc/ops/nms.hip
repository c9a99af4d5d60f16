// Batched per-class non-max suppression (TF CombinedNonMaxSuppression) for
// gfx950: bf16 boxes [B,N,q,4] (q = 1 or C, rows y1,x1,y2,x2) and bf16
// scores, class-major [B,C,N].
//
//   k_nms_select  one 256-thread workgroup per (image, class) runs the
//                 greedy loop and writes the class's P kept boxes, in the
//                 order kept, to cls_score / cls_idx [B, C*P] (unused
//                 slots -inf / 0). The best max_total of those C*P slots
//                 are then picked by the top-k kernels (ops/topk.hip).
//   k_nms_gather  one thread per output row (b, m) turns a top-k result
//                 (slot, value) back into box, score and class, and one
//                 ballot count per image gives valid_detections.
//
// A candidate travels as the 64-bit composite of ops/topk.hip,
//     key << 48 | ~index << 16 | raw bits
// whose plain descending order is "higher score, then lower box index";
// composite 0 is "none". A round of the greedy loop is one pass over the
// live candidates: every thread kills those of its share whose IoU with
// the box kept in the round before exceeds the threshold and keeps the
// largest surviving composite, with its box; a DPP reduction in each wave
// and a four-entry LDS exchange make the round's winner known to all
// threads. The exchange carries the winner's box and is double-buffered,
// so a round costs one barrier. The winner is written to slot r, marked
// dead by its owner and suppresses in round r + 1. P rounds cost P * n
// IoUs; the n^2 / 2 bitmask method is worse for P << n, the usual case.
//
// Two geometries behind one uniform branch, by the number of candidates
// (score > score_threshold) the first pass over the class's row finds:
//   resident  at most nms_lds_candidates() of them: the first pass has
//             compacted composite (8 B) and box (8 B) of each into LDS and
//             every round runs out of LDS. 4096 candidates are 64 KB of the
//             CU's 160 KB: two workgroups per CU.
//   streamed  more: an alive bit per box lives in LDS (64 KB at N = 2^19),
//             one byte per 8 boxes, and every round re-reads the scores of
//             bytes with a live bit (one 16-byte load) and the boxes from
//             L2.
// The row is addressed in a frame that starts at the 16-byte boundary at
// or below its first score, so every 8-score vector is one aligned load;
// the first and last vector are read element by element under a mask.
//
// IoU is TF's CPU formula in f32: corners min/max-normalised, a box of
// area <= 0 has IoU 0 with everything, inter / (a_i + a_j - inter) with a
// correctly rounded division and no contraction.
#include "../common.h"
#include "../kernels.h"

#include <map>
#include <mutex>
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

constexpr int NMS_TPB = 256;
constexpr int NMS_WAVES = NMS_TPB / WAVE;
constexpr int NMS_MAX_BLOCKS = 2048;
constexpr int NMS_MAX_N = 1 << 19;       // the alive mask's 64 KB
constexpr int NMS_LDS_MAX = 8192;        // largest settable cap: 128 KB
constexpr int NMS_HEADER = 256;          // exchange + counter, bytes
constexpr uint32_t BF16_NEG_INF = 0xff80u;
constexpr uint32_t BF16_NAN = 0x7fc0u;

// candidates up to this many run out of LDS (measured, profiles/nms.md);
// scripts/nms_probe.py moves it to time both sides
int g_lds_candidates = 4096;

struct alignas(8) Box2 { uint32_t yx1, yx2; };   // bf16 y1 | x1 << 16, ...
struct alignas(16) Vec8 { uint32_t w[4]; };      // 8 bf16 scores
struct alignas(16) Exch { uint64_t comp; Box2 box; };

// Functions of the HIP headers keep the packed-f32 feature and would be
// called, not inlined, from this file's functions: the hot loops use
// builtins only (see ops/lstm.hip).
TFSC_DEV void block_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

TFSC_DEV float bf_f32(uint32_t raw) {
  return __builtin_bit_cast(float, raw << 16);
}

TFSC_DEV uint32_t key_of(uint32_t b) {
  if (b == 0x8000u) b = 0;
  return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}

TFSC_DEV uint64_t composite(uint32_t raw, uint32_t index) {
  return (uint64_t(key_of(raw)) << 48) | (uint64_t(~index) << 16) | raw;
}

TFSC_DEV uint32_t comp_index(uint64_t c) { return ~uint32_t(c >> 16); }

TFSC_DEV uint32_t elem(const Vec8& r, int j) {
  return (r.w[j >> 1] >> ((j & 1) * 16)) & 0xffffu;
}

// one class's scores of one image, in the aligned frame
struct ScoreRow {
  const ushort* base;   // frame origin, 16-byte aligned
  int shift;            // frame position of the row's first score
  int n;

  TFSC_DEV int vectors() const { return (shift + n + 7) / 8; }

  // vector v of the frame; positions outside the row read as NaN, which
  // is never a candidate
  TFSC_DEV Vec8 raw8(int v) const {
    const int q0 = v * 8;
    if (q0 >= shift && q0 + 8 <= shift + n)
      return *reinterpret_cast<const Vec8*>(base + q0);
    Vec8 r;
    #pragma unroll
    for (int j = 0; j < 4; ++j) r.w[j] = BF16_NAN | (BF16_NAN << 16);
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int q = q0 + j;
      if (q >= shift && q < shift + n) {
        const int sh = (j & 1) * 16;
        r.w[j >> 1] = (r.w[j >> 1] & ~(0xffffu << sh)) |
                      (uint32_t(base[q]) << sh);
      }
    }
    return r;
  }
};

// bit j: score j of the vector is a candidate (NaN fails the comparison)
TFSC_DEV uint32_t candidates(const Vec8& r, float score_thr) {
  uint32_t m = 0;
  #pragma unroll
  for (int j = 0; j < 8; ++j)
    if (bf_f32(elem(r, j)) > score_thr) m |= 1u << j;
  return m;
}

struct Corners { float y0, x0, y1, x1, area; };

TFSC_DEV Corners corners(Box2 b) {
  #pragma clang fp contract(off)
  const float ya = bf_f32(b.yx1 & 0xffffu), xa = bf_f32(b.yx1 >> 16);
  const float yb = bf_f32(b.yx2 & 0xffffu), xb = bf_f32(b.yx2 >> 16);
  Corners c;
  c.y0 = yb < ya ? yb : ya;
  c.y1 = ya < yb ? yb : ya;
  c.x0 = xb < xa ? xb : xa;
  c.x1 = xa < xb ? xb : xa;
  c.area = (c.y1 - c.y0) * (c.x1 - c.x0);
  return c;
}

// IoU(kept box s, box b) > thr. An empty intersection is IoU 0 without
// the division: both areas are positive there, so the quotient is 0 too.
TFSC_DEV bool suppressed(const Corners& s, Box2 b, float thr) {
  #pragma clang fp contract(off)
  const Corners c = corners(b);
  float iou = 0.f;
  if (s.area > 0.f && c.area > 0.f) {
    const float iy0 = s.y0 < c.y0 ? c.y0 : s.y0;
    const float ix0 = s.x0 < c.x0 ? c.x0 : s.x0;
    const float iy1 = c.y1 < s.y1 ? c.y1 : s.y1;
    const float ix1 = c.x1 < s.x1 ? c.x1 : s.x1;
    const float ih = iy1 - iy0, iw = ix1 - ix0;
    if (ih > 0.f && iw > 0.f) {
      const float inter = ih * iw;
      iou = inter / (s.area + c.area - inter);
    }
  }
  return iou > thr;
}

// max(v, the lane that DPP control CTRL pairs this lane with)
template <int CTRL>
TFSC_DEV uint64_t dpp_max(uint64_t v) {
  const int lo = __builtin_amdgcn_update_dpp(0, int(uint32_t(v)), CTRL, 0xf,
                                             0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, int(uint32_t(v >> 32)), CTRL,
                                             0xf, 0xf, true);
  const uint64_t o = (uint64_t(uint32_t(hi)) << 32) | uint32_t(lo);
  return o > v ? o : v;
}

// the wave's largest v, in every lane: xor 1, xor 2, half-row mirror and
// row mirror leave each row of 16 lanes holding its maximum; the four row
// values are read as scalars
TFSC_DEV uint64_t wave_max(uint64_t v) {
  v = dpp_max<0xB1>(v);      // quad_perm [1,0,3,2]
  v = dpp_max<0x4E>(v);      // quad_perm [2,3,0,1]
  v = dpp_max<0x141>(v);     // row_half_mirror
  v = dpp_max<0x140>(v);     // row_mirror
  uint64_t best = 0;
  #pragma unroll
  for (int row = 0; row < WAVE / 16; ++row) {
    const uint32_t lo = uint32_t(
        __builtin_amdgcn_readlane(int(uint32_t(v)), row * 16));
    const uint32_t hi = uint32_t(
        __builtin_amdgcn_readlane(int(uint32_t(v >> 32)), row * 16));
    const uint64_t o = (uint64_t(hi) << 32) | lo;
    best = o > best ? o : best;
  }
  return best;
}

struct NmsArgs {
  const ushort* scores;     // [B*C, N] class-major
  const Box2* boxes;        // [B, N, q]
  ushort* cls_score;        // [B*C, P]
  int* cls_idx;             // [B*C, P]
  int64_t rows;             // B * C
  int N, C, q, P, cap;
  float iou_thr, score_thr;
};

__global__ __launch_bounds__(NMS_TPB)
void k_nms_select(NmsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  Exch* exch = reinterpret_cast<Exch*>(lds);                 // [2][WAVES]
  uint32_t* count = reinterpret_cast<uint32_t*>(lds + 2 * NMS_WAVES *
                                                sizeof(Exch));
  uint64_t* comp_s = reinterpret_cast<uint64_t*>(lds + NMS_HEADER);
  Box2* box_s = reinterpret_cast<Box2*>(lds + NMS_HEADER +
                                        size_t(a.cap) * 8);
  unsigned char* alive = lds + NMS_HEADER;
  const int t = threadIdx.x, lane = t % WAVE, wv = t / WAVE;
  const int64_t step = gridDim.x;

  for (int64_t w = blockIdx.x; w < a.rows; w += step) {
    const int64_t b = w / a.C;
    const int c = int(w % a.C);
    const ushort* first = a.scores + w * a.N;
    const int shift = int((reinterpret_cast<uintptr_t>(first) & 15) / 2);
    const ScoreRow row{first - shift, shift, a.N};
    const int nv = row.vectors();
    // box i of this class is bx[i * q]
    const Box2* bx = a.boxes + b * a.N * a.q + (a.q == 1 ? 0 : c);
    ushort* out_score = a.cls_score + w * a.P;
    int* out_idx = a.cls_idx + w * a.P;

    if (t == 0) *count = 0;
    block_sync();
    // first pass: count the candidates and compact the first `cap`
    for (int v = t; v < nv; v += NMS_TPB) {
      const Vec8 r = row.raw8(v);
      const uint32_t m = candidates(r, a.score_thr);
      if (!m) continue;
      uint32_t pos = __hip_atomic_fetch_add(count, uint32_t(__builtin_popcount(m)),
                                            __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_WORKGROUP);
      #pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (!((m >> j) & 1)) continue;
        if (pos < uint32_t(a.cap)) {
          const uint32_t i = uint32_t(v * 8 + j - shift);
          comp_s[pos] = composite(elem(r, j), i);
          box_s[pos] = bx[int64_t(i) * a.q];
        }
        ++pos;
      }
    }
    block_sync();
    const int cnt = int(*count);
    const bool resident = cnt <= a.cap;          // uniform
    if (!resident) {
      for (int v = t; v < nv; v += NMS_TPB)
        alive[v] = (unsigned char)candidates(row.raw8(v), a.score_thr);
      block_sync();
    }

    Corners sup = {0.f, 0.f, 0.f, 0.f, 0.f};
    int r = 0;
    if (cnt > 0) {
      for (; r < a.P; ++r) {
        const bool have = r > 0;
        // this thread's best live candidate: composite, box and its LDS
        // slot (resident) or frame position (streamed)
        uint64_t best_comp = 0;
        Box2 best_box = {0, 0};
        int best_where = 0;
        if (resident) {
          for (int i = t; i < cnt; i += NMS_TPB) {
            const uint64_t cp = comp_s[i];
            if (cp == 0) continue;
            const Box2 bb = box_s[i];
            if (have && suppressed(sup, bb, a.iou_thr)) {
              comp_s[i] = 0;
              continue;
            }
            if (cp > best_comp) {
              best_comp = cp;
              best_box = bb;
              best_where = i;
            }
          }
        } else {
          for (int v = t; v < nv; v += NMS_TPB) {
            const uint32_t m0 = alive[v];
            if (!m0) continue;
            const Vec8 rv = row.raw8(v);
            uint32_t m = m0;
            #pragma unroll
            for (int j = 0; j < 8; ++j) {
              if (!((m0 >> j) & 1)) continue;
              const uint32_t i = uint32_t(v * 8 + j - shift);
              // round 0 suppresses nothing: it loads only its best's box
              const uint64_t cp = composite(elem(rv, j), i);
              if (!have && cp < best_comp) continue;
              const Box2 bb = bx[int64_t(i) * a.q];
              if (have && suppressed(sup, bb, a.iou_thr)) {
                m &= ~(1u << j);
                continue;
              }
              if (cp > best_comp) {
                best_comp = cp;
                best_box = bb;
                best_where = v * 8 + j;
              }
            }
            if (m != m0) alive[v] = (unsigned char)m;
          }
        }

        // the round's winner: composites are distinct, so one lane of a
        // wave with any live candidate owns the wave's maximum
        const uint64_t wmax = wave_max(best_comp);
        Exch* ex = exch + (r & 1) * NMS_WAVES;
        if (wmax == 0 ? lane == 0 : best_comp == wmax) {
          Exch e;
          e.comp = wmax;
          e.box = best_box;
          ex[wv] = e;
        }
        block_sync();
        Exch win = ex[0];
        #pragma unroll
        for (int k = 1; k < NMS_WAVES; ++k) {
          const Exch e = ex[k];
          if (e.comp > win.comp) win = e;
        }
        if (win.comp == 0) break;                // uniform: nothing alive
        if (best_comp == win.comp) {             // the owner marks it dead
          if (resident)
            comp_s[best_where] = 0;
          else
            alive[best_where >> 3] &=
                (unsigned char)~(1u << (best_where & 7));
        }
        if (t == 0) {
          out_score[r] = ushort(win.comp & 0xffffu);
          out_idx[r] = int(comp_index(win.comp));
        }
        sup = corners(win.box);
      }
    }
    for (int i = r + t; i < a.P; i += NMS_TPB) {
      out_score[i] = ushort(BF16_NEG_INF);
      out_idx[i] = 0;
    }
    block_sync();
  }
}

struct GatherArgs {
  const int* slot;          // [B, k] top-k indices into [C*P]
  const ushort* val;        // [B, k] top-k values, -inf = none
  const int* cls_idx;       // [B, C*P]
  const Box2* boxes;        // [B, N, q]
  Box2* out_boxes;          // [B, M]
  ushort* out_scores;       // [B, M]
  ushort* out_classes;      // [B, M]
  int* out_valid;           // [B]
  int B, N, C, q, P, k, M, clip;
};

TFSC_DEV uint32_t clip01(uint32_t raw) {
  const float f = bf_f32(raw);
  return f < 0.f ? 0u : f > 1.f ? 0x3f80u : raw;
}

__global__ __launch_bounds__(NMS_TPB)
void k_nms_gather(GatherArgs a) {
  __shared__ int valid_s;
  const int t = threadIdx.x, lane = t % WAVE;
  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    if (t == 0) valid_s = 0;
    block_sync();
    for (int m0 = 0; m0 < a.M; m0 += NMS_TPB) {
      const int m = m0 + t;
      Box2 ob = {0, 0};
      uint32_t sc = 0, cl = 0;
      bool valid = false;
      if (m < a.k) {
        const uint32_t v = a.val[int64_t(b) * a.k + m];
        const int s = a.slot[int64_t(b) * a.k + m];
        if (v != BF16_NEG_INF && unsigned(s) < unsigned(a.C * a.P)) {
          const int c = s / a.P;
          const int i = a.cls_idx[int64_t(b) * a.C * a.P + s];
          if (unsigned(i) < unsigned(a.N)) {
            ob = a.boxes[(int64_t(b) * a.N + i) * a.q + (a.q == 1 ? 0 : c)];
            if (a.clip) {
              ob.yx1 = clip01(ob.yx1 & 0xffffu) | clip01(ob.yx1 >> 16) << 16;
              ob.yx2 = clip01(ob.yx2 & 0xffffu) | clip01(ob.yx2 >> 16) << 16;
            }
            sc = v;
            cl = f2bf(float(c));
            valid = true;
          }
        }
      }
      if (m < a.M) {
        a.out_boxes[int64_t(b) * a.M + m] = ob;
        a.out_scores[int64_t(b) * a.M + m] = ushort(sc);
        a.out_classes[int64_t(b) * a.M + m] = ushort(cl);
      }
      const uint64_t bal = __builtin_amdgcn_ballot_w64(valid);
      if (lane == 0 && bal)
        __hip_atomic_fetch_add(&valid_s, __builtin_popcountll(bal),
                               __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    block_sync();
    if (t == 0) a.out_valid[b] = valid_s;
    block_sync();
  }
}

// The LDS one workgroup may allocate on the current device. The first
// call on a device also lifts k_nms_select's dynamic LDS limit to it (the
// default is 64 KB). A function attribute is no stream operation, but a
// process may drive more than one device, so it is kept per device; the
// launcher calls this before it launches.
int64_t lds_limit() {
  static std::mutex mu;
  static std::map<int, int64_t> limits;
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  auto it = limits.find(dev);
  if (it != limits.end()) return it->second;
  int v = 0;
  HIP_CHECK(hipDeviceGetAttribute(
      &v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
  HIP_CHECK(hipFuncSetAttribute(
      reinterpret_cast<const void*>(k_nms_select),
      hipFuncAttributeMaxDynamicSharedMemorySize, v));
  limits[dev] = v;
  return v;
}

void check_shape(int64_t B, int64_t N, int64_t C, int64_t q, int64_t P) {
  if (B < 0 || N < 1 || N > NMS_MAX_N || C < 1 || C > INT32_MAX / 2)
    throw std::runtime_error("nms: bad shape B = " + std::to_string(B) +
                             ", N = " + std::to_string(N) + " (at most " +
                             std::to_string(NMS_MAX_N) + "), C = " +
                             std::to_string(C));
  if (q != 1 && q != C)
    throw std::runtime_error("nms: q = " + std::to_string(q) +
                             " is neither 1 nor C = " + std::to_string(C));
  if (P < 1 || P > N)
    throw std::runtime_error("nms: P = " + std::to_string(P) +
                             " outside [1, N = " + std::to_string(N) + "]");
  if (B * C > INT32_MAX / P || B * N > INT32_MAX / q)
    throw std::runtime_error("nms: extent out of range");
}

}  // namespace

int nms_lds_candidates() { return g_lds_candidates; }

void set_nms_lds_candidates(int n) {
  if (n < 1 || n > NMS_LDS_MAX)
    throw std::runtime_error("nms: the LDS candidate cap must be in [1, " +
                             std::to_string(NMS_LDS_MAX) + "]");
  g_lds_candidates = n;
}

void launch_nms_select(hipStream_t s, const ushort* scores_cm,
                       const ushort* boxes, ushort* cls_score, int* cls_idx,
                       int64_t B, int64_t N, int64_t C, int64_t q, int64_t P,
                       float iou_thr, float score_thr) {
  check_shape(B, N, C, q, P);
  if (!(iou_thr >= 0.f && iou_thr <= 1.f))
    throw std::runtime_error("nms: iou_threshold outside [0, 1]");
  if (score_thr != score_thr)
    throw std::runtime_error("nms: score_threshold is NaN");
  if (!scores_cm || !boxes || !cls_score || !cls_idx)
    throw std::runtime_error("nms: select needs scores, boxes, cls_score "
                             "and cls_idx");
  if (reinterpret_cast<uintptr_t>(boxes) % 8)
    throw std::runtime_error("nms: boxes must be 8-byte aligned");
  if (B == 0) return;

  NmsArgs a;
  a.scores = scores_cm;
  a.boxes = reinterpret_cast<const Box2*>(boxes);
  a.cls_score = cls_score;
  a.cls_idx = cls_idx;
  a.rows = B * C;
  a.N = int(N); a.C = int(C); a.q = int(q); a.P = int(P);
  // a class has at most N candidates: small N needs less LDS
  a.cap = int(N < g_lds_candidates ? N : g_lds_candidates);
  a.iou_thr = iou_thr;
  a.score_thr = score_thr;
  // the alive mask: one byte per vector of the frame, whose first score
  // sits at position 0..7
  const int64_t mask_bytes = (N + 7 + 7) / 8;
  int64_t body = int64_t(a.cap) * 16;
  if (mask_bytes > body) body = mask_bytes;
  const int64_t lds = NMS_HEADER + ceil_div(body, 16) * 16;
  if (lds > lds_limit())
    throw std::runtime_error("nms: " + std::to_string(lds) +
                             " bytes of LDS exceed the device's limit");
  const int64_t blocks = a.rows < NMS_MAX_BLOCKS ? a.rows : NMS_MAX_BLOCKS;
  hipLaunchKernelGGL(k_nms_select, dim3(unsigned(blocks)), dim3(NMS_TPB),
                     size_t(lds), s, a);
}

void launch_nms_gather(hipStream_t s, const int* slot, const ushort* val,
                       const int* cls_idx, const ushort* boxes,
                       ushort* out_boxes, ushort* out_scores,
                       ushort* out_classes, int* out_valid, int64_t B,
                       int64_t N, int64_t C, int64_t q, int64_t P, int64_t k,
                       int64_t M, int64_t clip) {
  check_shape(B, N, C, q, P);
  if (M < 1 || M > INT32_MAX / 4 || B * M > INT32_MAX)
    throw std::runtime_error("nms: M = " + std::to_string(M) +
                             " out of range");
  if (k < 1 || k > M || k > C * P)
    throw std::runtime_error("nms: k = " + std::to_string(k) +
                             " outside [1, min(M, C * P)]");
  if (clip != 0 && clip != 1)
    throw std::runtime_error("nms: clip must be 0 or 1");
  if (!slot || !val || !cls_idx || !boxes || !out_boxes || !out_scores ||
      !out_classes || !out_valid)
    throw std::runtime_error("nms: gather needs all eight pointers");
  if (reinterpret_cast<uintptr_t>(boxes) % 8 ||
      reinterpret_cast<uintptr_t>(out_boxes) % 8)
    throw std::runtime_error("nms: boxes must be 8-byte aligned");
  if (B == 0) return;

  GatherArgs a;
  a.slot = slot; a.val = val; a.cls_idx = cls_idx;
  a.boxes = reinterpret_cast<const Box2*>(boxes);
  a.out_boxes = reinterpret_cast<Box2*>(out_boxes);
  a.out_scores = out_scores; a.out_classes = out_classes;
  a.out_valid = out_valid;
  a.B = int(B); a.N = int(N); a.C = int(C); a.q = int(q); a.P = int(P);
  a.k = int(k); a.M = int(M); a.clip = int(clip);
  const int64_t blocks = B < NMS_MAX_BLOCKS ? B : NMS_MAX_BLOCKS;
  hipLaunchKernelGGL(k_nms_gather, dim3(unsigned(blocks)), dim3(NMS_TPB), 0,
                     s, a);
}

}  // namespace tfsc

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
