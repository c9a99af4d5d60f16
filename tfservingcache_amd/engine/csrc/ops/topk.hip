// Row-wise top-k over the last axis (TF TopKV2) for gfx950: bf16 scores
// [rows, cols] -> the k largest values (bf16, original bits) and their
// i32 indices, values descending, ties by lower index first.
//
// A bf16 word maps to a 16-bit key that orders like the value (-0.0 is
// folded onto +0.0 first, so the zeros tie). An element travels as the
// 64-bit composite
//     key << 48 | ~index << 16 | raw bits
// whose plain descending order is the TF order; composite 0 is never a
// real element (index < 2^31) and serves as padding.
//
// Two kernels, both 256 threads:
//   k_topk_sort    rows of at most SORT_COLS columns: the whole row as
//                  composites in LDS, bitonic sort, first k written.
//   k_topk_select  one workgroup per (row, segment): an exact two-pass
//                  radix select on the key (high byte, then low byte
//                  inside the chosen bin) gives the threshold key T, the
//                  number of keys above it and how many keys equal to T
//                  are still needed; a walk in index order collects
//                  exactly k composites into LDS, which are sorted and
//                  written. The row is never sorted.
// A row split into P segments writes P*k composites per row to scratch
// and the same select kernel, instantiated on a loader that reads
// composites, picks the final k. Segments cover ascending index ranges
// and each segment's list is sorted, so equal keys still meet the walk
// in ascending index order.
//
// Data movement in k_topk_select: the segment is addressed in a frame
// that starts at the 16-byte boundary at or below its first element, so
// every 8-element vector is one aligned 16-byte load; the first and last
// vector of a segment (rows with cols % 8 != 0 start anywhere) are read
// element by element under a bounds mask instead. When the frame fits
// CACHE_ELEMS the first pass parks the raw words in LDS and the next two
// read them there; otherwise they re-read global memory. LDS per
// workgroup is 45 KB (cache 32 KB, candidates 8 KB, histograms and
// suffix sums 5 KB): three workgroups per CU of 160 KB.
#include "../common.h"
#include "../kernels.h"

#include <stdexcept>
#include <string>

namespace tfsc {

namespace {

constexpr int TOPK_TPB = 256;
constexpr int TOPK_WAVES = TOPK_TPB / WAVE;
constexpr int TOPK_MAX_K = 1024;
constexpr int TOPK_MAX_BLOCKS = 2048;
constexpr int SORT_COLS = 2048;          // k_topk_sort's LDS row
constexpr int CACHE_ELEMS = 16384;       // k_topk_select's LDS segment
constexpr int CACHE_VECS = CACHE_ELEMS / 8;

// rows of at most this many columns go to k_topk_sort (measured,
// profiles/topk.md); scripts/topk_probe.py moves it to time both sides
int g_sort_max_cols = 256;

TFSC_DEV uint32_t key_of(uint32_t b) {
  if (b == 0x8000u) b = 0;
  return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}

TFSC_DEV uint64_t composite(uint32_t raw, int64_t index) {
  return (uint64_t(key_of(raw)) << 48) |
         (uint64_t(~uint32_t(index)) << 16) | raw;
}

// descending bitonic sort of n (a power of two) composites in LDS; the
// caller synchronises before, the sort ends synchronised
TFSC_DEV void bitonic_desc(uint64_t* a, int n) {
  for (int k2 = 2; k2 <= n; k2 <<= 1)
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < n / 2; t += TOPK_TPB) {
        int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        int p = i | j;
        bool desc = (i & k2) == 0;
        uint64_t x = a[i], y = a[p];
        if ((x < y) == desc) {
          a[i] = y;
          a[p] = x;
        }
      }
      __syncthreads();
    }
}

TFSC_DEV int pow2_at_least(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

// first k of the sorted composites -> the row's outputs
TFSC_DEV void write_row(const uint64_t* a, int k, ushort* vals, int* idx) {
  for (int i = threadIdx.x; i < k; i += TOPK_TPB) {
    uint64_t c = a[i];
    vals[i] = ushort(c & 0xffffu);
    idx[i] = int(~uint32_t(c >> 16));
  }
}

// ---------------------------------------------------------------------------
// short rows: sort the row
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(TOPK_TPB)
void k_topk_sort(const ushort* __restrict__ x, ushort* __restrict__ vals,
                 int* __restrict__ idx, int64_t rows, int cols, int k) {
  __shared__ uint64_t row_s[SORT_COLS];
  const int n = pow2_at_least(cols);
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const ushort* xr = x + row * cols;
    for (int i = threadIdx.x; i < n; i += TOPK_TPB)
      row_s[i] = i < cols ? composite(xr[i], i) : 0;
    __syncthreads();
    bitonic_desc(row_s, n);
    write_row(row_s, k, vals + row * k, idx + row * k);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// loaders of k_topk_select: 8 elements per call as kr[j] = key | raw << 16
// and a mask of the valid ones
// ---------------------------------------------------------------------------
struct LoadBf16 {
  static constexpr bool kCache = true;
  const ushort* base;   // frame origin, 16-byte aligned
  int shift;            // frame position of the segment's first element
  int64_t n;            // segment length
  int64_t index0;       // row index of the segment's first element

  TFSC_DEV int64_t frame() const { return shift + n; }

  TFSC_DEV uint4 raw8(int64_t v) const {
    int64_t q0 = v * 8;
    if (q0 >= shift && q0 + 8 <= shift + n)
      return *reinterpret_cast<const uint4*>(base + q0);
    uint32_t w[4] = {0, 0, 0, 0};
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      int64_t q = q0 + j;
      if (q >= shift && q < shift + n)
        w[j >> 1] |= uint32_t(base[q]) << ((j & 1) * 16);
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
  }

  TFSC_DEV uint32_t unpack(uint4 r, int64_t v, uint32_t kr[8]) const {
    uint32_t w[4] = {r.x, r.y, r.z, r.w};
    uint32_t mask = 0;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      int64_t q = v * 8 + j;
      uint32_t raw = (w[j >> 1] >> ((j & 1) * 16)) & 0xffffu;
      kr[j] = key_of(raw) | (raw << 16);
      if (q >= shift && q < shift + n) mask |= 1u << j;
    }
    return mask;
  }

  TFSC_DEV uint64_t comp(int64_t q, uint32_t kr) const {
    return composite(kr >> 16, index0 + (q - shift));
  }
};

struct LoadComp {
  static constexpr bool kCache = false;
  const uint64_t* src;
  int64_t n;

  TFSC_DEV int64_t frame() const { return n; }
  TFSC_DEV uint4 raw8(int64_t) const { return make_uint4(0, 0, 0, 0); }

  TFSC_DEV uint32_t load8(int64_t v, uint32_t kr[8]) const {
    uint32_t mask = 0;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      int64_t q = v * 8 + j;
      uint64_t c = q < n ? src[q] : 0;
      kr[j] = uint32_t(c >> 48);
      if (c != 0) mask |= 1u << j;      // composite 0 is padding
    }
    return mask;
  }

  TFSC_DEV uint64_t comp(int64_t q, uint32_t) const { return src[q]; }
};

template <class L>
TFSC_DEV uint32_t fetch8(const L& ld, const uint4* cache, bool cached,
                         int64_t v, uint32_t kr[8]) {
  if constexpr (L::kCache) {
    return ld.unpack(cached ? cache[v] : ld.raw8(v), v, kr);
  } else {
    return ld.load8(v, kr);
  }
}

// Merge the per-wave histograms into hist[0..255], scan them from the
// top bin down and return, in every thread, the bin holding the want-th
// largest key, the count of keys above that bin, and the total count.
// hist is [TOPK_WAVES][256] followed by 256 words for the suffix sums.
TFSC_DEV void find_bin(uint32_t* hist, uint32_t* sel, int want_or_neg,
                       int k, int* bin, int* above, int* total) {
  const int t = threadIdx.x, lane = t % WAVE, wv = t / WAVE;
  uint32_t h = 0;
  #pragma unroll
  for (int w = 0; w < TOPK_WAVES; ++w) h += hist[w * 256 + t];
  // inclusive suffix sum over the 256 bins, one bin per thread
  uint32_t s = h;
  #pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    uint32_t o = __shfl_down(s, off, WAVE);
    if (lane + off < WAVE) s += o;
  }
  if (lane == 0) sel[4 + wv] = s;
  __syncthreads();
  #pragma unroll
  for (int w = 0; w < TOPK_WAVES; ++w)
    if (w > wv) s += sel[4 + w];
  uint32_t* sfx = hist + TOPK_WAVES * 256;
  sfx[t] = s;
  __syncthreads();
  const int tot = int(sfx[0]);
  // want_or_neg < 0: the first pass, which wants min(k, total)
  const int want = want_or_neg < 0 ? (k < tot ? k : tot) : want_or_neg;
  const int ab = int(s - h);
  if (ab < want && int(s) >= want) {
    sel[0] = uint32_t(t);
    sel[1] = uint32_t(ab);
  }
  __syncthreads();
  *bin = int(sel[0]);
  *above = int(sel[1]);
  *total = tot;
}

// Select the k largest of one loader's elements into cand (sorted,
// padded with 0 up to k when fewer exist).
template <class L>
TFSC_DEV void select_k(const L& ld, int k, uint64_t* cand, uint32_t* hist,
                       uint32_t* sel, uint4* cache) {
  const int t = threadIdx.x, lane = t % WAVE, wv = t / WAVE;
  const int64_t nv = (ld.frame() + 7) / 8;
  const bool cached = L::kCache && nv <= CACHE_VECS;
  uint32_t* my_hist = hist + wv * 256;
  uint32_t kr[8];

  // pass 1: histogram of the key's high byte
  for (int i = t; i < TOPK_WAVES * 256; i += TOPK_TPB) hist[i] = 0;
  if (t < 2) sel[t] = 0;
  __syncthreads();
  for (int64_t v = t; v < nv; v += TOPK_TPB) {
    uint32_t mask;
    if constexpr (L::kCache) {
      uint4 r = ld.raw8(v);
      if (cached) cache[v] = r;
      mask = ld.unpack(r, v, kr);
    } else {
      mask = ld.load8(v, kr);
    }
    // neighbours mostly share a bin: add runs, not elements
    int prev = -1;
    uint32_t run = 0;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (!((mask >> j) & 1)) continue;
      int b = int((kr[j] >> 8) & 0xffu);
      if (b != prev) {
        if (run) atomicAdd(&my_hist[prev], run);
        prev = b;
        run = 0;
      }
      ++run;
    }
    if (run) atomicAdd(&my_hist[prev], run);
  }
  __syncthreads();
  int hi_bin, above_hi, total;
  find_bin(hist, sel, -1, k, &hi_bin, &above_hi, &total);
  const int keff = k < total ? k : total;
  const int npad = pow2_at_least(k);
  if (keff == 0) {                       // empty segment: all padding
    for (int i = t; i < npad; i += TOPK_TPB) cand[i] = 0;
    __syncthreads();
    return;
  }

  // pass 2: histogram of the low byte inside that bin
  for (int i = t; i < TOPK_WAVES * 256; i += TOPK_TPB) hist[i] = 0;
  __syncthreads();
  for (int64_t v = t; v < nv; v += TOPK_TPB) {
    uint32_t mask = fetch8(ld, cache, cached, v, kr);
    #pragma unroll
    for (int j = 0; j < 8; ++j)
      if (((mask >> j) & 1) && int((kr[j] >> 8) & 0xffu) == hi_bin)
        atomicAdd(&my_hist[kr[j] & 0xffu], 1u);
  }
  __syncthreads();
  int lo_bin, above_lo;
  find_bin(hist, sel, keff - above_hi, k, &lo_bin, &above_lo, &total);
  const uint32_t T = uint32_t(hi_bin << 8 | lo_bin);
  const int count_gt = above_hi + above_lo;
  const int need = keff - count_gt;      // keys == T still wanted, >= 1

  // pass 3: walk in index order; every key > T and the first `need`
  // keys == T land in cand[0..keff)
  int base_gt = 0, base_eq = 0;
  uint32_t* wtot = sel + 8;              // [2][TOPK_WAVES]
  int parity = 0;
  for (int64_t v0 = 0; v0 < nv; v0 += TOPK_TPB, parity ^= 1) {
    const int64_t v = v0 + t;
    uint32_t mask = 0;
    if (v < nv) mask = fetch8(ld, cache, cached, v, kr);
    uint32_t gt = 0, eq = 0;             // bit j: element j is > T / == T
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (!((mask >> j) & 1)) continue;
      uint32_t key = kr[j] & 0xffffu;
      if (key > T) gt |= 1u << j;
      else if (key == T) eq |= 1u << j;
    }
    // block-wide exclusive scan of (count gt | count eq << 16)
    const uint32_t mine = uint32_t(__popc(gt)) | uint32_t(__popc(eq)) << 16;
    uint32_t s = mine;
    #pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
      uint32_t o = __shfl_up(s, off, WAVE);
      if (lane >= off) s += o;
    }
    if (lane == WAVE - 1) wtot[parity * TOPK_WAVES + wv] = s;
    __syncthreads();
    uint32_t before = 0, chunk = 0;
    #pragma unroll
    for (int w = 0; w < TOPK_WAVES; ++w) {
      uint32_t wt = wtot[parity * TOPK_WAVES + w];
      if (w < wv) before += wt;
      chunk += wt;
    }
    const uint32_t excl = before + s - mine;
    int pos_gt = base_gt + int(excl & 0xffffu);
    int pos_eq = base_eq + int(excl >> 16);
    if (gt | eq) {
      #pragma unroll
      for (int j = 0; j < 8; ++j) {
        if ((gt >> j) & 1) {
          if (pos_gt < count_gt) cand[pos_gt] = ld.comp(v * 8 + j, kr[j]);
          ++pos_gt;
        } else if ((eq >> j) & 1) {
          if (pos_eq < need)
            cand[count_gt + pos_eq] = ld.comp(v * 8 + j, kr[j]);
          ++pos_eq;
        }
      }
    }
    base_gt += int(chunk & 0xffffu);
    base_eq += int(chunk >> 16);
    if (base_gt >= count_gt && base_eq >= need) break;   // uniform
  }

  // pass 4: sort the candidates
  for (int i = keff + t; i < npad; i += TOPK_TPB) cand[i] = 0;
  __syncthreads();
  bitonic_desc(cand, npad);
}

struct TopkArgs {
  const ushort* x;          // [rows, cols] bf16 (segment launch)
  const uint64_t* part_in;  // [rows, P, k] composites (merge launch)
  uint64_t* part_out;       // segment launch with P > 1, else null
  ushort* vals;             // [rows, k]
  int* idx;                 // [rows, k]
  int64_t rows, cols, seglen;
  int k, P;
};

template <bool MERGE>
__global__ __launch_bounds__(TOPK_TPB)
void k_topk_select(TopkArgs a) {
  __shared__ uint64_t cand[TOPK_MAX_K];
  __shared__ uint32_t hist[(TOPK_WAVES + 1) * 256];
  __shared__ uint32_t sel[8 + 2 * TOPK_WAVES];
  __shared__ uint4 cache[MERGE ? 1 : CACHE_VECS];
  const int64_t items = MERGE ? a.rows : a.rows * a.P;
  for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {
    int64_t row;
    if constexpr (MERGE) {
      row = w;
      LoadComp ld{a.part_in + row * a.P * a.k, int64_t(a.P) * a.k};
      select_k(ld, a.k, cand, hist, sel, cache);
    } else {
      row = w / a.P;
      int64_t s0 = (w % a.P) * a.seglen;
      int64_t n = a.cols - s0 < a.seglen ? a.cols - s0 : a.seglen;
      if (n < 0) n = 0;
      const ushort* first = a.x + row * a.cols + s0;
      int shift = int((reinterpret_cast<uintptr_t>(first) & 15) / 2);
      LoadBf16 ld{first - shift, shift, n, s0};
      select_k(ld, a.k, cand, hist, sel, cache);
    }
    if (!MERGE && a.part_out) {
      uint64_t* out = a.part_out + w * a.k;
      for (int i = threadIdx.x; i < a.k; i += TOPK_TPB) out[i] = cand[i];
    } else {
      write_row(cand, a.k, a.vals + row * a.k, a.idx + row * a.k);
    }
    __syncthreads();
  }
}

int blocks_for(int64_t items) {
  return int(items < 1 ? 1 : items < TOPK_MAX_BLOCKS ? items
                                                     : TOPK_MAX_BLOCKS);
}

}  // namespace

int topk_sort_max_cols() { return g_sort_max_cols; }

void set_topk_sort_max_cols(int cols) {
  if (cols < 0 || cols > SORT_COLS)
    throw std::runtime_error("topk: sort bound must be in [0, " +
                             std::to_string(SORT_COLS) + "]");
  g_sort_max_cols = cols;
}

void launch_topk_last(hipStream_t s, const ushort* x, int* idx, ushort* vals,
                      void* scratch, int64_t rows, int64_t cols, int64_t k,
                      int64_t P) {
  if (rows < 0 || cols < 1 || cols > INT32_MAX)
    throw std::runtime_error("topk: bad shape [" + std::to_string(rows) +
                             ", " + std::to_string(cols) + "]");
  if (k < 1 || k > TOPK_MAX_K || k > cols)
    throw std::runtime_error("topk: k = " + std::to_string(k) +
                             " outside [1, min(cols, " +
                             std::to_string(TOPK_MAX_K) + ")]");
  if (P < 1 || P > cols || P > 4096)
    throw std::runtime_error("topk: P = " + std::to_string(P) +
                             " outside [1, min(cols, 4096)]");
  if (P > 1 && scratch == nullptr)
    throw std::runtime_error("topk: a split row needs scratch");
  if (rows == 0) return;
  if (P == 1 && cols <= g_sort_max_cols) {
    hipLaunchKernelGGL(k_topk_sort, dim3(blocks_for(rows)), dim3(TOPK_TPB),
                       0, s, x, vals, idx, rows, int(cols), int(k));
    return;
  }
  TopkArgs a;
  a.x = x;
  a.part_in = reinterpret_cast<const uint64_t*>(scratch);
  a.part_out = P > 1 ? reinterpret_cast<uint64_t*>(scratch) : nullptr;
  a.vals = vals;
  a.idx = idx;
  a.rows = rows;
  a.cols = cols;
  a.seglen = ceil_div(cols, P);
  a.k = int(k);
  a.P = int(P);
  hipLaunchKernelGGL(k_topk_select<false>, dim3(blocks_for(rows * P)),
                     dim3(TOPK_TPB), 0, s, a);
  if (P > 1)
    hipLaunchKernelGGL(k_topk_select<true>, dim3(blocks_for(rows)),
                       dim3(TOPK_TPB), 0, s, a);
}

}  // namespace tfsc
