// Weight layout on the device: one launch turns slots of the bf16 master
// blob into the pre-transposed, K-padded regions of a model's transform
// arena (what GpuModel.conv_weight / conv_weight_cpad / gemm_weight
// compute with torch on a first load). A repeat cold load uploads the blob
// once and runs this instead of uploading the same bytes a second time in
// arena order.
//
// Each LayoutEntry (built by engine/emit.py weight_layout_table) describes
// one region as a padded 2-D transpose of a blob slot, see kernels.h. One
// workgroup writes one 64x64 destination tile; it finds its entry by
// binary search in the prefix sum of tiles per entry. Every byte of an
// entry is written, its zero padding included, and nothing outside it.
// Pure data movement: HBM-bound, no arithmetic on the values.
#include "../common.h"
#include "../kernels.h"

#include <stdexcept>
#include <string>
#include <vector>

namespace tfsc {

static_assert(sizeof(LayoutEntry) == 40, "emit.LAYOUT_ENTRY_DTYPE mirrors it");

constexpr int WL_TILE = 64;
constexpr int WL_TPB = 256;
// LDS row of 72 elements (144 bytes): rows stay 16-byte aligned for the
// vector reads, and the pad spreads the transposing 2-byte writes of a
// wave (8 rows apart) over more than one bank
constexpr int WL_ROW = WL_TILE + 8;
constexpr int WL_VECS = WL_TILE * WL_TILE / 8;      // 16-byte groups a tile

TFSC_DEV bool wl_aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

// 8 consecutive elements of a source row of `cols` elements starting at
// column c; columns >= cols read as zero. A 16-byte load only when the
// address allows it (rows of odd length are not aligned).
TFSC_DEV short8_t wl_load8(const ushort* row, int c, int cols) {
  const ushort* p = row + c;
  if (c + 8 <= cols && wl_aligned16(p))
    return *reinterpret_cast<const short8_t*>(p);
  short8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
  #pragma unroll
  for (int i = 0; i < 8; ++i)
    if (c + i < cols) v[i] = (short)p[i];
  return v;
}

TFSC_DEV void wl_store8(ushort* p, short8_t v) {
  if (wl_aligned16(p)) {
    *reinterpret_cast<short8_t*>(p) = v;
    return;
  }
  #pragma unroll
  for (int i = 0; i < 8; ++i) p[i] = (ushort)v[i];
}

__global__ __launch_bounds__(WL_TPB) void k_weight_layout(
    const ushort* __restrict__ blob, uint8_t* __restrict__ arena,
    const LayoutEntry* __restrict__ table, int n_entries,
    const int* __restrict__ tile_start, int total_tiles) {
  __shared__ __attribute__((aligned(16))) ushort lds[WL_TILE * WL_ROW];
  const int b = blockIdx.x;
  if (b >= total_tiles) return;
  // the last entry whose first tile is <= b
  int lo = 0, hi = n_entries - 1;
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (tile_start[mid] <= b) lo = mid; else hi = mid - 1;
  }
  const LayoutEntry E = table[lo];
  const int t = b - tile_start[lo];
  const int tiles_k = E.kp / WL_TILE;
  const int tr = t / tiles_k;
  const int d0 = tr * WL_TILE;                  // first destination row
  const int k0 = (t - tr * tiles_k) * WL_TILE;  // first destination column
  const int drows = E.transpose ? E.cin : E.rin;
  const ushort* src = blob + E.src_off;
  ushort* dst = reinterpret_cast<ushort*>(arena + E.dst_off);
  const int tid = threadIdx.x;

  if (!E.transpose) {
    // row copy, columns >= cin zero
    for (int g = tid; g < WL_VECS; g += WL_TPB) {
      int r = d0 + (g >> 3);
      int k = k0 + (g & 7) * 8;
      if (r >= drows) continue;
      short8_t v = wl_load8(src + (int64_t)r * E.cin, k, E.cin);
      wl_store8(dst + (int64_t)r * E.kp + k, v);
    }
    return;
  }

  // transpose: destination row d is source column d; destination column k
  // is widened source row k = q * c_dst + c, which is source row
  // q * c_src + c when c < c_src and zero otherwise (as is every k past
  // the last source row)
  for (int g = tid; g < WL_VECS; g += WL_TPB) {
    int kk = g >> 3;
    int j8 = (g & 7) * 8;
    int k = k0 + kk;
    int q = k / E.c_dst;
    int c = k - q * E.c_dst;
    int64_t sr = (int64_t)q * E.c_src + c;
    short8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (c < E.c_src && sr < E.rin)
      v = wl_load8(src + sr * E.cin, d0 + j8, E.cin);
    #pragma unroll
    for (int i = 0; i < 8; ++i)
      lds[(j8 + i) * WL_ROW + kk] = (ushort)v[i];
  }
  __syncthreads();
  for (int g = tid; g < WL_VECS; g += WL_TPB) {
    int j = g >> 3;
    int k8 = (g & 7) * 8;
    int r = d0 + j;
    if (r >= drows) continue;
    short8_t v = *reinterpret_cast<const short8_t*>(&lds[j * WL_ROW + k8]);
    wl_store8(dst + (int64_t)r * E.kp + k0 + k8, v);
  }
}

void launch_weight_layout(hipStream_t s, const ushort* blob, uint8_t* arena,
                          const LayoutEntry* table_dev, int n_entries,
                          const int* tile_start_dev, int total_tiles) {
  if (!blob || !arena || !table_dev || !tile_start_dev)
    throw std::runtime_error("weight_layout: null pointer");
  if (n_entries < 1 || total_tiles < n_entries)
    throw std::runtime_error(
        "weight_layout: " + std::to_string(n_entries) + " entries, " +
        std::to_string(total_tiles) + " tiles");
  hipLaunchKernelGGL(k_weight_layout, dim3(total_tiles), dim3(WL_TPB), 0, s,
                     blob, arena, table_dev, n_entries, tile_start_dev,
                     total_tiles);
}

namespace {

void wl_check(hipError_t e, hipStream_t s, const char* what) {
  if (e == hipSuccess) return;
  // what was enqueued before the failure still reads the caller's
  // buffers: let it finish before the caller can free them
  (void)hipStreamSynchronize(s);
  throw std::runtime_error(std::string("restore_weights: ") + what + ": " +
                           hipGetErrorString(e));
}

// [off, off + n) inside [0, size), without overflow
bool wl_inside(int64_t off, int64_t n, int64_t size) {
  return off >= 0 && n >= 0 && off <= size && n <= size - off;
}

}  // namespace

void restore_weights(hipStream_t s, ushort* blob_dev,
                     const ushort* blob_pinned, int64_t blob_bytes,
                     uint8_t* arena_dev, int64_t arena_bytes,
                     const uint8_t* arena_pinned, int64_t pinned_bytes,
                     const std::vector<RestoreSpan>& spans,
                     const LayoutEntry* table_dev, int n_entries,
                     const int* tile_start_dev, int total_tiles) {
  // every check comes before the first enqueue
  if (blob_bytes < 0 || arena_bytes < 0 || pinned_bytes < 0)
    throw std::runtime_error("restore_weights: negative size");
  if (blob_bytes > 0 && (!blob_dev || !blob_pinned))
    throw std::runtime_error("restore_weights: null blob pointer");
  if (arena_bytes > 0 && !arena_dev)
    throw std::runtime_error("restore_weights: null arena pointer");
  if (!spans.empty() && (!arena_dev || !arena_pinned))
    throw std::runtime_error("restore_weights: spans without an arena");
  for (const RestoreSpan& sp : spans) {
    if (sp.nbytes < 0)
      throw std::runtime_error("restore_weights: negative span size");
    if (!wl_inside(sp.arena_off, sp.nbytes, arena_bytes))
      throw std::runtime_error("restore_weights: span outside the arena");
    if (!wl_inside(sp.pinned_off, sp.nbytes, pinned_bytes))
      throw std::runtime_error(
          "restore_weights: span outside the pinned remainder");
  }
  if (n_entries < 0 || total_tiles < n_entries)
    throw std::runtime_error(
        "restore_weights: " + std::to_string(n_entries) + " entries, " +
        std::to_string(total_tiles) + " tiles");
  if (n_entries > 0 && (!blob_dev || !arena_dev || !table_dev ||
                        !tile_start_dev))
    throw std::runtime_error("restore_weights: null layout pointer");

  bool any = false;
  if (blob_bytes > 0) {
    wl_check(hipMemcpyAsync(blob_dev, blob_pinned, (size_t)blob_bytes,
                            hipMemcpyHostToDevice, s), s, "blob copy");
    any = true;
  }
  for (const RestoreSpan& sp : spans) {
    if (sp.nbytes == 0) continue;
    wl_check(hipMemcpyAsync(arena_dev + sp.arena_off,
                            arena_pinned + sp.pinned_off, (size_t)sp.nbytes,
                            hipMemcpyHostToDevice, s), s, "span copy");
    any = true;
  }
  if (n_entries > 0) {
    // stream order puts the launch after the blob copy it reads
    launch_weight_layout(s, blob_dev, arena_dev, table_dev, n_entries,
                         tile_start_dev, total_tiles);
    wl_check(hipGetLastError(), s, "layout launch");
    any = true;
  }
  if (any) wl_check(hipStreamSynchronize(s), s, "synchronize");
}

}  // namespace tfsc
