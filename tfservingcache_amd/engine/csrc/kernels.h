// Host-side kernel launcher declarations. All activation buffers are
// bf16 (ushort) unless noted; integer buffers are int32. Launches are
// asynchronous on the given stream.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>

namespace tfsc {

// elementwise fn codes (planner 'eltwise' op)
enum EltFn : int {
  ELT_ADD = 0, ELT_SUB, ELT_MUL, ELT_DIV, ELT_MAX, ELT_MIN, ELT_SQDIFF,
  ELT_RELU, ELT_TANH, ELT_SIGMOID, ELT_ERF, ELT_SQRT, ELT_RSQRT, ELT_EXP,
  ELT_NEG, ELT_SQUARE, ELT_GELU, ELT_RELU6,
};

// activation codes for fused epilogues
enum Act : int { ACT_NONE = 0, ACT_RELU, ACT_TANH, ACT_SIGMOID, ACT_GELU,
                 ACT_RELU6 };

constexpr int MAX_DIMS = 6;

struct BcastArgs {          // broadcast strides (elements), 0 = broadcast
  int ndim;
  int64_t dims[MAX_DIMS];
  int64_t sa[MAX_DIMS];
  int64_t sb[MAX_DIMS];
};

void launch_eltwise_unary(hipStream_t s, const ushort* x, ushort* y,
                          int64_t n, int fn);
void launch_eltwise_binary(hipStream_t s, const ushort* a, const ushort* b,
                           ushort* y, int64_t n_out, const BcastArgs& bc,
                           int fn);
void launch_bn_act(hipStream_t s, const ushort* x, const ushort* scale,
                   const ushort* shift, ushort* y, int64_t rows, int64_t c,
                   int act);
void launch_softmax(hipStream_t s, const ushort* x, ushort* y,
                    int64_t rows, int64_t cols);
// y = (x - mean) * rsqrt(var + eps) * gamma + beta over the last dim, with
// var = mean((x - mean)^2) taken in a second pass over the row
void launch_layernorm(hipStream_t s, const ushort* x, const ushort* gamma,
                      const ushort* beta, ushort* y, int64_t rows,
                      int64_t cols, float eps);
void launch_reduce_mean_last(hipStream_t s, const ushort* x, ushort* y,
                             int64_t rows, int64_t cols);
// mean over axis 1 of [d0, d1, d2] (global mean over H,W of NHWC is
// d1 = H*W)
void launch_reduce_mean_mid(hipStream_t s, const ushort* x, ushort* y,
                            int64_t d0, int64_t d1, int64_t d2);
void launch_pool(hipStream_t s, const ushort* x, ushort* y, bool is_max,
                 int N, int H, int W, int C, int Ho, int Wo, int kh, int kw,
                 int sh, int sw, int pt, int pl);
// NDHWC max / average pooling (K_POOL's 18-int form). Taps outside the
// volume are skipped; the average divides by the in-volume tap count. 8
// channels per thread with 16-byte accesses when C % 8 == 0 and both
// pointers are 16-byte aligned, one element per thread otherwise. Throws
// before any launch on an extent, window or stride < 1.
void launch_pool3d(hipStream_t s, const ushort* x, ushort* y, bool is_max,
                   int N, int D, int H, int W, int C, int Do, int Ho, int Wo,
                   int kd, int kh, int kw, int sd, int sh, int sw, int pf,
                   int pt, int pl);
void launch_transpose(hipStream_t s, const ushort* x, ushort* y, int ndim,
                      const int64_t* out_dims, const int64_t* in_strides,
                      int64_t n_out);
// inverse of launch_transpose: LINEAR source -> STRIDED destination
// (concat writes each input into an offset slice of the output)
void launch_scatter(hipStream_t s, const ushort* x, ushort* y, int ndim,
                    const int64_t* in_dims, const int64_t* out_strides,
                    int64_t n_in);
void launch_gather_rows(hipStream_t s, const ushort* table, const int* idx,
                        ushort* y, int64_t n_idx, int64_t row_elems);
void launch_pad_nhwc(hipStream_t s, const ushort* x, ushort* y,
                     int N, int H, int W, int C, int pt, int pb, int pl,
                     int pr);
void launch_pad_last(hipStream_t s, const ushort* x, ushort* y,
                     int64_t rows, int c_in, int c_out);
void launch_f32_to_bf16(hipStream_t s, const float* x, ushort* y,
                        int64_t n);
// dtype casts between workspace tensors: 0 = i32 -> bf16,
// 1 = bf16 -> i32 (truncate toward zero, TF Cast semantics)
void launch_cast(hipStream_t s, const void* x, void* y, int64_t n,
                 int mode);
// rowwise argmax over the last dim: [rows, cols] bf16 -> i32 (first
// max wins on ties, TF semantics; a row of all -inf answers 0)
void launch_argmax_last(hipStream_t s, const ushort* x, int* y,
                        int64_t rows, int64_t cols);
// rowwise top-k over the last dim (TF TopKV2), ops/topk.hip:
// [rows, cols] bf16 -> vals [rows, k] bf16 (the elements' own bits) and
// idx [rows, k] i32, values descending, equal values by lower index
// (+0.0 and -0.0 are equal). Exact selection, no arithmetic. P > 1
// splits every row into P segments of ceil(cols / P) columns whose
// partial results meet in `scratch` (rows * P * k * 8 bytes, 8-byte
// aligned; may be null when P == 1) and a second launch picks the final
// k. NaN order is unspecified. Throws before any launch unless
// 1 <= k <= min(cols, 1024), 1 <= P <= min(cols, 4096), cols < 2^31 and
// scratch is set when P > 1.
void launch_topk_last(hipStream_t s, const ushort* x, int* idx, ushort* vals,
                      void* scratch, int64_t rows, int64_t cols, int64_t k,
                      int64_t P);
// rows of at most this many columns (<= 2048) are sorted whole instead of
// radix-selected; a measurement switch (scripts/topk_probe.py)
int topk_sort_max_cols();
void set_topk_sort_max_cols(int cols);
// reduction over the middle axis of a bf16 view [outer, red, inner]
// (inner == 1: over the last axis), ops/reduce.hip: y [outer, inner]
// bf16, f32 accumulation, one rounding. fn: 0 mean, 1 sum, 2 max, 3 min,
// 4 prod. P > 1 splits red into P segments of ceil(red / P) whose f32
// partials meet in `scratch` (outer * inner * P * 4 bytes; may be null
// when P == 1) and a second launch folds them. Max and min skip NaN.
// Throws before any launch unless every extent is >= 1,
// 1 <= P <= min(red, 4096) and scratch is set when P > 1.
void launch_reduce(hipStream_t s, const ushort* x, ushort* y, void* scratch,
                   int64_t outer, int64_t red, int64_t inner, int fn,
                   int64_t P);
// rows of at most wave_max_cols columns run one wave per row, longer ones
// one workgroup per (row, segment); a k_reduce_cols tile is at most
// cols_tx_max lanes wide (a power of two <= 256) and narrows, down to 8
// lanes, while the launch has fewer than cols_wg_target workgroups (0:
// never); reduce_cols_lg_tx is log2 of the width chosen. Measurement
// switches (scripts/reduce_probe.py).
int reduce_wave_max_cols();
int reduce_cols_tx_max();
int reduce_cols_wg_target();
int reduce_cols_lg_tx(int64_t outer, int64_t inner, int64_t P, bool vec);
void set_reduce_thresholds(int wave_max_cols, int cols_tx_max,
                           int cols_wg_target);
void launch_bf16_to_f32(hipStream_t s, const ushort* x, float* y,
                        int64_t n);

// One region of a model's transform arena as a padded 2-D transpose of a
// slot of the bf16 master blob (ops/weight_layout.hip; the table is built
// by engine/emit.py weight_layout_table, whose LAYOUT_ENTRY_DTYPE mirrors
// this struct). The slot is a row-major [rin][cin] matrix at element
// src_off of the blob; the region starts at byte dst_off of the arena.
//   transpose == 0: dst [rin][kp], dst[r][k] = src[r][k], 0 for k >= cin
//     (gemm_weight with trans_b: a row copy with pad).
//   transpose == 1: dst [cin][kp], dst[j][k] = src[q * c_src + c][j] with
//     k = q * c_dst + c, 0 when c >= c_src or the source row is >= rin
//     (conv_weight and gemm_weight without trans_b: c_src == c_dst;
//     conv_weight_cpad: c_src = C, c_dst = c8, zeros between).
// kp is a multiple of 64, at least the widened row count.
struct LayoutEntry {
  int64_t src_off;
  int64_t dst_off;
  int32_t rin, cin;
  int32_t c_src, c_dst;
  int32_t transpose;
  int32_t kp;
};
// Lays out every entry in one launch: one workgroup per 64x64 destination
// tile, tile_start_dev [n_entries + 1] the prefix sum of tiles per entry
// (every entry has at least one), total_tiles its last element. Writes
// all rows * kp * 2 bytes of each entry and nothing else. 16-byte accesses
// where an address is 16-byte aligned, element accesses elsewhere. The
// table lives on the device and is not checked here: emit.py
// check_layout_table bounds it against the blob and the arena. Throws
// before the launch on a null pointer, n_entries < 1 or
// total_tiles < n_entries.
void launch_weight_layout(hipStream_t s, const ushort* blob, uint8_t* arena,
                          const LayoutEntry* table_dev, int n_entries,
                          const int* tile_start_dev, int total_tiles);

// One contiguous run of arena bytes a repeat load copies from the plan's
// pinned remainder (int weights, fp8 bytes and scales).
struct RestoreSpan {
  int64_t arena_off, pinned_off, nbytes;
};
// A repeat cold load's whole upload on stream s, ended by one blocking
// hipStreamSynchronize(s): blob_bytes from blob_pinned to blob_dev (0:
// the blob is on the device already), every span from arena_pinned to
// arena_dev, then the layout launch above when n_entries > 0. Host
// pointers are pinned memory. Everything that can be checked on the host
// is checked before the first enqueue, and a failed check throws with
// nothing enqueued: a negative size, a null pointer that the sizes say is
// used, a span outside [0, arena_bytes) or [0, pinned_bytes),
// total_tiles < n_entries. The table is trusted as in
// launch_weight_layout. Every HIP return code is checked; on a failure
// after the first enqueue the stream is synchronised before the throw.
void restore_weights(hipStream_t s, ushort* blob_dev,
                     const ushort* blob_pinned, int64_t blob_bytes,
                     uint8_t* arena_dev, int64_t arena_bytes,
                     const uint8_t* arena_pinned, int64_t pinned_bytes,
                     const std::vector<RestoreSpan>& spans,
                     const LayoutEntry* table_dev, int n_entries,
                     const int* tile_start_dev, int total_tiles);

// GEMM: C[M,N] = act(A[M,K] @ B[K,N] + bias [+ residual]).
// A row-major bf16, B row-major bf16 (pre-transposed at load if the graph
// wanted B^T), C bf16. f32 accumulate via MFMA.
void launch_gemm(hipStream_t s, const ushort* A, const ushort* B,
                 const ushort* bias, const ushort* residual, ushort* C,
                 int64_t M, int64_t N, int64_t K, int act, float alpha);

// Batched GEMM over leading batch dim: [bat, M, K] @ [bat, K, N] (operands
// contiguous; strides in elements; stride 0 broadcasts an operand).
void launch_batched_gemm(hipStream_t s, const ushort* A, const ushort* B,
                         ushort* C, int64_t bat, int64_t M, int64_t N,
                         int64_t K, int64_t strideA, int64_t strideB,
                         int64_t strideC, bool trans_b, float alpha);

// Fused implicit-GEMM NHWC Conv2D (C % 8 == 0):
//   y[N*Ho*Wo, Kc] = act(x (*) w + bias [+ residual])
// with w pre-transposed [Kc][pad64(R*S*C)] like launch_gemm's B. The
// A-tile gather happens in the GEMM's LDS staging (per-lane source
// address from the conv geometry; out-of-image patches read from
// `zeros`, a >=16-byte zeroed device buffer).
// groups > 1 is a grouped conv on its own kernel: group g reads input
// channels g*Cg.. (Cg = C/groups, Cg % 8 == 0) and writes output
// channels g*Ng.. (Ng = Kc/groups, Ng % 8 == 0); w is
// [Kc][pad64(R*S*Cg)], row g*Ng + n being group g's filter n, and
// k_pad = pad64(R*S*Cg).
// (dh, dw) != (1, 1) is a dilated (atrous) conv on its own kernel: tap
// (r, s) reads hi = ho*sh - pt + r*dh, wi = wo*sw - pl + s*dw; w and
// k_pad = pad64(R*S*C) are laid out as for dilation 1. When C % 64 == 0
// the kernel can skip the K tiles of taps that lie outside the image for
// a whole M tile (see set_conv_dilated_skip). Throws before any launch on dh < 1 or dw < 1, on a
// dilation with groups > 1, and on a dilation with C % 8 != 0.
// dh == dw == 1 runs exactly the kernels described above.
void launch_conv_igemm(hipStream_t s, const ushort* x, const ushort* w,
                       const ushort* bias, const ushort* residual,
                       const ushort* zeros, ushort* y,
                       int N, int H, int W, int C, int Kc, int R, int S,
                       int sh, int sw, int pt, int pl, int Ho, int Wo,
                       int k_pad, int act, int groups = 1, int dh = 1,
                       int dw = 1);
// 3-D conv (K_CONV's 23-int form), NDHWC: y[N,Do,Ho,Wo,Kc] =
// act(conv3d(x[N,D,H,W,C], w) + bias [+ residual]); tap (t, r, s) reads
// di = do*sd - pf + t, hi = ho*sh - pt + r, wi = wo*sw - pl + s. w is
// [Kc][pad64(T*R*S*C)] with k = ((t*R + r)*S + s)*C + c and
// k_pad = pad64(T*R*S*C). Implicit GEMM on its own kernel, no im2col
// buffer; C % 64 == 0 takes the instantiation whose tap is block-uniform.
// groups, dh and dw are the 23-int form's reserved slots: throws before
// any launch unless they are all 1, on C % 8 != 0, on a k_pad that is not
// pad64(T*R*S*C), and on any extent or stride < 1.
void launch_conv3d_igemm(hipStream_t s, const ushort* x, const ushort* w,
                         const ushort* bias, const ushort* residual,
                         const ushort* zeros, ushort* y,
                         int N, int D, int H, int W, int C, int Kc,
                         int T, int R, int S, int sd, int sh, int sw,
                         int pf, int pt, int pl, int Do, int Ho, int Wo,
                         int k_pad, int act, int groups, int dh, int dw);
// 3-D transposed conv (K_CONV's 24-int form; Conv3DBackpropInputV2),
// NDHWC: y[N,Do,Ho,Wo,Kc] = act(sum x[n,i,j,l,ci] * w[t,r,s,co,ci] + bias
// [+ residual]) over od = i*sd - pf + t, oh = j*sh - pt + r,
// ow = l*sw - pl + s, with (pf, pt, pl) the low pads of the forward conv
// and x = [N,D,H,W,C]. One launch of a phase-split implicit GEMM: phase
// (pd,ph,pw) = ((od+pf) % sd, ...) is a stride-1 conv over x with the taps
// t = pd + sd*a, a < A(pd) = ceil((T - pd)/sd), so no inserted zero is
// multiplied. w is [Kc][k_pad]: taps phase-major ((pd,ph,pw) row-major),
// inside a phase ordered (a',b',c') with a' = A-1-a, channels innermost.
// A phase's K range starts at a multiple of C and is walked in tiles of 64,
// so when C % 64 != 0 its last tile runs past its last tap; the row holds
// all-zero taps after the T*R*S real ones until the last tile of every
// phase ends inside it, and k_pad = pad64(taps * C). Throws before any
// launch on a k_pad that is not that, on C % 8 != 0, on any extent or
// stride < 1, a negative pad, and on M or k beyond int32.
void launch_conv3d_transpose_igemm(hipStream_t s, const ushort* x,
                                   const ushort* w, const ushort* bias,
                                   const ushort* residual,
                                   const ushort* zeros, ushort* y,
                                   int N, int D, int H, int W, int C, int Kc,
                                   int T, int R, int S, int sd, int sh,
                                   int sw, int pf, int pt, int pl, int Do,
                                   int Ho, int Wo, int k_pad, int act);
// dead-tap skipping of the dilated kernel: 0 never, 1 where it pays
// (default: more than one block per CU and a filter reach of at least an
// eighth of the image), 2 wherever C % 64 == 0. A measurement switch
// (scripts/dilated_conv_probe.py)
int conv_dilated_skip();
void set_conv_dilated_skip(int mode);

// im2col for NHWC conv: out[N*Ho*Wo, K_pad] where the first R*S*C columns
// hold the patch elements (r,s,c order, c fastest) and columns >= R*S*C
// are zero (K_pad is the GEMM's 64-multiple). Out-of-image patch elements
// are zero. The conv then runs as launch_gemm with pre-transposed weights
// [Kc][K_pad].
void launch_im2col(hipStream_t s, const ushort* x, ushort* y,
                   int N, int H, int W, int C, int R, int S,
                   int sh, int sw, int pt, int pl, int Ho, int Wo,
                   int k_pad);

// Depthwise NHWC conv (MobileNet-class). With depth_multiplier == 1:
//   y[n,ho,wo,c] = act(sum_{r,s} x[n, ho*sh-pt+r, wo*sw-pl+s, c] * w[r,s,c]
//                      + bias[c])
// Memory-bound (no MFMA shape): vectorized 4x bf16 over the contiguous
// channel dim, grid-stride over N*Ho*Wo*C/4. w is the [R,S,C,1] master
// read as flat [R*S*C].
// mult > 1 is the depth multiplier M (K_DEPTHWISE's optional 14th int):
// C stays the INPUT channel count, and w [R,S,C*M], bias [C*M] and
// y [N,Ho,Wo,C*M] are indexed by k = c*M + m (the TF [R,S,C,M] filter
// read flat), output channel k reading input channel k / M:
//   y[n,ho,wo,k] = act(sum_{r,s} x[n, ho*sh-pt+r, wo*sw-pl+s, k/M]
//                      * w[r,s,k] + bias[k])
// 8 output channels (16 bytes) per thread when (C*M) % 8 == 0 and
// M in {2,4} or M % 8 == 0, one output element per thread otherwise.
// mult == 1 runs exactly the kernels described above. Throws on
// mult < 1 before any launch.
// (dh, dw) != (1, 1) with mult == 1 is the atrous separable case
// (K_DEPTHWISE's optional 15th and 16th ints): tap (r, s) reads
// hi = ho*sh - pt + r*dh, wi = wo*sw - pl + s*dw, 8 channels per thread
// when C % 8 == 0, one output element per thread otherwise. Throws before
// any launch on dh < 1 or dw < 1 and on a dilation with mult > 1.
void launch_depthwise_conv(hipStream_t s, const ushort* x, const ushort* w,
                           const ushort* bias, ushort* y,
                           int N, int H, int W, int C, int R, int S,
                           int sh, int sw, int pt, int pl, int Ho, int Wo,
                           int act, int mult = 1, int dh = 1, int dw = 1);

// NHWC image resize with TF's coordinate rules (ResizeNearestNeighbor /
// ResizeBilinear): mode 0 = nearest, 1 = bilinear. The per-axis scale is
// (in-1)/(out-1) when align_corners and out > 1, else in/out, computed
// here in f32 and passed to the kernel. Bilinear lerps in f32 and rounds
// to bf16 once. 16-byte vector path when C % 8 == 0. Throws on
// non-positive dims, an unknown mode, or both flags set.
void launch_resize_nhwc(hipStream_t s, const ushort* x, ushort* y, int N,
                        int H, int W, int C, int Ho, int Wo, int mode,
                        bool align_corners, bool half_pixel_centers);

// Zero-insertion (transposed-conv input dilation):
//   y[n, i*sh, j*sw, c] = x[n,i,j,c], every other element 0, with
//   y [N, (h-1)*sh+1, (w-1)*sw+1, C]. Writes all of y in one pass.
void launch_zero_insert_nhwc(hipStream_t s, const ushort* x, ushort* y,
                             int N, int h, int w, int C, int sh, int sw);

// fp8 (OCP e4m3) GEMM with rowwise dequant in the f32 epilogue:
// C[M,N] = act(acc(Aq @ Bq^T) * sa[m] * sb[n] + bias [+ residual]).
// Aq/Bq are e4m3 bytes with K padded to a multiple of 128; B^T layout
// [N][Kp] like launch_gemm's pre-transposed weights. 2x the bf16 MFMA
// rate on gfx950 (profiles/fp8_groundwork.md).
void launch_gemm_fp8(hipStream_t s, const uint8_t* A, const float* sa,
                     const uint8_t* B, const float* sb,
                     const ushort* bias, const ushort* residual,
                     ushort* C, int64_t M, int64_t N, int64_t K,
                     int act);

// rowwise activation quantization for the fp8 GEMM: bf16 [M,K] ->
// e4m3 [M,Kp] (zero-padded) + f32 amax/448 scale per row
void launch_quant_rowwise(hipStream_t s, const ushort* x, uint8_t* q,
                          float* scales, int64_t M, int64_t K,
                          int64_t Kp);

// Fused multi-head attention over the natural [B*S, H*D] QKV layout
// (flash-style online softmax; D must be 64 or 128, anything else
// throws). See ops/attention.hip.
// bias (nullable, bf16) is added to the scaled scores before the
// softmax, read as bias[b*sb + h*sh + q*sq + kv] with strides in
// elements; a 0 stride broadcasts that dimension ([B,1,1,S] key
// padding: sb=S; [1,1,S,S] causal: sq=S). A null bias launches the
// unmasked kernels.
void launch_attention(hipStream_t s, const ushort* Q, const ushort* K,
                      const ushort* V, ushort* O, int B, int S, int H,
                      int D_, float scale, const ushort* bias = nullptr,
                      int64_t bias_sb = 0, int64_t bias_sh = 0,
                      int64_t bias_sq = 0);

// Fused LSTM over a whole sequence (TF BlockLSTM / BlockLSTMV2, K_LSTM),
// ops/lstm.hip. With the gates in the order (i, ci, f, o):
//   z = pre[t, b] + h_{t-1} W_h
//   i = s(z_i + c wci), f = s(z_f + c wcf), g = tanh(z_ci)
//   c' = g i + c f, clamped to +-clip when clip > 0
//   o = s(z_o + c' wco), h = o tanh(c')
// `pre` is x W_x + b for every row, bf16 [rows][N], N = 64 * ceil(H / 16),
// row (t, b) at row t * pre_t + b * pre_b. Column
// (j / 16) * 64 + (j % 16) * 4 + gate holds that gate of unit j; columns of
// units >= H are zero. W_h is [N][pad64(H)] in the same column order, K
// zero-padded. wci / wcf / wco are [H] (all three or none), h0 / c0 [B][H]
// (null: zero state). h and the optional cs are bf16, row (t, b) at element
// t * st_t + b * st_b. The cell state stays f32 for the whole sequence; h
// is rounded to bf16 once per step and that value is the next step's
// operand. cstate is an f32 [B][H] scratch, re-initialised by every call.
// H <= lstm_resident_max_h() runs one launch (one workgroup per 16 batch
// rows, W_h resident in LDS); anything larger runs one launch per step.
// Throws before any launch on T, B or H < 1, on a null pre, W_h, h or
// cstate, on a partial peephole triple, and on strides that fail a
// sufficient no-overlap test: with the axes ordered by stride, the smaller
// one >= H and the larger one >= (n_small - 1) * small + H (time-major and
// batch-major layouts pass; other interleavings are refused).
void launch_lstm(hipStream_t s, const ushort* pre, const ushort* wh,
                 const ushort* wci, const ushort* wcf, const ushort* wco,
                 const ushort* h0, const ushort* c0, float* cstate,
                 ushort* h, ushort* cs, int64_t T, int64_t B, int64_t H,
                 int64_t st_t, int64_t st_b, int64_t pre_t, int64_t pre_b,
                 float clip);
// largest H served by the resident kernel. The default is what the LDS a
// workgroup may allocate holds (W_h plus two h buffers, one 16-unit tile
// per wave, at most 8 waves); set 0 to force the stepped kernel, a negative
// value to restore the default. A measurement switch
// (scripts/lstm_probe.py)
int lstm_resident_max_h();
void set_lstm_resident_max_h(int h);

// Per-class non-max suppression (TF CombinedNonMaxSuppression, K_NMS),
// ops/nms.hip. Boxes are bf16 [B, N, q, 4] with q = 1 (shared by the
// classes) or C, rows [y1, x1, y2, x2], 8-byte aligned.
//
// select: scores_cm is bf16 [B, C, N] (class-major). For every (image,
// class) the boxes with score > score_thr (NaN fails) are visited by
// descending score, equal scores (+0.0 == -0.0) by lower box index; one is
// kept unless its IoU with a box kept earlier exceeds iou_thr, until P are
// kept. IoU is f32: corners min/max-normalised, area <= 0 gives 0, else
// inter / (a_i + a_j - inter), correctly rounded. The r-th kept box's
// score bits go to cls_score[b, c * P + r] and its box index to cls_idx;
// unused slots hold -inf and 0. One launch, one workgroup per (image,
// class), nothing returns to the host.
//
// gather: slot / val [B, k] are the top-k of cls_score over its C * P
// slots. Row m < k whose value is not -inf becomes box (clipped to [0, 1]
// when clip), score and class slot / P as bf16; every other row of the M
// is zeros; out_valid[b] counts the former.
//
// Both throw before any launch unless 1 <= N <= 2^19, C >= 1, q is 1 or C,
// 1 <= P <= N, 0 <= iou_thr <= 1, 1 <= k <= min(M, C * P), clip is 0 or 1,
// every pointer is set and the boxes are 8-byte aligned.
void launch_nms_select(hipStream_t s, const ushort* scores_cm,
                       const ushort* boxes, ushort* cls_score, int* cls_idx,
                       int64_t B, int64_t N, int64_t C, int64_t q, int64_t P,
                       float iou_thr, float score_thr);
void launch_nms_gather(hipStream_t s, const int* slot, const ushort* val,
                       const int* cls_idx, const ushort* boxes,
                       ushort* out_boxes, ushort* out_scores,
                       ushort* out_classes, int* out_valid, int64_t B,
                       int64_t N, int64_t C, int64_t q, int64_t P, int64_t k,
                       int64_t M, int64_t clip);
// classes with at most this many candidates (<= 8192) run the greedy loop
// out of LDS, the others stream scores and boxes from L2 under an LDS alive
// mask; a measurement switch (scripts/nms_probe.py)
int nms_lds_candidates();
void set_nms_lds_candidates(int n);

}  // namespace tfsc
