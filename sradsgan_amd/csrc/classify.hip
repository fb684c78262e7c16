// Scene-classification evaluation of SR outputs (sradsgan_amd/classify.py; the reference's Scene_classification_mfe.py).
//   cls_channel_sums_*   uint8 NHWC -> per-image per-channel sums as 64-bit integers, two stages, no float anywhere
//   cls_preprocess       uint8 -> fp32 NHWC, (float(x) - mean_c) * fp32(1/255): Keras applies the function first, the rescale second
//   cls_dense_fwd_*      y[m][N] = x[m][K] W[K][N] + b (+ ReLU, + dropout): the classifier head, m <= 64 rows per call
//   cls_dense_wgrad      dW[K][N] = x^T dy, db = column sums of dy
//   cls_dense_dgrad      dx[m][K] = dy W^T (+ the backward of ReLU and dropout): layer 2 into layer 1 only, so K is small
//   cls_softmax_ce_*     one wave per row over C <= 64 classes; loss per row in fp32, batch sum in fp64 in a fixed order
//   cls_confusion        first-index arg-max per row, counted into an int32 [C][C] table
//
// The dense kernels are exact fp32 whatever srhip_set_conv_math says: two SR models are compared on identical classifier
// arithmetic.  The forward is a skinny GEMM that streams W once (33.5 MB at K = 32768, N = 256).  At m = 64 it is balanced:
// 1.07 GFLOP against 33.5 MB is 32 FLOP per byte, where the chip offers ~25 (fp32 peak / HBM peak).  The fp32 VALU and the
// fp32-input MFMA have the same peak, but the MFMA takes one VGPR per operand and no broadcast of the 64 x-rows across lanes, so
// it reaches that peak from a plain loop where a VALU kernel needs an LDS-staged x and 64 accumulator chains per lane: the
// forward and the weight gradient use v_mfma_f32_32x32x2_f32.  Every output is one chain of fused multiply-adds in a FIXED order,
// so results are reproducible -- but the order is not ascending k: within an 8-step the two lane halves alternate (kb, kb + 4,
// kb + 1, kb + 5, ...), and the four waves' 128-long sums are then added through LDS.  A host reference cannot reproduce the bits
// by summing in k order.  The data gradient is a few MFLOP and stays on fmaf.  Split-K: a block owns a 512-long K chunk of a 64-column panel, its four
// waves own 128-long slices and meet through LDS in wave order, the block writes one partial slab, and a second launch adds the
// slabs in chunk order with the bias, ReLU and dropout -- no atomics, no in-launch hand-off between blocks.
//
// Dropout is counter-based: keep(seed, step, e) = Philox4x32-10(counter = {e lo, e hi, step lo, step hi}, key = {seed lo,
// seed hi}).x < 2^31, e = row * N + column of the layer's output.  Kept values are doubled (inverted scaling at rate 0.5).  The
// backward recomputes the function; no mask is stored.
#include "common.h"
#include "philox.h"

namespace srhip {

// ---- Philox4x32-10 (philox.h): dropout reads the first word ----
__device__ __forceinline__ bool dropout_keep(unsigned long long seed, unsigned long long step, unsigned long long e) {
  return philox_first((unsigned)e, (unsigned)(e >> 32), (unsigned)step, (unsigned)(step >> 32), (unsigned)seed,
                      (unsigned)(seed >> 32)) < 0x80000000u;
}

// ---- channel sums ------------------------------------------------------------------------------------------------------ //
constexpr int CS_MAXC = 4;

// grid (segs, n): block (seg, img) sums the pixels seg*256 + t, stride segs*256, of image img.  A thread adds at most
// ceil(hw / (segs * 256)) <= 2^15 bytes per channel (the host bounds hw and sizes segs), so 32 bits hold every partial.
__global__ void cls_channel_sums_stage1(const unsigned char* __restrict__ img, unsigned long long* __restrict__ part, long hw, int c) {
  __shared__ unsigned red[4][CS_MAXC];
  const int segs = gridDim.x;
  const unsigned char* base = img + (long)blockIdx.y * hw * c;
  unsigned acc[CS_MAXC] = {0u, 0u, 0u, 0u};
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < hw; p += (long)segs * 256) {
    const unsigned char* q = base + p * c;
#pragma unroll
    for (int ch = 0; ch < CS_MAXC; ++ch)
      if (ch < c) acc[ch] += q[ch];
  }
#pragma unroll
  for (int ch = 0; ch < CS_MAXC; ++ch) {
    unsigned v = acc[ch];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);   // <= 64 * 2^15 * 255 < 2^32
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][ch] = v;
  }
  __syncthreads();
  if (threadIdx.x < CS_MAXC)
    part[((long)blockIdx.y * segs + blockIdx.x) * CS_MAXC + threadIdx.x] =
        (unsigned long long)red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

__global__ void cls_channel_sums_stage2(const unsigned long long* __restrict__ part, long long* __restrict__ sums, int n, int segs,
                                        int c) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * c) return;
  const int img = idx / c, ch = idx % c;
  unsigned long long s = 0;
  for (int k = 0; k < segs; ++k) s += part[((long)img * segs + k) * CS_MAXC + ch];
  sums[idx] = (long long)s;
}

inline int cs_segments(long hw) {
  long s = (hw + 4095) / 4096;
  return (int)(s < 1 ? 1 : (s > 256 ? 256 : s));
}

// ---- preprocess -------------------------------------------------------------------------------------------------------- //
__global__ void cls_preprocess_kernel(const unsigned char* __restrict__ img, const float* __restrict__ means, float* __restrict__ out,
                                      long count, int c) {
  const float inv255 = (float)(1.0 / 255.0);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (long)gridDim.x * blockDim.x) {
    const float d = (float)img[i] - means[(int)(i % c)];     // a subtraction then a product: nothing to contract into an fma
    out[i] = d * inv255;
  }
}

// ---- dense forward ----------------------------------------------------------------------------------------------------- //
constexpr int DENSE_CHUNK = 512;   // K per block
constexpr int DENSE_SLICE = 128;   // K per wave
constexpr int DENSE_MAXM = 64;

// grid (chunks, ceil(N / 64)), 256 threads.  Wave v of block (ch, pn) contracts k in [ch*512 + v*128, +128) for the rows 0..63 and
// the columns pn*64 .. pn*64+63.  One MFMA sums two k: lane half 0 carries k0..k0+3 over four MFMAs, half 1 carries k0+4..k0+7
// (A and B agree on that, which is all the instruction asks).  Rows >= m and columns >= N are loaded as zeros and never stored.
__global__ void __launch_bounds__(256) cls_dense_fwd_partial(const float* __restrict__ x, const float* __restrict__ w,
                                                             float* __restrict__ part, int m, int k, int n) {
  __shared__ float red[4][64][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 31, hf = lane >> 5;
  const int n0 = blockIdx.y * 64;
  const int kbeg = blockIdx.x * DENSE_CHUNK + wave * DENSE_SLICE;
  const int kend = min(kbeg + DENSE_SLICE, k);
  const bool two_rows = m > 32;                    // uniform
  const bool two_cols = n0 + 32 < n;               // uniform
  const bool r0 = i < m, r1 = i + 32 < m;
  const bool c0 = n0 + i < n, c1 = n0 + 32 + i < n;
  const float* x0 = x + (long)i * k + 4 * hf;
  const float* x1 = x + (long)(i + 32) * k + 4 * hf;
  const float* wc = w + n0 + i;
  f32x16 a00 = {0}, a01 = {0}, a10 = {0}, a11 = {0};
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  for (int kb = kbeg; kb < kend; kb += 8) {        // k % 8 == 0 (host): a step is inside [0, k) as a whole
    const f32x4 xa = r0 ? *reinterpret_cast<const f32x4*>(x0 + kb) : zero4;
    const f32x4 xb = (two_rows && r1) ? *reinterpret_cast<const f32x4*>(x1 + kb) : zero4;
    float b0[4], b1[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const long row = (long)(kb + 4 * hf + s) * n;
      b0[s] = c0 ? wc[row] : 0.f;
      b1[s] = (two_cols && c1) ? wc[row + 32] : 0.f;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      a00 = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[s], b0[s], a00, 0, 0, 0);
      if (two_cols) a01 = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[s], b1[s], a01, 0, 0, 0);
      if (two_rows) {
        a10 = __builtin_amdgcn_mfma_f32_32x32x2f32(xb[s], b0[s], a10, 0, 0, 0);
        if (two_cols) a11 = __builtin_amdgcn_mfma_f32_32x32x2f32(xb[s], b1[s], a11, 0, 0, 0);
      }
    }
  }
  // C/D of the 32x32 forms: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * hf;
    red[wave][row][i] = a00[r];
    red[wave][row][i + 32] = a01[r];
    red[wave][row + 32][i] = a10[r];
    red[wave][row + 32][i + 32] = a11[r];
  }
  __syncthreads();
  float* slab = part + (long)blockIdx.x * m * n;
  for (int e = threadIdx.x; e < 64 * 64; e += 256) {
    const int row = e >> 6, col = e & 63;
    if (row < m && n0 + col < n)
      slab[(long)row * n + n0 + col] = ((red[0][row][col] + red[1][row][col]) + red[2][row][col]) + red[3][row][col];
  }
}

// y = sum of the slabs in chunk order + bias, ReLU, dropout
__global__ void cls_dense_fwd_finish(const float* __restrict__ part, const float* __restrict__ bias, float* __restrict__ y, int chunks,
                                     int m, int n, int relu, int dropout, unsigned long long seed, unsigned long long step) {
  const long total = (long)m * n;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  float v = part[e];
  for (int c = 1; c < chunks; ++c) v += part[(long)c * total + e];
  if (bias) v += bias[(int)(e % n)];
  if (relu) v = v < 0.f ? 0.f : v;                       // lets a NaN through like ATen's ReLU (fmaxf would return 0)
  if (dropout) v = dropout_keep(seed, step, (unsigned long long)e) ? 2.f * v : 0.f;
  y[e] = v;
}

// ---- dense weight gradient --------------------------------------------------------------------------------------------- //
// grid (ceil(K / 32), ceil(N / 128)), 256 threads: wave v owns the 32 x 32 tile dW[k0 .. k0+31][n0 .. n0+31], n0 = (blockIdx.y * 4
// + v) * 32, contracted over the m <= 64 rows two at a time in row order.  No block-level synchronisation: a wave outside N leaves.
__global__ void __launch_bounds__(256) cls_dense_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                              float* __restrict__ dw, int m, int k, int n) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 31, hf = lane >> 5;
  const int k0 = blockIdx.x * 32, n0 = (blockIdx.y * 4 + wave) * 32;
  if (n0 >= n) return;
  const bool kin = k0 + i < k, cin = n0 + i < n;
  f32x16 acc = {0};
  for (int r = hf; r < ((m + 1) & ~1); r += 2) {
    const bool rin = r < m;
    const float a = (rin && kin) ? x[(long)r * k + k0 + i] : 0.f;
    const float b = (rin && cin) ? dy[(long)r * n + n0 + i] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = k0 + (r & 3) + 8 * (r >> 2) + 4 * hf;
    if (row < k && cin) dw[(long)row * n + n0 + i] = acc[r];
  }
}

__global__ void cls_colsum_kernel(const float* __restrict__ dy, float* __restrict__ db, int m, int n) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  float s = 0.f;
  for (int r = 0; r < m; ++r) s += dy[(long)r * n + c];
  db[c] = s;
}

// ---- dense data gradient ----------------------------------------------------------------------------------------------- //
// dx[r][j] = sum_c dy[r][c] W[j][c] in class order (fmaf), then the backward of the producing layer's ReLU (act = that layer's
// output: > 0 where the pre-activation was, wherever the element was kept) and of its dropout (the mask recomputed).
__global__ void cls_dense_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w, const float* __restrict__ act,
                                       float* __restrict__ dx, int m, int k, int n, int relu, int dropout, unsigned long long seed,
                                       unsigned long long step) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)m * k) return;
  const int r = (int)(e / k), j = (int)(e % k);
  const float* d = dy + (long)r * n;
  const float* wr = w + (long)j * n;
  float v = 0.f;
  for (int c = 0; c < n; ++c) v = fmaf(d[c], wr[c], v);
  if (dropout) v = dropout_keep(seed, step, (unsigned long long)e) ? 2.f * v : 0.f;
  if (relu && !(act[e] > 0.f)) v = 0.f;
  dx[e] = v;
}

// ---- softmax + cross-entropy ------------------------------------------------------------------------------------------- //
// One wave per row, lane c holds class c.  z - max, exp, butterfly sum (a fixed order), log-softmax; no probability clipping.
__global__ void cls_softmax_ce_kernel(const float* __restrict__ logits, const int* __restrict__ labels, float* __restrict__ row_loss,
                                      float* __restrict__ dlogits, int m, int c, float scale) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= m) return;                                   // whole waves leave: the shuffles below see full waves
  const bool in = lane < c;
  const float z = in ? logits[(long)row * c + lane] : -INFINITY;
  const float mx = wave_max(z);
  const float x = z - mx;
  const float e = in ? expf(x) : 0.f;
  const float s = wave_sum(e);
  const float logp = x - logf(s);
  const int label = labels[row];
  const bool valid = label >= 0 && label < c;
  const float lp = __shfl(logp, valid ? label : 0, 64);
  if (lane == 0) row_loss[row] = valid ? -lp : 0.f;
  if (dlogits && in) dlogits[(long)row * c + lane] = (e / s - ((valid && lane == label) ? 1.f : 0.f)) * scale;
}

// fp64 sum of the row losses: lane l adds rows l, l + 64, ... in order, then a butterfly
__global__ void cls_loss_sum_kernel(const float* __restrict__ row_loss, double* __restrict__ out, int m) {
  double s = 0.0;
  for (int r = threadIdx.x; r < m; r += 64) s += (double)row_loss[r];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (threadIdx.x == 0) out[0] = s;
}

// ---- arg-max and confusion counts ---------------------------------------------------------------------------------------- //
__global__ void cls_confusion_kernel(const float* __restrict__ logits, const int* __restrict__ labels, int* __restrict__ pred,
                                     int* __restrict__ table, int m, int c) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= m) return;
  const float* z = logits + (long)row * c;
  float best = z[0];
  int arg = 0;
  for (int j = 1; j < c; ++j)
    if (pool_takes(z[j], best)) {                         // strict: the first maximum wins; a NaN logit is the maximum, as in torch.argmax
      best = z[j];
      arg = j;
    }
  if (pred) pred[row] = arg;
  if (table && labels) {
    const int t = labels[row];
    if (t >= 0 && t < c) atomicAdd(&table[t * c + arg], 1);   // integer adds: the counts do not depend on arrival order
  }
}

}  // namespace srhip

using namespace srhip;

extern "C" {

size_t srhip_cls_channel_sums_workspace(int n, int h, int w) {
  if (n <= 0 || h <= 0 || w <= 0) return 0;
  return (size_t)n * cs_segments((long)h * w) * CS_MAXC * sizeof(unsigned long long);
}

int srhip_cls_channel_sums(const unsigned char* img, long long* sums, void* workspace, size_t workspace_bytes, int n, int h, int w,
                           int c, void* stream) {
  SRHIP_REQUIRE(img && sums && workspace, "cls_channel_sums: null tensor");
  SRHIP_REQUIRE(n > 0 && n <= 65535 && h > 0 && w > 0 && c >= 1 && c <= CS_MAXC, "cls_channel_sums: bad size n %d, %d x %d x %d", n, h,
                w, c);
  const long hw = (long)h * w;
  SRHIP_REQUIRE(hw <= (1L << 31), "cls_channel_sums: image too large");
  SRHIP_REQUIRE(workspace_bytes >= srhip_cls_channel_sums_workspace(n, h, w) && ((size_t)workspace & 7) == 0,
                "cls_channel_sums: workspace too small or misaligned");
  const int segs = cs_segments(hw);
  hipLaunchKernelGGL(cls_channel_sums_stage1, dim3(segs, n), dim3(256), 0, as_stream(stream), img, (unsigned long long*)workspace, hw,
                     c);
  hipLaunchKernelGGL(cls_channel_sums_stage2, dim3(cdiv((long)n * c, 64)), dim3(64), 0, as_stream(stream),
                     (const unsigned long long*)workspace, sums, n, segs, c);
  return check_launch("cls_channel_sums");
}

int srhip_cls_preprocess(const unsigned char* img, const float* means_dev, float* out, long count, int c, void* stream) {
  SRHIP_REQUIRE(img && means_dev && out, "cls_preprocess: null tensor");
  SRHIP_REQUIRE(count > 0 && c >= 1 && count % c == 0, "cls_preprocess: %ld elements are no multiple of %d channels", count, c);
  const long blocks = (count + 255) / 256;
  hipLaunchKernelGGL(cls_preprocess_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, as_stream(stream), img,
                     means_dev, out, count, c);
  return check_launch("cls_preprocess");
}

int srhip_cls_dense_chunks(int k) { return k > 0 ? cdiv(k, DENSE_CHUNK) : 0; }

int srhip_cls_dense_fwd(const float* x, const float* w, const float* bias, float* y, float* partials, size_t partial_bytes, int m,
                        int k, int n, int relu, int dropout, unsigned long long seed, unsigned long long step, void* stream) {
  SRHIP_REQUIRE(x && w && y && partials, "cls_dense_fwd: null tensor");
  SRHIP_REQUIRE(m >= 1 && m <= DENSE_MAXM && k >= 8 && k % 8 == 0 && n >= 1 && n <= 65535 * 64,
                "cls_dense_fwd: needs 1 <= m <= 64, k a positive multiple of 8, n >= 1 (got m %d, k %d, n %d)", m, k, n);
  SRHIP_REQUIRE(((size_t)x & 15) == 0, "cls_dense_fwd: x must be 16-byte aligned");
  const int chunks = srhip_cls_dense_chunks(k);
  SRHIP_REQUIRE(partial_bytes >= (size_t)chunks * m * n * sizeof(float), "cls_dense_fwd: partial buffer too small");
  hipLaunchKernelGGL(cls_dense_fwd_partial, dim3(chunks, cdiv(n, 64)), dim3(256), 0, as_stream(stream), x, w, partials, m, k, n);
  hipLaunchKernelGGL(cls_dense_fwd_finish, dim3(cdiv((long)m * n, 256)), dim3(256), 0, as_stream(stream), (const float*)partials, bias, y,
                     chunks, m, n, relu, dropout, seed, step);
  return check_launch("cls_dense_fwd");
}

int srhip_cls_dense_wgrad(const float* x, const float* dy, float* dw, float* db, int m, int k, int n, void* stream) {
  SRHIP_REQUIRE(x && dy && dw, "cls_dense_wgrad: null tensor");
  SRHIP_REQUIRE(m >= 1 && m <= DENSE_MAXM && k >= 1 && n >= 1 && cdiv(n, 128) <= 65535,
                "cls_dense_wgrad: needs 1 <= m <= 64, k >= 1, n >= 1 (got m %d, k %d, n %d)", m, k, n);
  hipLaunchKernelGGL(cls_dense_wgrad_kernel, dim3(cdiv(k, 32), cdiv(n, 128)), dim3(256), 0, as_stream(stream), x, dy, dw, m, k, n);
  if (db) hipLaunchKernelGGL(cls_colsum_kernel, dim3(cdiv(n, 64)), dim3(64), 0, as_stream(stream), dy, db, m, n);
  return check_launch("cls_dense_wgrad");
}

int srhip_cls_dense_dgrad(const float* dy, const float* w, const float* act, float* dx, int m, int k, int n, int relu, int dropout,
                          unsigned long long seed, unsigned long long step, void* stream) {
  SRHIP_REQUIRE(dy && w && dx && (act || !relu), "cls_dense_dgrad: null tensor");
  SRHIP_REQUIRE(m >= 1 && k >= 1 && n >= 1 && (long)m * k / 256 < 0x7fffffffL, "cls_dense_dgrad: bad size m %d, k %d, n %d", m, k, n);
  hipLaunchKernelGGL(cls_dense_dgrad_kernel, dim3(cdiv((long)m * k, 256)), dim3(256), 0, as_stream(stream), dy, w, act, dx, m, k, n,
                     relu, dropout, seed, step);
  return check_launch("cls_dense_dgrad");
}

int srhip_cls_softmax_ce_fwd_bwd(const float* logits, const int* labels, float* row_loss, double* loss_sum, float* dlogits, int m,
                                 int c, float scale, void* stream) {
  SRHIP_REQUIRE(logits && labels && row_loss && loss_sum, "cls_softmax_ce: null tensor");
  SRHIP_REQUIRE(m >= 1 && c >= 1 && c <= 64, "cls_softmax_ce: needs m >= 1 and 1 <= classes <= 64 (got m %d, c %d)", m, c);
  hipLaunchKernelGGL(cls_softmax_ce_kernel, dim3(cdiv(m, 4)), dim3(256), 0, as_stream(stream), logits, labels, row_loss, dlogits, m, c,
                     scale);
  hipLaunchKernelGGL(cls_loss_sum_kernel, dim3(1), dim3(64), 0, as_stream(stream), (const float*)row_loss, loss_sum, m);
  return check_launch("cls_softmax_ce");
}

int srhip_cls_confusion(const float* logits, const int* labels, int* pred, int* table, int m, int c, void* stream) {
  SRHIP_REQUIRE(logits && (pred || (table && labels)), "cls_confusion: null tensor");
  SRHIP_REQUIRE(m >= 1 && c >= 1 && c <= 32768, "cls_confusion: bad size m %d, c %d", m, c);
  hipLaunchKernelGGL(cls_confusion_kernel, dim3(cdiv(m, 256)), dim3(256), 0, as_stream(stream), logits, labels, pred, table, m, c);
  return check_launch("cls_confusion");
}

}  // extern "C"
