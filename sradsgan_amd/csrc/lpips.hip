// LPIPS (net-lin, AlexNet, v0.1) of the reference's validation loops (sradsgan.py:561, 1125-1132, 1326-1332;
// utils/PerceptualSimilarity/networks_basic.py:64-105, pretrained_networks.py:57-96), forward only (the metric runs under no_grad):
//   * the stem: scaling layer + AlexNet features[0:2] (conv 3->64 k11 s4 p2 + ReLU) in one pass,
//   * the 3x3 stride-2 max pool of features[2] and [5],
//   * the head of one tap: per-pixel channel normalisation of both images, squared difference, the learned 1x1 weights, pixel sums,
//   * the finish: partial sums -> mean over pixels per tap -> sum of the taps, per pair, in float64.
// AlexNet's convs 2-5 are ordinary srhip_conv2d_fwd calls (bias + ReLU epilogue).
#include "common.h"

namespace srhip {

// ---- stem --------------------------------------------------------------------------------------------------------------------------
// K = 363 on a 3-channel image: exact fp32 on the VALU (an fmaf chain per output, taps in (ky, kx, ci) order), like the project's other
// 3-channel kernels.  A block computes an 8 x 16 tile of output pixels for all 64 channels: the 39 x 71 x 3 input patch goes to LDS
// once with the affine applied (out-of-image taps stay 0: the conv pads in the scaled space), the weights one kernel row (33 x 64) at a
// time.  A thread owns one tile column (8 pixels) x 4 channels = 32 accumulators; per k it reads 8 patch words (4 addresses per wave,
// broadcast) and one float4 of weights (16 addresses per wave) for 32 FMAs.
constexpr int ST_TH = 8, ST_TW = 16, ST_K = 11, ST_S = 4, ST_P = 2, ST_CO = 64;
constexpr int ST_PH = (ST_TH - 1) * ST_S + ST_K, ST_PW = (ST_TW - 1) * ST_S + ST_K;     // 39 x 71
constexpr int ST_ROWK = ST_K * 3;                                                       // 33 (kx, ci) taps per kernel row

// ReLU that lets a NaN through like ATen's (fmaxf would return 0): a NaN image must not score a finite LPIPS
__device__ __forceinline__ float relu_nan(float v) { return v < 0.f ? 0.f : v; }

__global__ __launch_bounds__(256) void lpips_stem_kernel(const float* __restrict__ x, const float* __restrict__ w_hwio,
                                                         const float* __restrict__ bias, float* __restrict__ y, int h, int wd, int ho,
                                                         int wo, int normalize) {
  __shared__ float patch[ST_PH * ST_PW * 3];
  __shared__ __attribute__((aligned(16))) float wk[ST_ROWK * ST_CO];
  const int tid = threadIdx.x, n = blockIdx.z;
  const int oy0 = blockIdx.y * ST_TH, ox0 = blockIdx.x * ST_TW;
  const int iy0 = oy0 * ST_S - ST_P, ix0 = ox0 * ST_S - ST_P;
  const float shift[3] = {-.030f, -.088f, -.188f}, scale[3] = {.458f, .448f, .450f};   // networks_basic.py:101-102
  for (int e = tid; e < ST_PH * ST_PW * 3; e += 256) {
    const int pix = e / 3, ch = e - pix * 3;
    const int r = pix / ST_PW, c = pix - r * ST_PW;
    const int gy = iy0 + r, gx = ix0 + c;
    float v = 0.f;
    if (gy >= 0 && gy < h && gx >= 0 && gx < wd) {
      v = x[(((size_t)n * h + gy) * wd + gx) * 3 + ch];
      if (normalize) v = 2.f * v - 1.f;                                                  // PerceptualSimilarity/__init__.py:36-38
      v = (v - shift[ch]) / scale[ch];
    }
    patch[e] = v;
  }
  const int cg = tid & 15, col = tid >> 4;
  float acc[ST_TH][4];
#pragma unroll
  for (int r = 0; r < ST_TH; ++r) acc[r][0] = acc[r][1] = acc[r][2] = acc[r][3] = 0.f;
  for (int ky = 0; ky < ST_K; ++ky) {
    __syncthreads();                                    // the patch is complete (ky = 0) / the previous kernel row is consumed
    for (int e = tid; e < ST_ROWK * ST_CO / 4; e += 256)
      reinterpret_cast<float4*>(wk)[e] = reinterpret_cast<const float4*>(w_hwio + (size_t)ky * ST_ROWK * ST_CO)[e];
    __syncthreads();
    const float* prow = patch + (ky * ST_PW + col * ST_S) * 3;
#pragma unroll 3
    for (int k = 0; k < ST_ROWK; ++k) {
      const float4 wv = *reinterpret_cast<const float4*>(wk + k * ST_CO + cg * 4);
#pragma unroll
      for (int r = 0; r < ST_TH; ++r) {
        const float xv = prow[r * ST_S * ST_PW * 3 + k];
        acc[r][0] = fmaf(xv, wv.x, acc[r][0]);
        acc[r][1] = fmaf(xv, wv.y, acc[r][1]);
        acc[r][2] = fmaf(xv, wv.z, acc[r][2]);
        acc[r][3] = fmaf(xv, wv.w, acc[r][3]);
      }
    }
  }
  const int ox = ox0 + col;
  if (ox >= wo) return;
  const float4 b = *reinterpret_cast<const float4*>(bias + cg * 4);
#pragma unroll
  for (int r = 0; r < ST_TH; ++r) {
    const int oy = oy0 + r;
    if (oy < ho) {
      float4 o;
      o.x = relu_nan(acc[r][0] + b.x);
      o.y = relu_nan(acc[r][1] + b.y);
      o.z = relu_nan(acc[r][2] + b.z);
      o.w = relu_nan(acc[r][3] + b.w);
      *reinterpret_cast<float4*>(y + (((size_t)n * ho + oy) * wo + ox) * ST_CO + cg * 4) = o;
    }
  }
}

// ---- nn.MaxPool2d(kernel_size=3, stride=2): floor mode, no padding; a thread per output pixel and 4 channels ---------------------
__global__ __launch_bounds__(256) void maxpool3x3s2_kernel(const float* __restrict__ x, float* __restrict__ y, int h, int w, int c4,
                                                           int ho, int wo, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int cv = (int)(i % c4);
  long p = i / c4;
  const int ox = (int)(p % wo);
  p /= wo;
  const int oy = (int)(p % ho);
  const long n = p / ho;
  const float4* src = reinterpret_cast<const float4*>(x) + ((n * h + 2 * oy) * w + 2 * ox) * c4 + cv;
  float4 m = src[0];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      if (dy == 0 && dx == 0) continue;
      const float4 v = src[((long)dy * w + dx) * c4];
      if (pool_takes(v.x, m.x)) m.x = v.x;
      if (pool_takes(v.y, m.y)) m.y = v.y;
      if (pool_takes(v.z, m.z)) m.z = v.z;
      if (pool_takes(v.w, m.w)) m.w = v.w;
    }
  reinterpret_cast<float4*>(y)[i] = m;
}

// ---- head --------------------------------------------------------------------------------------------------------------------------
// 16 lanes per pixel: both feature vectors are read twice (norms, then the weighted squared difference of the normalised values; the
// maps are small and the second read hits the cache).  fp32 per channel as the reference's tensors are; the channel sum crosses the 16
// lanes in fp64 and pixel sums stay in fp64.  Deterministic: a fixed pixel -> thread map, a fixed tree, no atomics.
constexpr int LPIPS_BLOCKS = 32;

__device__ inline float group16_sum(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ inline double group16_sum(double v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void lpips_head_kernel(const float* __restrict__ f, const int* __restrict__ pairs,
                                                         const float* __restrict__ w, double* __restrict__ partial, long hw, int c4) {
  __shared__ double red[256];
  const int tid = threadIdx.x, lane = tid & 15, p = blockIdx.y;
  const float4* f0 = reinterpret_cast<const float4*>(f) + (size_t)pairs[2 * p] * hw * c4;
  const float4* f1 = reinterpret_cast<const float4*>(f) + (size_t)pairs[2 * p + 1] * hw * c4;
  const float4* wv = reinterpret_cast<const float4*>(w);
  double acc = 0.0;
  // every lane of a 16-lane group walks the same pixels, so the shuffles below always see whole groups
  for (long pix = (long)blockIdx.x * 16 + (tid >> 4); pix < hw; pix += (long)gridDim.x * 16) {
    const float4* a = f0 + pix * c4;
    const float4* b = f1 + pix * c4;
    float n0 = 0.f, n1 = 0.f;
    for (int j = lane; j < c4; j += 16) {
      const float4 u = a[j], v = b[j];
      n0 += u.x * u.x + u.y * u.y + u.z * u.z + u.w * u.w;
      n1 += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    const float d0 = sqrtf(group16_sum(n0)) + 1e-10f, d1 = sqrtf(group16_sum(n1)) + 1e-10f;   // eps after the root (__init__.py:42-44)
    float s = 0.f;
    for (int j = lane; j < c4; j += 16) {
      const float4 u = a[j], v = b[j], k = wv[j];
      const float ex = u.x / d0 - v.x / d1, ey = u.y / d0 - v.y / d1, ez = u.z / d0 - v.z / d1, ew = u.w / d0 - v.w / d1;
      s += k.x * (ex * ex) + k.y * (ey * ey) + k.z * (ez * ez) + k.w * (ew * ew);
    }
    acc += group16_sum((double)s);
  }
  red[tid] = lane == 0 ? acc : 0.0;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) partial[(size_t)p * gridDim.x + blockIdx.x] = red[0];
}

constexpr int LPIPS_MAX_TAPS = 8;
struct TapCounts {
  double hw[LPIPS_MAX_TAPS];
};

__global__ void lpips_finish_kernel(const double* __restrict__ partial, double* __restrict__ out, int ntaps, int npairs, TapCounts counts) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npairs) return;
  double total = 0.0;
  for (int t = 0; t < ntaps; ++t) {
    double s = 0.0;
    for (int j = 0; j < LPIPS_BLOCKS; ++j) s += partial[((size_t)t * npairs + p) * LPIPS_BLOCKS + j];
    total += s / counts.hw[t];
  }
  out[p] = total;
}

}  // namespace srhip

using namespace srhip;

extern "C" {

int srhip_lpips_stem(const float* x, const float* w_hwio, const float* bias, float* y, int m, int h, int w, int normalize, void* stream) {
  SRHIP_REQUIRE(x && w_hwio && bias && y, "lpips_stem: null tensor");
  SRHIP_REQUIRE(m > 0 && m <= 65535 && h >= 7 && w >= 7, "lpips_stem: needs 1 <= M <= 65535 and H, W >= 7");
  const int ho = (h + 2 * ST_P - ST_K) / ST_S + 1, wo = (w + 2 * ST_P - ST_K) / ST_S + 1;
  SRHIP_REQUIRE(cdiv(ho, ST_TH) <= 65535, "lpips_stem: image too tall");
  hipLaunchKernelGGL(lpips_stem_kernel, dim3(cdiv(wo, ST_TW), cdiv(ho, ST_TH), m), dim3(256), 0, as_stream(stream), x, w_hwio, bias, y, h,
                     w, ho, wo, normalize);
  return check_launch("lpips_stem");
}

int srhip_maxpool3x3s2_fwd(const float* x, float* y, int n, int h, int w, int c, void* stream) {
  SRHIP_REQUIRE(x && y, "maxpool3x3s2_fwd: null tensor");
  SRHIP_REQUIRE(n > 0 && c > 0 && c % 4 == 0 && h >= 3 && w >= 3, "maxpool3x3s2_fwd: needs C %% 4 == 0 and H, W >= 3");
  const int ho = (h - 3) / 2 + 1, wo = (w - 3) / 2 + 1;
  const long total = (long)n * ho * wo * (c / 4);
  SRHIP_REQUIRE(cdiv(total, 256) > 0, "maxpool3x3s2_fwd: tensor too large");
  hipLaunchKernelGGL(maxpool3x3s2_kernel, dim3(cdiv(total, 256)), dim3(256), 0, as_stream(stream), x, y, h, w, c / 4, ho, wo, total);
  return check_launch("maxpool3x3s2_fwd");
}

int srhip_lpips_blocks(void) { return LPIPS_BLOCKS; }

int srhip_lpips_head(const float* f, const int* pairs, const float* w, double* partial, int m, int npairs, int h, int wd, int c,
                     void* stream) {
  SRHIP_REQUIRE(f && pairs && w && partial, "lpips_head: null tensor");
  SRHIP_REQUIRE(m > 0 && npairs > 0 && npairs <= 65535 && h > 0 && wd > 0 && c > 0 && c % 4 == 0,
                "lpips_head: needs C %% 4 == 0 and 1 <= pairs <= 65535");
  hipLaunchKernelGGL(lpips_head_kernel, dim3(LPIPS_BLOCKS, npairs), dim3(256), 0, as_stream(stream), f, pairs, w, partial, (long)h * wd,
                     c / 4);
  return check_launch("lpips_head");
}

int srhip_lpips_finish(const double* partial, const long* tap_pixels, int ntaps, int npairs, double* out, void* stream) {
  SRHIP_REQUIRE(partial && tap_pixels && out, "lpips_finish: null pointer");
  SRHIP_REQUIRE(ntaps > 0 && ntaps <= LPIPS_MAX_TAPS && npairs > 0, "lpips_finish: needs 1 <= taps <= 8");
  TapCounts counts;
  for (int t = 0; t < LPIPS_MAX_TAPS; ++t) {
    counts.hw[t] = t < ntaps ? (double)tap_pixels[t] : 1.0;
    SRHIP_REQUIRE(counts.hw[t] > 0.0, "lpips_finish: empty tap");
  }
  hipLaunchKernelGGL(lpips_finish_kernel, dim3(cdiv(npairs, 64)), dim3(64), 0, as_stream(stream), partial, out, ntaps, npairs, counts);
  return check_launch("lpips_finish");
}

}  // extern "C"
