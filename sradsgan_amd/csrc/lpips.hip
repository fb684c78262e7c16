// LPIPS (net-lin, AlexNet, v0.1) of the reference's validation loops (sradsgan.py:561, 1125-1132, 1326-1332;
// utils/PerceptualSimilarity/networks_basic.py:64-105, pretrained_networks.py:57-96); the forward passes (the metric runs under no_grad):
//   * the stem: scaling layer + AlexNet features[0:2] (conv 3->64 k11 s4 p2 + ReLU) in one pass,
//   * the 3x3 stride-2 max pool of features[2] and [5],
//   * the head of one tap: per-pixel channel normalisation of both images, squared difference, the learned 1x1 weights, pixel sums,
//   * the finish: partial sums -> mean over pixels per tap -> sum of the taps, per pair, in float64.
// AlexNet's convs 2-5 are ordinary srhip_conv2d_fwd calls (bias + ReLU epilogue).
// As a loss (lpips.LPIPS.loss) the same chain runs backwards: the head, pool and stem backward kernels below, and srhip_conv2d_dgrad
// for convs 2-5.
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

// ---- backward: the taps and heads as a loss (lpips.LPIPS.loss) ---------------------------------------------------------------------
// Exact fp32, no atomics, one fixed summation order per output value, and nothing that crosses images: an image's gradient does not
// depend on what else is in the batch.

// Head backward of one tap, to the PRED feature map (the second index of each pair) and through that tap's ReLU.  With f the pred and t
// the target features of a pixel, n = sqrt(sum f^2), D = n + eps, e_c = f_c / D - t_c / D_t, q_c = 2 w_c e_c s, S = sum_c q_c f_c:
//   df_c = q_c / D - f_c S / (D^2 n), evaluated as (q_c - (S / D) (f_c / n)) / D so that no product of small norms underflows.
// s = upstream[0] * inv_count stays on the device.  f_c <= 0 writes 0 (a NaN feature fails the comparison and passes its NaN on, like
// ATen's threshold_backward); a pixel with n == 0 writes zeros without forming 0 / 0 (every channel is masked there; torch autograd
// yields NaN at such a pixel -- a deliberate departure).  The forward head's layout: 16 lanes per pixel, the same pixel -> thread map.
__global__ __launch_bounds__(256) void lpips_head_bwd_kernel(const float* __restrict__ f, const int* __restrict__ pairs,
                                                             const float* __restrict__ w, const float* __restrict__ upstream,
                                                             float inv_count, float* __restrict__ df, long hw, int c4) {
  const int tid = threadIdx.x, lane = tid & 15, p = blockIdx.y;
  const float4* ft = reinterpret_cast<const float4*>(f) + (size_t)pairs[2 * p] * hw * c4;
  const float4* fp = reinterpret_cast<const float4*>(f) + (size_t)pairs[2 * p + 1] * hw * c4;
  const float4* wv = reinterpret_cast<const float4*>(w);
  float4* out = reinterpret_cast<float4*>(df) + (size_t)p * hw * c4;
  const float s2 = 2.f * (upstream[0] * inv_count);
  for (long pix = (long)blockIdx.x * 16 + (tid >> 4); pix < hw; pix += (long)gridDim.x * 16) {
    const float4* a = fp + pix * c4;
    const float4* b = ft + pix * c4;
    float n0 = 0.f, n1 = 0.f;
    for (int j = lane; j < c4; j += 16) {
      const float4 u = a[j], v = b[j];
      n0 += u.x * u.x + u.y * u.y + u.z * u.z + u.w * u.w;
      n1 += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    const float nrm = sqrtf(group16_sum(n0));
    const float d0 = nrm + 1e-10f, d1 = sqrtf(group16_sum(n1)) + 1e-10f;
    if (nrm == 0.f) {                                    // group-uniform: all 16 lanes hold the same sum
      for (int j = lane; j < c4; j += 16) out[pix * c4 + j] = make_float4(0.f, 0.f, 0.f, 0.f);
      continue;
    }
    float sq = 0.f;
    for (int j = lane; j < c4; j += 16) {
      const float4 u = a[j], v = b[j], k = wv[j];
      const float qx = s2 * k.x * (u.x / d0 - v.x / d1), qy = s2 * k.y * (u.y / d0 - v.y / d1);
      const float qz = s2 * k.z * (u.z / d0 - v.z / d1), qw = s2 * k.w * (u.w / d0 - v.w / d1);
      sq += qx * u.x + qy * u.y + qz * u.z + qw * u.w;
    }
    const float r = group16_sum(sq) / d0;
    for (int j = lane; j < c4; j += 16) {
      const float4 u = a[j], v = b[j], k = wv[j];
      const float qx = s2 * k.x * (u.x / d0 - v.x / d1), qy = s2 * k.y * (u.y / d0 - v.y / d1);
      const float qz = s2 * k.z * (u.z / d0 - v.z / d1), qw = s2 * k.w * (u.w / d0 - v.w / d1);
      float4 o;
      o.x = u.x <= 0.f ? 0.f : (qx - r * (u.x / nrm)) / d0;
      o.y = u.y <= 0.f ? 0.f : (qy - r * (u.y / nrm)) / d0;
      o.z = u.z <= 0.f ? 0.f : (qz - r * (u.z / nrm)) / d0;
      o.w = u.w <= 0.f ? 0.f : (qw - r * (u.w / nrm)) / d0;
      out[pix * c4 + j] = o;
    }
  }
}

// Backward of nn.MaxPool2d(3, 2) in gather form, fused with what follows it here: dx = gather(dy) * [x > 0] + residual.  A thread owns
// one input pixel and 4 channels, visits the at most 2 x 2 windows that contain the pixel in ascending (oy, ox) order, recomputes each
// window's arg-max with the forward's scan (pool_takes: the first maximum wins) and adds that window's dy when the arg-max is its own
// position.  x is the pool's input (a ReLU output); relu != 0 applies its mask (x <= 0 writes 0, so a NaN passes the gradient on).
__global__ __launch_bounds__(256) void maxpool3x3s2_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                               const float* __restrict__ residual, float* __restrict__ dx, int h, int w,
                                                               int c4, int ho, int wo, int relu, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int cv = (int)(i % c4);
  long p = i / c4;
  const int ix = (int)(p % w);
  p /= w;
  const int iy = (int)(p % h);
  const long n = p / h;
  const float4* xs = reinterpret_cast<const float4*>(x);
  const float4* gs = reinterpret_cast<const float4*>(dy);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const int oy_lo = iy < 2 ? 0 : (iy - 1) / 2, oy_hi = min(iy / 2, ho - 1);
  const int ox_lo = ix < 2 ? 0 : (ix - 1) / 2, ox_hi = min(ix / 2, wo - 1);
  for (int oy = oy_lo; oy <= oy_hi; ++oy)
    for (int ox = ox_lo; ox <= ox_hi; ++ox) {
      const float4* src = xs + ((n * h + 2 * oy) * w + 2 * ox) * c4 + cv;
      const int mine = (iy - 2 * oy) * 3 + (ix - 2 * ox);
      float4 m = src[0];
      int ax = 0, ay = 0, az = 0, aw = 0;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          if (ky == 0 && kx == 0) continue;
          const float4 v = src[((long)ky * w + kx) * c4];
          const int at = ky * 3 + kx;
          if (pool_takes(v.x, m.x)) { m.x = v.x; ax = at; }
          if (pool_takes(v.y, m.y)) { m.y = v.y; ay = at; }
          if (pool_takes(v.z, m.z)) { m.z = v.z; az = at; }
          if (pool_takes(v.w, m.w)) { m.w = v.w; aw = at; }
        }
      const float4 g = gs[((n * ho + oy) * wo + ox) * c4 + cv];
      if (ax == mine) acc[0] += g.x;
      if (ay == mine) acc[1] += g.y;
      if (az == mine) acc[2] += g.z;
      if (aw == mine) acc[3] += g.w;
    }
  float4 o = make_float4(acc[0], acc[1], acc[2], acc[3]);
  if (relu) {
    const float4 v = xs[i];
    o.x = v.x <= 0.f ? 0.f : o.x;
    o.y = v.y <= 0.f ? 0.f : o.y;
    o.z = v.z <= 0.f ? 0.f : o.z;
    o.w = v.w <= 0.f ? 0.f : o.w;
  }
  if (residual) {
    const float4 r = reinterpret_cast<const float4*>(residual)[i];
    o.x += r.x;
    o.y += r.y;
    o.z += r.z;
    o.w += r.w;
  }
  reinterpret_cast<float4*>(dx)[i] = o;
}

// Data gradient of the stem back to the image, the scaling layer's factor included, in gather form.  With u = y + 2, image row y takes
// kernel rows ky = (u mod 4) + 4 j < 11 at output rows oy = (u - ky) / 4: at most 3 x 3 output positions x 64 channels = 576 fmaf in one
// chain per value, (oy, ox, co) ascending.  A block owns the 32 x 32 pixels with u, v in [32 b, 32 b + 32): they read a 10 x 10 tile of
// output positions, staged in LDS (zero outside the map) beside the whole [11][11][3][64] weight.  The phase (u mod 4, v mod 4) fixes
// the tap set, so a wave takes one row phase, a 16-lane group one column phase, and a thread the four pixels (A, B), (A + 4, B),
// (A, B + 4), (A + 4, B + 4) of its phase's 8 x 8 grid with all 3 channels: 12 chains share every weight vector.
// LDS banks (ds_read_b128, 16-lane groups {0-3, 12-15, 20-27}, ...: each holds all 16 (A, B) once): a tile position is 68 floats and a
// tile row 12 positions, so the 16 positions A * 12 + B fall on 16 different 16-byte slots; a weight tap is 3 * 64 + 4 floats, so the
// two column phases of a group read different slots.  125 KB of LDS: one block per CU, which this small pass (2.7 GFLOP at 32 x 216 x
// 216) can afford.
constexpr int SB_T = 32, SB_POS = 10, SB_PITCH = 12, SB_GP = 68, SB_WT = 3 * ST_CO + 4;
constexpr int SB_G_FLOATS = SB_POS * SB_PITCH * SB_GP, SB_W_FLOATS = ST_K * ST_K * SB_WT;
constexpr size_t SB_LDS_BYTES = (size_t)(SB_G_FLOATS + SB_W_FLOATS) * sizeof(float);

__global__ __launch_bounds__(256) void lpips_stem_bwd_kernel(const float* __restrict__ g, const float* __restrict__ w_hwio,
                                                             float* __restrict__ dx, int h, int wd, int ho, int wo, int normalize) {
  extern __shared__ __attribute__((aligned(16))) float sb_lds[];
  float* gt = sb_lds;                                    // [10][12][68]
  float* wl = sb_lds + SB_G_FLOATS;                      // [121][196]
  const int tid = threadIdx.x, n = blockIdx.z;
  const int oy0 = blockIdx.y * (SB_T / 4) - 2, ox0 = blockIdx.x * (SB_T / 4) - 2;
  for (int e = tid; e < SB_POS * SB_POS * (ST_CO / 4); e += 256) {
    const int pos = e >> 4, q = e & 15;
    const int r = pos / SB_POS, c = pos - r * SB_POS;
    const int oy = oy0 + r, ox = ox0 + c;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (oy >= 0 && oy < ho && ox >= 0 && ox < wo) v = reinterpret_cast<const float4*>(g + (((size_t)n * ho + oy) * wo + ox) * ST_CO)[q];
    *reinterpret_cast<float4*>(gt + (r * SB_PITCH + c) * SB_GP + q * 4) = v;
  }
  for (int e = tid; e < ST_K * ST_K * 3 * (ST_CO / 4); e += 256) {
    const int tap = e / 48, q = e - tap * 48;
    *reinterpret_cast<float4*>(wl + tap * SB_WT + q * 4) = reinterpret_cast<const float4*>(w_hwio)[e];
  }
  __syncthreads();
  const int py = tid >> 6, px = (tid >> 4) & 3, ta = (tid >> 2) & 3, tb = tid & 3;
  float acc[4][3];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i][0] = acc[i][1] = acc[i][2] = 0.f;
  for (int jy = 2; jy >= 0; --jy) {                      // oy = 8 by + A - jy ascending
    const int ky = py + 4 * jy;
    if (ky >= ST_K) continue;
    for (int jx = 2; jx >= 0; --jx) {
      const int kx = px + 4 * jx;
      if (kx >= ST_K) continue;
      const float* wp = wl + (ky * ST_K + kx) * SB_WT;
      const float* g00 = gt + ((ta - jy + 2) * SB_PITCH + (tb - jx + 2)) * SB_GP;
      const float* g10 = g00 + 4 * SB_PITCH * SB_GP;
#pragma unroll 2
      for (int q = 0; q < ST_CO; q += 4) {
        float4 gv[4];
        gv[0] = *reinterpret_cast<const float4*>(g00 + q);
        gv[1] = *reinterpret_cast<const float4*>(g10 + q);
        gv[2] = *reinterpret_cast<const float4*>(g00 + 4 * SB_GP + q);
        gv[3] = *reinterpret_cast<const float4*>(g10 + 4 * SB_GP + q);
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) {
          const float4 wv = *reinterpret_cast<const float4*>(wp + ci * ST_CO + q);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            acc[i][ci] = fmaf(gv[i].x, wv.x, acc[i][ci]);
            acc[i][ci] = fmaf(gv[i].y, wv.y, acc[i][ci]);
            acc[i][ci] = fmaf(gv[i].z, wv.z, acc[i][ci]);
            acc[i][ci] = fmaf(gv[i].w, wv.w, acc[i][ci]);
          }
        }
      }
    }
  }
  const float scale[3] = {.458f, .448f, .450f};
  const float num = normalize ? 2.f : 1.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {                          // i: bit 0 = row A + 4, bit 1 = column B + 4
    const int y = blockIdx.y * SB_T + 4 * (ta + 4 * (i & 1)) + py - 2;
    const int x = blockIdx.x * SB_T + 4 * (tb + 4 * (i >> 1)) + px - 2;
    if (y < 0 || y >= h || x < 0 || x >= wd) continue;
    float* o = dx + (((size_t)n * h + y) * wd + x) * 3;
#pragma unroll
    for (int ci = 0; ci < 3; ++ci) o[ci] = acc[i][ci] * (num / scale[ci]);
  }
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

int srhip_lpips_head_bwd(const float* f, const int* pairs, const float* w, const float* upstream, float inv_count, float* df, int m,
                         int npairs, int h, int wd, int c, void* stream) {
  SRHIP_REQUIRE(f && pairs && w && upstream && df, "lpips_head_bwd: null tensor");
  SRHIP_REQUIRE(m > 0 && npairs > 0 && npairs <= 65535 && h > 0 && wd > 0 && c > 0 && c % 4 == 0,
                "lpips_head_bwd: needs C %% 4 == 0 and 1 <= pairs <= 65535");
  hipLaunchKernelGGL(lpips_head_bwd_kernel, dim3(LPIPS_BLOCKS, npairs), dim3(256), 0, as_stream(stream), f, pairs, w, upstream, inv_count,
                     df, (long)h * wd, c / 4);
  return check_launch("lpips_head_bwd");
}

int srhip_maxpool3x3s2_bwd(const float* x, const float* dy, const float* residual, float* dx, int n, int h, int w, int c, int relu,
                           void* stream) {
  SRHIP_REQUIRE(x && dy && dx, "maxpool3x3s2_bwd: null tensor");
  SRHIP_REQUIRE(n > 0 && c > 0 && c % 4 == 0 && h >= 3 && w >= 3, "maxpool3x3s2_bwd: needs C %% 4 == 0 and H, W >= 3");
  const int ho = (h - 3) / 2 + 1, wo = (w - 3) / 2 + 1;
  const long total = (long)n * h * w * (c / 4);
  SRHIP_REQUIRE(cdiv(total, 256) > 0, "maxpool3x3s2_bwd: tensor too large");
  hipLaunchKernelGGL(maxpool3x3s2_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, as_stream(stream), x, dy, residual, dx, h, w, c / 4, ho,
                     wo, relu, total);
  return check_launch("maxpool3x3s2_bwd");
}

int srhip_lpips_stem_bwd(const float* g, const float* w_hwio, float* dx, int m, int h, int w, int normalize, void* stream) {
  SRHIP_REQUIRE(g && w_hwio && dx, "lpips_stem_bwd: null tensor");
  SRHIP_REQUIRE(m > 0 && m <= 65535 && h >= 7 && w >= 7, "lpips_stem_bwd: needs 1 <= M <= 65535 and H, W >= 7");
  const int ho = (h + 2 * ST_P - ST_K) / ST_S + 1, wo = (w + 2 * ST_P - ST_K) / ST_S + 1;
  SRHIP_REQUIRE(cdiv(h + 2, SB_T) <= 65535, "lpips_stem_bwd: image too tall");
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(lpips_stem_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)SB_LDS_BYTES);
    attr_set = true;
  }
  hipLaunchKernelGGL(lpips_stem_bwd_kernel, dim3(cdiv(w + 2, SB_T), cdiv(h + 2, SB_T), m), dim3(256), SB_LDS_BYTES, as_stream(stream), g,
                     w_hwio, dx, h, w, ho, wo, normalize);
  return check_launch("lpips_stem_bwd");
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
