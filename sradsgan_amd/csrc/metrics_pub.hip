// Evaluation by the papers' protocol (EDSR, RCAN, ESRGAN, SwinIR, HAT, BasicSR: calculate_psnr / calculate_ssim; the reference ships the same
// two functions in GDP_x0/core/metrics.py:109-160) on the device.  The arithmetic is the contract stated in include/sradsgan_hip.h:
//   * float input is quantised like tensor2img(min_max=(0, 1)): (uint8) rintf(clamp(x, 0, 1) * 255.f), a NaN -> byte 0;
//   * `crop` rows and columns are shaved from every border;
//   * luma mode: num = 65481 r + 128553 g + 24966 b (exact int32), Y = 16 + num / 255000 in fp64, never rounded to fp32 or to a byte;
//   * MSE over the cropped pixels and channels as an EXACT integer sum (of byte differences, or of differences of `num` in luma mode,
//     kept as two uint64 halves because the luma sum passes 2^64 for a large scene);
//   * SSIM with the 11 x 11 Gaussian window g g^T (sigma 1.5) at every position whose window lies inside the cropped image,
//     population covariance, C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2, everything in fp64.
// A fixed number of partials per image (PUB_BLOCKS) is reduced in a fixed order and nothing is accumulated with atomics, so an image's
// three results carry the same bits alone or anywhere in a batch.
#include <math.h>

#include "common.h"

namespace srhip {

constexpr int PUB_BLOCKS = 512;   // partials per image: two 4096 x 4096 scene tiles' worth of blocks for each of the 256 CUs
constexpr int PUB_T = 16;         // SSIM tile side in valid positions
constexpr int PUB_HT = PUB_T + 10;
// Row pitch of the staged halo, in elements.  The horizontal pass reads 16 consecutive columns of two consecutive rows per 32-lane
// group: with 8-byte elements (64 banks of 4 B) the second row has to start 32 banks after the first -- pitch = 16 (mod 32) elements --
// and the same pitch puts the 4-byte RGBX pixels of the byte form 16 banks apart (32 banks for 4-byte reads).  48 is the first such
// pitch that holds the 26 columns.
constexpr int PUB_HP = 48;

struct PubWindow {
  double g[11];
};

// tensor2img(min_max=(0, 1)): diff_quant_kernel's rule with lo = 0, hi = 1, where (v - lo) / (hi - lo) is v itself.  fmaxf drops a NaN
// operand, so a NaN becomes byte 0 (a byte cannot carry one; include/sradsgan_hip.h says so).
__device__ __forceinline__ int pub_byte(float x) { return (int)rintf(fminf(fmaxf(x, 0.f), 1.f) * 255.f); }
__device__ __forceinline__ int pub_byte(unsigned char x) { return (int)x; }

__device__ __forceinline__ int pub_luma_num(int r, int g, int b) { return 65481 * r + 128553 * g + 24966 * b; }

// Sum of squared differences over the cropped region: a block walks rows, a thread the row's elements.  partial: uint64
// [n][PUB_BLOCKS][2] = {sum of the low 32 bits of d^2, sum of the high bits}: d^2 < 2^52 per pixel in luma mode, so each half stays far
// below 2^64 for any image whose pixel count fits 32 bits.
template <typename In, bool LUMA>
__global__ __launch_bounds__(256) void pub_sse_kernel(const In* __restrict__ a, const In* __restrict__ b,
                                                      unsigned long long* __restrict__ partial, int h, int w, int c, int crop) {
  __shared__ unsigned long long r0[256], r1[256];
  const int n = blockIdx.y, tid = threadIdx.x;
  const int hc = h - 2 * crop, wc = w - 2 * crop;
  unsigned long long lo = 0, hi = 0;
  for (int y = blockIdx.x; y < hc; y += gridDim.x) {
    const size_t row = (((size_t)n * h + y + crop) * w + crop) * c;
    if constexpr (LUMA) {
      for (int x = tid; x < wc; x += 256) {
        const size_t o = row + (size_t)x * 3;
        const int na = pub_luma_num(pub_byte(a[o]), pub_byte(a[o + 1]), pub_byte(a[o + 2]));
        const int nb = pub_luma_num(pub_byte(b[o]), pub_byte(b[o + 1]), pub_byte(b[o + 2]));
        const long long d = (long long)na - nb;
        const unsigned long long q = (unsigned long long)(d * d);
        lo += q & 0xffffffffull;
        hi += q >> 32;
      }
    } else {
      for (int x = tid; x < wc * c; x += 256) {
        const int d = pub_byte(a[row + x]) - pub_byte(b[row + x]);
        lo += (unsigned long long)(d * d);
      }
    }
  }
  r0[tid] = lo;
  r1[tid] = hi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      r0[tid] += r0[tid + o];
      r1[tid] += r1[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    partial[((size_t)n * gridDim.x + blockIdx.x) * 2 + 0] = r0[0];
    partial[((size_t)n * gridDim.x + blockIdx.x) * 2 + 1] = r1[0];
  }
}

// Staged halo element: RGBX bytes (RGB mode, every channel staged once) or the fp64 luma.
template <bool LUMA>
struct PubStage {
  typedef unsigned int type;     // four bytes, channel ch in bits [8 ch, 8 ch + 8)
};
template <>
struct PubStage<true> {
  typedef double type;
};

// Gaussian SSIM.  A block walks 16 x 16 tiles of valid positions in a grid-stride loop.  The 26 x 26 halo of both images is staged once
// in LDS, quantised (and in luma mode converted) while staging; the window is applied separably: 11 horizontal taps of the five moments
// a, b, a^2, b^2, ab into LDS rows [5][26][16], then 11 vertical taps in registers, then the formula.  partial: double [n][PUB_BLOCKS].
template <typename In, bool LUMA>
__global__ __launch_bounds__(256) void pub_ssim_kernel(const In* __restrict__ a, const In* __restrict__ b, double* __restrict__ partial,
                                                       int h, int w, int c, int crop, PubWindow win) {
  constexpr int T = PUB_T, HT = PUB_HT, HP = PUB_HP;
  typedef typename PubStage<LUMA>::type stage_t;
  __shared__ stage_t sa[HT * HP], sb[HT * HP];
  __shared__ double hm[5][HT][T];
  __shared__ double red[256];
  const int n = blockIdx.y, tid = threadIdx.x;
  const int hc = h - 2 * crop, wc = w - 2 * crop;       // cropped image
  const int vh = hc - 10, vw = wc - 10;                 // valid positions
  const int tiles_x = (vw + T - 1) / T, tiles_y = (vh + T - 1) / T;
  const long tiles = (long)tiles_x * tiles_y;
  const double c1 = (0.01 * 255.0) * (0.01 * 255.0), c2 = (0.03 * 255.0) * (0.03 * 255.0);
  const int ly = tid >> 4, lx = tid & 15;
  const int nch = LUMA ? 1 : c;
  double acc = 0.0;
  for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int ty0 = (int)(t / tiles_x) * T, tx0 = (int)(t % tiles_x) * T;
    // no barrier here: the previous tile's staging was last read before the barrier that precedes its vertical pass, and hm is not
    // written before the barrier after this staging
    // A thread stages up to NS halo pixels.  All their loads are issued before the first conversion, so that the tile waits for one
    // memory round trip instead of NS: a block has one tile in flight and the loop below, written per pixel, waited NS times.
    constexpr int NS = (HT * HT + 255) / 256;
    In ra[NS][3], rb[NS][3];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int e = tid + s * 256;
      const int py = e / HT, px = e - py * HT;
      const int gy = ty0 + py, gx = tx0 + px;            // in the cropped image
      const bool inside = e < HT * HT && gy < hc && gx < wc;
      // a pixel outside the image reads the image's first cropped pixel instead (its value is dropped below), and a channel the image
      // does not have reads channel 0: every load is unconditional and in bounds, so none of them sits behind a branch of its own
      const size_t o = (((size_t)n * h + (inside ? gy : 0) + crop) * w + (inside ? gx : 0) + crop) * c;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int kk = (LUMA || k < c) ? k : 0;
        ra[s][k] = a[o + kk];
        rb[s][k] = b[o + kk];
      }
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int e = tid + s * 256;
      const int py = e / HT, px = e - py * HT;
      const bool inside = e < HT * HT && ty0 + py < hc && tx0 + px < wc;
      stage_t va = 0, vb = 0;
      if (inside) {
        if constexpr (LUMA) {
          va = (stage_t)(16.0 + (double)pub_luma_num(pub_byte(ra[s][0]), pub_byte(ra[s][1]), pub_byte(ra[s][2])) / 255000.0);
          vb = (stage_t)(16.0 + (double)pub_luma_num(pub_byte(rb[s][0]), pub_byte(rb[s][1]), pub_byte(rb[s][2])) / 255000.0);
        } else {
          unsigned int ua = 0, ub = 0;
#pragma unroll
          for (int k = 0; k < 3; ++k)
            if (k < c) {
              ua |= (unsigned int)pub_byte(ra[s][k]) << (8 * k);
              ub |= (unsigned int)pub_byte(rb[s][k]) << (8 * k);
            }
          va = (stage_t)ua;
          vb = (stage_t)ub;
        }
      }
      if (e < HT * HT) {
        sa[py * HP + px] = va;
        sb[py * HP + px] = vb;
      }
    }
    __syncthreads();
    for (int ch = 0; ch < nch; ++ch) {
      for (int e = tid; e < HT * T; e += 256) {          // horizontal taps: 26 rows x 16 columns
        const int py = e >> 4, px = e & 15;
        double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
#pragma unroll
        for (int k = 0; k < 11; ++k) {
          double va, vb;
          if constexpr (LUMA) {
            va = (double)sa[py * HP + px + k];
            vb = (double)sb[py * HP + px + k];
          } else {
            va = (double)(((unsigned int)sa[py * HP + px + k] >> (8 * ch)) & 255u);
            vb = (double)(((unsigned int)sb[py * HP + px + k] >> (8 * ch)) & 255u);
          }
          const double gk = win.g[k];
          m0 += gk * va;
          m1 += gk * vb;
          m2 += gk * (va * va);
          m3 += gk * (vb * vb);
          m4 += gk * (va * vb);
        }
        hm[0][py][px] = m0;
        hm[1][py][px] = m1;
        hm[2][py][px] = m2;
        hm[3][py][px] = m3;
        hm[4][py][px] = m4;
      }
      __syncthreads();
      if (ty0 + ly < vh && tx0 + lx < vw) {              // vertical taps in registers, then the formula
        double ua = 0.0, ub = 0.0, eaa = 0.0, ebb = 0.0, eab = 0.0;
#pragma unroll
        for (int k = 0; k < 11; ++k) {
          const double gk = win.g[k];
          ua += gk * hm[0][ly + k][lx];
          ub += gk * hm[1][ly + k][lx];
          eaa += gk * hm[2][ly + k][lx];
          ebb += gk * hm[3][ly + k][lx];
          eab += gk * hm[4][ly + k][lx];
        }
        const double ua2 = ua * ua, ub2 = ub * ub, uab = ua * ub;
        const double vaa = eaa - ua2, vbb = ebb - ub2, vab = eab - uab;
        acc += ((2.0 * uab + c1) * (2.0 * vab + c2)) / ((ua2 + ub2 + c1) * (vaa + vbb + c2));
      }
      if (ch + 1 < nch) __syncthreads();                 // hm is rewritten for the next channel
    }
  }
  red[tid] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) partial[(size_t)n * gridDim.x + blockIdx.x] = red[0];
}

// One wave per image: lane l sums partials l, l + 64, ... in that order, lane 0 then the 64 lane sums in lane order.
// sse_den: what the integer sum is divided by before the pixel count (1 in RGB mode, 255000^2 in luma mode).
__global__ __launch_bounds__(64) void pub_finish_kernel(const unsigned long long* __restrict__ sse, const double* __restrict__ ssim,
                                                        double* __restrict__ out, int n, double sse_den, double count, double ssim_count) {
  __shared__ unsigned long long l0[64], l1[64];
  __shared__ double ls[64];
  const int b = blockIdx.x, lane = threadIdx.x;
  unsigned long long s0 = 0, s1 = 0;
  double ss = 0.0;
  for (int j = lane; j < PUB_BLOCKS; j += 64) {
    s0 += sse[((size_t)b * PUB_BLOCKS + j) * 2];
    s1 += sse[((size_t)b * PUB_BLOCKS + j) * 2 + 1];
    ss += ssim[(size_t)b * PUB_BLOCKS + j];
  }
  l0[lane] = s0;
  l1[lane] = s1;
  ls[lane] = ss;
  __syncthreads();
  if (lane != 0) return;
  s0 = 0, s1 = 0, ss = 0.0;
  for (int j = 0; j < 64; ++j) {
    s0 += l0[j];
    s1 += l1[j];
    ss += ls[j];
  }
  // RGB mode: s1 = 0 and s0 < 2^53 for every image this ABI takes, so mse is the exact integer divided once
  const double total = s1 ? (double)s1 * 4294967296.0 + (double)s0 : (double)s0;
  const double mse = sse_den == 1.0 ? total / count : total / sse_den / count;
  out[b] = mse;
  out[n + b] = mse > 0.0 ? 10.0 * log10(255.0 * 255.0 / mse) : __builtin_inf();
  out[2 * n + b] = ss / ssim_count;
}

static PubWindow pub_window() {
  PubWindow win;
  double sum = 0.0;
  for (int i = 0; i < 11; ++i) {
    win.g[i] = exp(-(double)((i - 5) * (i - 5)) / 4.5);
    sum += win.g[i];
  }
  for (int i = 0; i < 11; ++i) win.g[i] /= sum;
  return win;
}

static int pub_check(const char* what, const void* a, const void* b, const void* out, int n, int h, int w, int c, int crop, int luma,
                     int is_float) {
  SRHIP_REQUIRE(a && b && out, "%s: null tensor", what);
  SRHIP_REQUIRE(n > 0 && h > 0 && w > 0 && (c == 1 || c == 3), "%s: needs n, h, w > 0 and c in {1, 3} (got n %d, h %d, w %d, c %d)", what, n,
                h, w, c);
  SRHIP_REQUIRE(!luma || c == 3, "%s: the luma channel needs c = 3, got %d", what, c);
  SRHIP_REQUIRE(crop >= 0 && (long)h - 2L * crop >= 11 && (long)w - 2L * crop >= 11,
                "%s: the cropped image must be at least 11 x 11 (h %d, w %d, crop_border %d)", what, h, w, crop);
  SRHIP_REQUIRE((is_float == 0 || is_float == 1) && (luma == 0 || luma == 1), "%s: is_float and luma are 0 or 1", what);
  return SRHIP_OK;
}

}  // namespace srhip

using namespace srhip;

extern "C" {

int srhip_pub_config(int* partials, int* tile) {
  SRHIP_REQUIRE(partials && tile, "pub_config: null pointer");
  *partials = PUB_BLOCKS;
  *tile = PUB_T;
  return SRHIP_OK;
}

int srhip_pub_sse(const void* a, const void* b, unsigned long long* partial, int n, int h, int w, int c, int crop, int luma, int is_float,
                  void* stream) {
  if (int rc = pub_check("pub_sse", a, b, partial, n, h, w, c, crop, luma, is_float)) return rc;
  const dim3 grid(PUB_BLOCKS, n), block(256);
  hipStream_t st = as_stream(stream);
  const float *fa = (const float*)a, *fb = (const float*)b;
  const unsigned char *ua = (const unsigned char*)a, *ub = (const unsigned char*)b;
  if (is_float && luma) hipLaunchKernelGGL((pub_sse_kernel<float, true>), grid, block, 0, st, fa, fb, partial, h, w, c, crop);
  else if (is_float) hipLaunchKernelGGL((pub_sse_kernel<float, false>), grid, block, 0, st, fa, fb, partial, h, w, c, crop);
  else if (luma) hipLaunchKernelGGL((pub_sse_kernel<unsigned char, true>), grid, block, 0, st, ua, ub, partial, h, w, c, crop);
  else hipLaunchKernelGGL((pub_sse_kernel<unsigned char, false>), grid, block, 0, st, ua, ub, partial, h, w, c, crop);
  return check_launch("pub_sse");
}

int srhip_pub_ssim(const void* a, const void* b, double* partial, int n, int h, int w, int c, int crop, int luma, int is_float,
                   void* stream) {
  if (int rc = pub_check("pub_ssim", a, b, partial, n, h, w, c, crop, luma, is_float)) return rc;
  const dim3 grid(PUB_BLOCKS, n), block(256);
  hipStream_t st = as_stream(stream);
  const PubWindow win = pub_window();
  const float *fa = (const float*)a, *fb = (const float*)b;
  const unsigned char *ua = (const unsigned char*)a, *ub = (const unsigned char*)b;
  if (is_float && luma) hipLaunchKernelGGL((pub_ssim_kernel<float, true>), grid, block, 0, st, fa, fb, partial, h, w, c, crop, win);
  else if (is_float) hipLaunchKernelGGL((pub_ssim_kernel<float, false>), grid, block, 0, st, fa, fb, partial, h, w, c, crop, win);
  else if (luma) hipLaunchKernelGGL((pub_ssim_kernel<unsigned char, true>), grid, block, 0, st, ua, ub, partial, h, w, c, crop, win);
  else hipLaunchKernelGGL((pub_ssim_kernel<unsigned char, false>), grid, block, 0, st, ua, ub, partial, h, w, c, crop, win);
  return check_launch("pub_ssim");
}

int srhip_pub_finish(const unsigned long long* sse_partial, const double* ssim_partial, double* out, int n, int h, int w, int c, int crop,
                     int luma, void* stream) {
  if (int rc = pub_check("pub_finish", sse_partial, ssim_partial, out, n, h, w, c, crop, luma, 0)) return rc;
  const double hc = (double)(h - 2 * crop), wc = (double)(w - 2 * crop), nch = luma ? 1.0 : (double)c;
  hipLaunchKernelGGL(pub_finish_kernel, dim3(n), dim3(64), 0, as_stream(stream), sse_partial, ssim_partial, out, n,
                     luma ? 255000.0 * 255000.0 : 1.0, hc * wc * nch, (hc - 10.0) * (wc - 10.0) * nch);
  return check_launch("pub_finish");
}

}  // extern "C"
