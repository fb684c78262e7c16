// The blur-and-noise degradation of training batches (model/util.py:383-405 BatchBlur, :342-348 b_GaussianNoising; degrade.py):
//   blur_kernel<C, U8>    depth-wise l x l cross-correlation of every sample with ITS OWN kernel on a reflection-padded image,
//                         l = 1..21: uint8 [N][H][W][C] -> uint8 (x / 255 in, trunc(acc * 255) out: to_pil_image's mul(255).byte())
//                         or a strided float [N][C][H][W] -> float without quantisation
//   degrade_noise_kernel  uint8 [N][H][W][C] -> float: clamp(byte / 255 + z * level[n], 0, 1), z supplied or drawn (Philox)
// The sum of one output is ONE fp32 chain in a fixed order, rows outer and columns inner, product and sum rounded separately
// (the build has -ffp-contract=off): acc = 0; acc = acc + k[i][j] * xpad[y + i][x + j].  No split accumulators, no fma: the
// bytes equal a float32 restatement in numpy and do not depend on the batch size, the tile or the launch shape.  The price is a
// dependent add per tap; the eight chains a thread owns are independent of each other and interleave.
//
// One block computes TY x TX pixels of one sample, all C channels.  The halo tile is staged ONCE as floats in LDS, one plane per
// channel, reflection resolved while staging, so the tap loop has no index arithmetic.  A thread owns STRIP adjacent pixels of one
// row and channel: per kernel row it walks a register window over l + STRIP - 1 staged values, every value feeding up to STRIP
// accumulators.  Lanes run over (strip, row) with the strip fastest: a wave half reads plane[row * RS + strip * STRIP + m] with
// 4 strips x 8 rows, conflict-free on the 32 banks for any ODD row stride RS (cdna_hip_programming guideline 4: break the
// power-of-two stride).  The l x l weights are the same for every lane of a block and are read through uniform addresses.
// uint8 results go through a small LDS tile so that global stores are whole dwords with scalar heads and tails per row.
#include "common.h"
#include "philox.h"

namespace srhip {

constexpr int BLUR_MAX_L = 21;
constexpr int BLUR_TX = 32, BLUR_TY = 32, BLUR_STRIP = 8;
constexpr int BLUR_STRIPS = BLUR_TX / BLUR_STRIP;             // strips per tile row
constexpr int BLUR_THREADS_PER_CH = BLUR_TY * BLUR_STRIPS;    // 128: two waves per channel

struct BlurStrides {
  long n, c, h, w;
};

struct BlurArgs {
  const void* in;            // uint8 [n][h][w][c] or float by strides
  void* out;
  const float* kernels;      // [n][l][l] or [l][l]
  BlurStrides xs, ys;        // float form only
  int n, h, w, l, per_sample;
  int rows, cols, rs;        // staged tile: rows x cols values per channel plane, row stride rs (odd)
};

__device__ __forceinline__ int reflect_clamped(int g, int size) {
  g = g < 0 ? -g : g;
  g = g >= size ? 2 * (size - 1) - g : g;
  return g < 0 ? 0 : (g >= size ? size - 1 : g);   // only positions no stored output reads get here
}

template <int C, bool U8>
__global__ void __launch_bounds__(BLUR_THREADS_PER_CH* C) blur_kernel(BlurArgs a) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x;
  const int nthreads = BLUR_THREADS_PER_CH * C;
  const int n = blockIdx.z, y0 = blockIdx.y * BLUR_TY, x0 = blockIdx.x * BLUR_TX;
  const int l = a.l, lo = l / 2;
  const int plane = a.rows * a.rs;

  // ---- stage: plane[ch][t][m] = x[reflect(y0 - lo + t)][reflect(x0 - lo + m)][ch] for m < TX + l - 1, zero in the window's slack
  {
    const int wave = tid >> 6, lane = tid & 63, nwaves = nthreads >> 6;
    const int need = BLUR_TX + l - 1;
    for (int t = wave; t < a.rows; t += nwaves) {
      const int gy = reflect_clamped(y0 - lo + t, a.h);
      for (int e = lane; e < a.cols * C; e += 64) {
        const int m = e / C, ch = e - m * C;
        float v = 0.0f;
        if (m < need) {
          const int gx = reflect_clamped(x0 - lo + m, a.w);
          if (U8)
            v = (float)static_cast<const unsigned char*>(a.in)[(((long)n * a.h + gy) * a.w + gx) * C + ch] / 255.0f;
          else
            v = static_cast<const float*>(a.in)[n * a.xs.n + ch * a.xs.c + gy * a.xs.h + gx * a.xs.w];
        }
        lds[ch * plane + t * a.rs + m] = v;
      }
    }
  }
  __syncthreads();

  const int sx = tid % BLUR_STRIPS, ty = (tid / BLUR_STRIPS) % BLUR_TY, ch = tid / BLUR_THREADS_PER_CH;
  const float* kern = a.kernels + (a.per_sample ? (long)n * l * l : 0);
  const float* row = lds + ch * plane + ty * a.rs + sx * BLUR_STRIP;
  float acc[BLUR_STRIP];
#pragma unroll
  for (int r = 0; r < BLUR_STRIP; ++r) acc[r] = 0.0f;
  for (int i = 0; i < l; ++i) {
    const float* k = kern + i * l;
    float win[2 * BLUR_STRIP];
#pragma unroll
    for (int m = 0; m < BLUR_STRIP; ++m) win[m] = row[m];
    for (int j0 = 0; j0 < l; j0 += BLUR_STRIP) {
#pragma unroll
      for (int m = 0; m < BLUR_STRIP; ++m) win[BLUR_STRIP + m] = row[j0 + BLUR_STRIP + m];
#pragma unroll
      for (int jj = 0; jj < BLUR_STRIP; ++jj) {
        if (j0 + jj < l) {                              // the same in every lane
          const float kv = k[j0 + jj];
#pragma unroll
          for (int r = 0; r < BLUR_STRIP; ++r) acc[r] = acc[r] + kv * win[jj + r];
        }
      }
#pragma unroll
      for (int m = 0; m < BLUR_STRIP; ++m) win[m] = win[BLUR_STRIP + m];
    }
    row += a.rs;
  }

  const int y = y0 + ty, xb = x0 + sx * BLUR_STRIP;
  if (!U8) {
    if (y < a.h) {
      float* o = static_cast<float*>(a.out) + n * a.ys.n + ch * a.ys.c + y * a.ys.h;
#pragma unroll
      for (int r = 0; r < BLUR_STRIP; ++r)
        if (xb + r < a.w) o[(xb + r) * a.ys.w] = acc[r];
    }
    return;
  }

  // ---- uint8: quantise into an interleaved LDS tile, then whole dwords per output row with scalar heads and tails
  __syncthreads();                                       // every wave is done reading the planes
  unsigned char* tile = reinterpret_cast<unsigned char*>(lds);
#pragma unroll
  for (int r = 0; r < BLUR_STRIP; ++r)
    tile[(ty * BLUR_TX + sx * BLUR_STRIP + r) * C + ch] = (unsigned char)(int)(acc[r] * 255.0f);
  __syncthreads();
  const int tw = min(BLUR_TX, a.w - x0), th = min(BLUR_TY, a.h - y0);
  const int nbytes = tw * C;                             // bytes of one tile row
  constexpr int SLOTS = BLUR_TX * 4 / 4 + 1;             // dwords a row of at most TX * 4 bytes can touch
  unsigned char* outp = static_cast<unsigned char*>(a.out);
  for (int s = tid; s < th * SLOTS; s += nthreads) {
    const int r = s / SLOTS, q = s - r * SLOTS;
    unsigned char* g = outp + (((long)n * a.h + y0 + r) * a.w + x0) * C;   // first byte of this tile row
    const int mis = (int)((size_t)g & 3);
    const int bb = max(4 * q - mis, 0), be = min(4 * q - mis + 4, nbytes);  // this slot's dword, cut to the row
    if (bb >= be) continue;
    const unsigned char* t = tile + r * BLUR_TX * C;
    if (be - bb == 4) {
      const unsigned word = t[bb] | (t[bb + 1] << 8) | (t[bb + 2] << 16) | ((unsigned)t[bb + 3] << 24);
      *reinterpret_cast<unsigned*>(g + bb) = word;       // (g + bb) & 3 == 0 by the choice of bb
    } else {
      for (int b = bb; b < be; ++b) g[b] = t[b];
    }
  }
}

// One thread per Philox group of 4 consecutive elements of the flat [n][h][w][c] index (the convention of srhip_augment_u8).
__global__ void degrade_noise_kernel(const unsigned char* __restrict__ lr, const float* __restrict__ level, const float* __restrict__ z,
                                     float* __restrict__ out, long total, long per_sample, int drawn, unsigned long long seed,
                                     unsigned long long step) {
  const long grp = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (grp * 4 >= total) return;
  float z4[4] = {0.f, 0.f, 0.f, 0.f};
  if (drawn) philox_normal4(seed, step, (unsigned long long)grp, z4);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long e = grp * 4 + k;
    if (e >= total) break;
    const float x = (float)lr[e] / 255.0f;               // srhip_u8_to_float's expression
    const float zv = z ? z[e] : z4[k];
    const float q = x + zv * level[e / per_sample];
    out[e] = q < 0.0f ? 0.0f : (q > 1.0f ? 1.0f : q);    // torch.clamp: a NaN fails both comparisons and stays
  }
}

static int blur_geometry(BlurArgs& a, int c, size_t& lds_bytes) {
  const int chunks = (a.l + BLUR_STRIP - 1) / BLUR_STRIP;
  a.rows = BLUR_TY + a.l - 1;
  a.cols = BLUR_TX + chunks * BLUR_STRIP;                // the register window reads whole strips
  a.rs = a.cols | 1;
  lds_bytes = (size_t)c * a.rows * a.rs * sizeof(float);
  const size_t tile_bytes = (size_t)BLUR_TY * BLUR_TX * c;
  if (lds_bytes < tile_bytes) lds_bytes = tile_bytes;
  return lds_bytes <= 64 * 1024;
}

template <bool U8>
static void blur_launch(const BlurArgs& a, int c, size_t lds_bytes, hipStream_t st) {
  const dim3 grid((unsigned)cdiv(a.w, BLUR_TX), (unsigned)cdiv(a.h, BLUR_TY), (unsigned)a.n);
  switch (c) {
    case 1: hipLaunchKernelGGL((blur_kernel<1, U8>), grid, dim3(BLUR_THREADS_PER_CH * 1), lds_bytes, st, a); break;
    case 2: hipLaunchKernelGGL((blur_kernel<2, U8>), grid, dim3(BLUR_THREADS_PER_CH * 2), lds_bytes, st, a); break;
    case 3: hipLaunchKernelGGL((blur_kernel<3, U8>), grid, dim3(BLUR_THREADS_PER_CH * 3), lds_bytes, st, a); break;
    default: hipLaunchKernelGGL((blur_kernel<4, U8>), grid, dim3(BLUR_THREADS_PER_CH * 4), lds_bytes, st, a); break;
  }
}

}  // namespace srhip

using namespace srhip;

extern "C" {

int srhip_blur_u8(const unsigned char* in, const float* kernels_dev, unsigned char* out, int n, int h, int w, int c, int l, void* stream) {
  SRHIP_REQUIRE(in && kernels_dev && out, "blur_u8: null tensor");
  SRHIP_REQUIRE(in != out, "blur_u8: not in place");
  SRHIP_REQUIRE(n > 0 && h > 0 && w > 0 && c > 0 && c <= 4, "blur_u8: bad size (n %d, %dx%dx%d)", n, h, w, c);
  SRHIP_REQUIRE(l >= 1 && l <= BLUR_MAX_L, "blur_u8: kernel size %d outside 1..%d", l, BLUR_MAX_L);
  SRHIP_REQUIRE(l / 2 < h && l / 2 < w, "blur_u8: reflection padding %d needs an image larger than it, got %dx%d", l / 2, h, w);
  SRHIP_REQUIRE(n <= 65535 && cdiv(h, BLUR_TY) <= 65535, "blur_u8: batch too large for one launch");
  SRHIP_REQUIRE(((size_t)kernels_dev & 3) == 0, "blur_u8: the kernels must be 4-byte aligned");
  BlurArgs a{};
  a.in = in, a.out = out, a.kernels = kernels_dev;
  a.n = n, a.h = h, a.w = w, a.l = l, a.per_sample = 1;
  size_t lds_bytes;
  SRHIP_REQUIRE(blur_geometry(a, c, lds_bytes), "blur_u8: tile does not fit the LDS");
  blur_launch<true>(a, c, lds_bytes, as_stream(stream));
  return check_launch("blur_u8");
}

int srhip_blur_f32(const float* x, const long* x_strides, const float* kernels_dev, int per_sample, float* y, const long* y_strides, int n,
                   int c, int h, int w, int l, void* stream) {
  SRHIP_REQUIRE(x && y && kernels_dev && x_strides && y_strides, "blur_f32: null tensor");
  SRHIP_REQUIRE(x != y, "blur_f32: not in place");
  SRHIP_REQUIRE(n > 0 && h > 0 && w > 0 && c > 0, "blur_f32: bad size (n %d, %dx%dx%d)", n, c, h, w);
  SRHIP_REQUIRE(l >= 1 && l <= BLUR_MAX_L, "blur_f32: kernel size %d outside 1..%d", l, BLUR_MAX_L);
  SRHIP_REQUIRE(l / 2 < h && l / 2 < w, "blur_f32: reflection padding %d needs an image larger than it, got %dx%d", l / 2, h, w);
  for (int k = 0; k < 4; ++k) SRHIP_REQUIRE(x_strides[k] >= 0 && y_strides[k] >= 0, "blur_f32: negative stride");
  SRHIP_REQUIRE(((size_t)x & 3) == 0 && ((size_t)y & 3) == 0 && ((size_t)kernels_dev & 3) == 0, "blur_f32: tensors must be 4-byte aligned");
  SRHIP_REQUIRE(cdiv(h, BLUR_TY) <= 65535, "blur_f32: image too tall for one launch");
  // channels go through the kernel four at a time (one LDS plane each); a launch covers at most 65535 samples
  for (int c0 = 0; c0 < c; c0 += 4) {
    const int cc = c - c0 < 4 ? c - c0 : 4;
    for (int n0 = 0; n0 < n; n0 += 65535) {
      BlurArgs a{};
      a.xs = BlurStrides{x_strides[0], x_strides[1], x_strides[2], x_strides[3]};
      a.ys = BlurStrides{y_strides[0], y_strides[1], y_strides[2], y_strides[3]};
      a.in = x + n0 * a.xs.n + c0 * a.xs.c, a.out = y + n0 * a.ys.n + c0 * a.ys.c;
      a.kernels = kernels_dev + (per_sample ? (long)n0 * l * l : 0);
      a.n = n - n0 < 65535 ? n - n0 : 65535, a.h = h, a.w = w, a.l = l, a.per_sample = per_sample != 0;
      size_t lds_bytes;
      SRHIP_REQUIRE(blur_geometry(a, cc, lds_bytes), "blur_f32: tile does not fit the LDS");
      blur_launch<false>(a, cc, lds_bytes, as_stream(stream));
      const int rc = check_launch("blur_f32");
      if (rc != SRHIP_OK) return rc;
    }
  }
  return SRHIP_OK;
}

int srhip_degrade_noise_u8(const unsigned char* lr, const float* level_dev, const float* z, float* out, int n, int h, int w, int c,
                           int drawn, unsigned long long seed, unsigned long long step, void* stream) {
  SRHIP_REQUIRE(lr && level_dev && out, "degrade_noise_u8: null tensor");
  SRHIP_REQUIRE(n > 0 && h > 0 && w > 0 && c > 0 && c <= 4, "degrade_noise_u8: bad size (n %d, %dx%dx%d)", n, h, w, c);
  SRHIP_REQUIRE(!(z && drawn), "degrade_noise_u8: noise is either supplied (z) or drawn, not both");
  SRHIP_REQUIRE(z || drawn, "degrade_noise_u8: needs z or drawn != 0");
  SRHIP_REQUIRE(((size_t)z & 3) == 0 && ((size_t)out & 3) == 0 && ((size_t)level_dev & 3) == 0, "degrade_noise_u8: float tensors must be 4-byte aligned");
  const long per_sample = (long)h * w * c, total = per_sample * n;
  SRHIP_REQUIRE(total < (1L << 38), "degrade_noise_u8: batch too large for one launch");
  hipLaunchKernelGGL(degrade_noise_kernel, dim3((unsigned)cdiv((total + 3) / 4, 256)), dim3(256), 0, as_stream(stream), lr, level_dev, z, out,
                     total, per_sample, drawn != 0, seed, step);
  return check_launch("degrade_noise_u8");
}

}  // extern "C"
