// The contrastive VGG19 losses of the reference (model/loss.py:121-298: Vgg19, ContrastLoss, NContrastLoss, ContrastCosineLoss,
// NContrastCosineLoss) around the ordinary conv kernels (contrast.py):
//   * the floor-mode 2 x 2 max pool for odd H or W, forward and backward (the backward fused with a ReLU mask and a residual add),
//   * per tap, the L1 distances of the anchor to the positive and to every negative in one pass (float64 partial sums), and their
//     gradient to the anchor through the tap's ReLU,
//   * per tap, the per-pixel cosine similarities of the anchor to the positive and every negative (float64 partial sums per sample),
//     and their gradient to the anchor through the tap's ReLU,
//   * one finish launch per loss kind: the partials of all taps -> the scalar loss and the coefficients of the backward, in float64,
//     left on the device.
// A tap holds the features of the stacked batch [a; p; n_1 .. n_N]: m = (2 + N) b images, operand k of sample s at image (k + 1) b + s.
// Exact fp32 elementwise work, fp64 reductions in one fixed order per value, no atomics, plain vector loads and stores.
#include "common.h"

namespace srhip {

constexpr int CT_MAX_OPS = 9;                 // the positive and up to 8 negatives
constexpr int CT_TAPS = 5;
constexpr int CT_L1_PARTS = 1024;             // blocks of the L1 forward = partial sums per operand
constexpr int CT_COS_PARTS = 64;              // blocks per sample of the cosine forward = partial sums per (sample, operand)

struct CtCounts {
  double v[CT_TAPS];
};

__device__ inline float ct_group16_sum(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ inline double ct_group16_sum(double v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ inline double ct_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float ct_sign(float d) { return (float)((d > 0.f) - (d < 0.f)); }

// ---- floor-mode 2 x 2 max pool --------------------------------------------------------------------------------------------------------
// ho = h / 2, wo = w / 2: an odd last row or column belongs to no window.  pool_takes is the project's window scan: the first maximum
// wins, as in ATen.
__global__ __launch_bounds__(256) void maxpool2x2_floor_kernel(const float* __restrict__ x, float* __restrict__ y, int h, int w, int c4,
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
  for (int k = 1; k < 4; ++k) {
    const float4 v = src[((long)(k >> 1) * w + (k & 1)) * c4];
    if (pool_takes(v.x, m.x)) m.x = v.x;
    if (pool_takes(v.y, m.y)) m.y = v.y;
    if (pool_takes(v.z, m.z)) m.z = v.z;
    if (pool_takes(v.w, m.w)) m.w = v.w;
  }
  reinterpret_cast<float4*>(y)[i] = m;
}

// Gather form: a thread owns one input pixel and 4 channels.  The pixel lies in at most one window; it recomputes that window's arg-max
// with the forward's scan and takes dy when the arg-max is its own position.  dx = gather(dy) [* (x > 0)] [+ residual]: x is the pool's
// input; relu != 0 applies the mask of x (x <= 0 writes 0, a NaN passes the gradient on, like ATen's threshold_backward).
__global__ __launch_bounds__(256) void maxpool2x2_floor_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                   const float* __restrict__ residual, float* __restrict__ dx, int h,
                                                                   int w, int c4, int ho, int wo, int relu, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int cv = (int)(i % c4);
  long p = i / c4;
  const int ix = (int)(p % w);
  p /= w;
  const int iy = (int)(p % h);
  const long n = p / h;
  const float4* xs = reinterpret_cast<const float4*>(x);
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  const int oy = iy >> 1, ox = ix >> 1;
  if (oy < ho && ox < wo) {
    const float4* src = xs + ((n * h + 2 * oy) * w + 2 * ox) * c4 + cv;
    const int mine = (iy & 1) * 2 + (ix & 1);
    float4 m = src[0];
    int ax = 0, ay = 0, az = 0, aw = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      const float4 v = src[((long)(k >> 1) * w + (k & 1)) * c4];
      if (pool_takes(v.x, m.x)) { m.x = v.x; ax = k; }
      if (pool_takes(v.y, m.y)) { m.y = v.y; ay = k; }
      if (pool_takes(v.z, m.z)) { m.z = v.z; az = k; }
      if (pool_takes(v.w, m.w)) { m.w = v.w; aw = k; }
    }
    const float4 g = reinterpret_cast<const float4*>(dy)[((n * ho + oy) * wo + ox) * c4 + cv];
    if (ax == mine) o.x = g.x;
    if (ay == mine) o.y = g.y;
    if (az == mine) o.z = g.z;
    if (aw == mine) o.w = g.w;
  }
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

// ---- L1 distances ---------------------------------------------------------------------------------------------------------------------
// Forward: CT_L1_PARTS blocks walk the anchor's float4s with a grid stride; a thread reads the anchor value once and each operand's
// value beside it, forms |a - x_k| in fp32 (one rounding) and adds it to its float64 sum of operand k.  Block sum: lanes by xor
// butterfly, then the four waves in ascending order.  partial [kops][CT_L1_PARTS]; every block writes, so nothing is zeroed first.
template <int KOPS>
__global__ __launch_bounds__(256) void contrast_l1_fwd_kernel(const float* __restrict__ f, double* __restrict__ partial, long per4) {
  __shared__ double red[CT_MAX_OPS][4];
  const float4* a = reinterpret_cast<const float4*>(f);
  double acc[KOPS];
#pragma unroll
  for (int k = 0; k < KOPS; ++k) acc[k] = 0.0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per4; i += (long)CT_L1_PARTS * 256) {
    const float4 u = a[i];
#pragma unroll
    for (int k = 0; k < KOPS; ++k) {
      const float4 v = a[(long)(k + 1) * per4 + i];
      acc[k] += (double)fabsf(u.x - v.x) + (double)fabsf(u.y - v.y) + (double)fabsf(u.z - v.z) + (double)fabsf(u.w - v.w);
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < KOPS; ++k) {
    const double s = ct_wave_sum(acc[k]);
    if (lane == 0) red[k][wave] = s;
  }
  __syncthreads();
  if (threadIdx.x < KOPS)
    partial[(size_t)threadIdx.x * CT_L1_PARTS + blockIdx.x] =
        ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
}

// Backward: da = up * (alpha * sign(a - p) - sum_j beta_j * sign(a - n_j)), sign(0) = 0, through the tap's ReLU (a <= 0 writes 0).
// coef = double [kops] on the device (alpha, beta_1 ..), up = a float32 device scalar.  The signs are exact, the sum runs in float64
// in ascending j and is rounded to fp32 once.
template <int KOPS>
__global__ __launch_bounds__(256) void contrast_l1_bwd_kernel(const float* __restrict__ f, const double* __restrict__ coef,
                                                              const float* __restrict__ upstream, float* __restrict__ da, long per4) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= per4) return;
  const float4* a = reinterpret_cast<const float4*>(f);
  const double up = (double)upstream[0];
  const float4 u = a[i];
  double sx, sy, sz, sw;
  {
    const float4 v = a[per4 + i];
    const double al = coef[0];
    sx = al * ct_sign(u.x - v.x);
    sy = al * ct_sign(u.y - v.y);
    sz = al * ct_sign(u.z - v.z);
    sw = al * ct_sign(u.w - v.w);
  }
#pragma unroll
  for (int k = 1; k < KOPS; ++k) {
    const float4 v = a[(long)(k + 1) * per4 + i];
    const double be = coef[k];
    sx -= be * ct_sign(u.x - v.x);
    sy -= be * ct_sign(u.y - v.y);
    sz -= be * ct_sign(u.z - v.z);
    sw -= be * ct_sign(u.w - v.w);
  }
  float4 o;
  o.x = u.x <= 0.f ? 0.f : (float)(up * sx);
  o.y = u.y <= 0.f ? 0.f : (float)(up * sy);
  o.z = u.z <= 0.f ? 0.f : (float)(up * sz);
  o.w = u.w <= 0.f ? 0.f : (float)(up * sw);
  reinterpret_cast<float4*>(da)[i] = o;
}

// Finish of the L1 kinds.  partial [CT_TAPS][kops][CT_L1_PARTS]; counts.v[t] = the elements of the anchor's tap t.  Per tap:
//   d_ap = S_0 / count, d_an = sum_j S_j / count, term = d_ap / (d_an + 1e-7)  (ablation: term = d_ap), loss = sum_t weight_t term_t,
//   alpha = weight / (count (d_an + 1e-7)), beta_j = weight d_ap / (count (d_an + 1e-7)^2)  (ablation: weight / count, 0).
// One block: wave w sums the partials of value w, w + 4, .. (each lane 16 of them in ascending order, then the butterfly).
__global__ __launch_bounds__(256) void contrast_l1_finish_kernel(const double* __restrict__ partial, int kops, int ablation, CtCounts counts,
                                                                 float* __restrict__ loss, double* __restrict__ coef) {
  __shared__ double sums[CT_TAPS * CT_MAX_OPS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int v = wave; v < CT_TAPS * kops; v += 4) {
    const double* src = partial + (size_t)v * CT_L1_PARTS + lane * (CT_L1_PARTS / 64);
    double s = 0.0;
    for (int j = 0; j < CT_L1_PARTS / 64; ++j) s += src[j];
    s = ct_wave_sum(s);
    if (lane == 0) sums[v] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double weight[CT_TAPS] = {1.0 / 32, 1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0};
  double total = 0.0;
  for (int t = 0; t < CT_TAPS; ++t) {
    const double cnt = counts.v[t];
    const double dap = sums[t * kops] / cnt;
    double dan = 0.0;
    for (int k = 1; k < kops; ++k) dan += sums[t * kops + k] / cnt;
    double alpha, beta;
    if (ablation) {
      total += weight[t] * dap;
      alpha = weight[t] / cnt;
      beta = 0.0;
    } else {
      const double den = dan + 1e-7;
      total += weight[t] * (dap / den);
      alpha = weight[t] / (cnt * den);
      beta = weight[t] * dap / (cnt * den * den);
    }
    coef[t * kops] = alpha;
    for (int k = 1; k < kops; ++k) coef[t * kops + k] = beta;
  }
  loss[0] = (float)total;
}

// ---- cosine similarities --------------------------------------------------------------------------------------------------------------
// F.cosine_similarity(a, x, dim=1) as ATen computes it: sum_c (a_c / max(|a|, 1e-8)) (x_c / max(|x|, 1e-8)).  Here per pixel
// cos = (a . x) / (max(|a|, eps) max(|x|, eps)): a zero-norm vector gives cos = 0 and no 0 / 0 is formed.  The forward forms the dot
// product and the norms in float64 (the losses take exp(mean cos / 0.07) and then a difference of logarithms that nearly cancels:
// fp32 cosines cost the loss 1e-5 of its value); the backward's per-pixel arithmetic is fp32.  The clamp is
// written `n < eps ? eps : n`, which keeps a NaN norm.  16 lanes per pixel (C is 64 .. 512, contiguous), the LPIPS head's map; blocks
// (CT_COS_PARTS, b): a sample's pixels are walked by its own blocks only, so its sums do not depend on the batch.
constexpr float CT_COS_EPS = 1e-8f;
__device__ __forceinline__ float ct_clamp_eps(float n) { return n < CT_COS_EPS ? CT_COS_EPS : n; }
__device__ __forceinline__ double ct_clamp_eps(double n) { return n < 1e-8 ? 1e-8 : n; }

template <int KOPS>
__global__ __launch_bounds__(256) void contrast_cos_fwd_kernel(const float* __restrict__ f, double* __restrict__ partial, long hw, int c4,
                                                               int b) {
  __shared__ double red[CT_MAX_OPS][16];
  const int tid = threadIdx.x, lane = tid & 15, s = blockIdx.y;
  const long img4 = hw * c4;
  const float4* base = reinterpret_cast<const float4*>(f);
  double acc[KOPS];
#pragma unroll
  for (int k = 0; k < KOPS; ++k) acc[k] = 0.0;
  // every lane of a 16-lane group walks the same pixels, so the shuffles always see whole groups
  for (long pix = (long)blockIdx.x * 16 + (tid >> 4); pix < hw; pix += (long)CT_COS_PARTS * 16) {
    const float4* a = base + (size_t)s * img4 + pix * c4;
    // a product of two fp32 values is exact in float64: the sums over C are float64 reductions of exact terms
    double na = 0.0, dot[KOPS], nx[KOPS];
#pragma unroll
    for (int k = 0; k < KOPS; ++k) dot[k] = nx[k] = 0.0;
    for (int j = lane; j < c4; j += 16) {
      const float4 u = a[j];
      const double ux = u.x, uy = u.y, uz = u.z, uw = u.w;
      na += ux * ux + uy * uy + uz * uz + uw * uw;
#pragma unroll
      for (int k = 0; k < KOPS; ++k) {
        const float4 v = a[(size_t)(k + 1) * b * img4 + j];
        const double vx = v.x, vy = v.y, vz = v.z, vw = v.w;
        dot[k] += ux * vx + uy * vy + uz * vz + uw * vw;
        nx[k] += vx * vx + vy * vy + vz * vz + vw * vw;
      }
    }
    const double ma = ct_clamp_eps(sqrt(ct_group16_sum(na)));
#pragma unroll
    for (int k = 0; k < KOPS; ++k) {
      const double mx = ct_clamp_eps(sqrt(ct_group16_sum(nx[k])));
      acc[k] += ct_group16_sum(dot[k]) / (ma * mx);
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < KOPS; ++k) red[k][tid >> 4] = acc[k];
  }
  __syncthreads();
  if (tid < KOPS) {
    double t = 0.0;
    for (int g = 0; g < 16; ++g) t += red[tid][g];
    partial[((size_t)s * KOPS + tid) * CT_COS_PARTS + blockIdx.x] = t;
  }
}

// Backward: with ma = max(|a|, eps), mx = max(|x|, eps), cos as above,
//   d cos / d a_c = x_c / (mx ma) - [|a| > eps] cos a_c / (ma |a|)
// (the clamp passes no gradient below eps, and the norm's gradient at 0 is 0, as in ATen).  da_c = up * inv_hw * sum_k gamma[s][k] *
// d cos_k / d a_c, written through the ReLU mask (a_c <= 0 writes 0).  gamma = double [b][kops] on the device.  The pixel is read twice:
// the norms and dot products first, then da_c = ra * sum_k (g_k rx_k) x_kc - a_c * q * sum_k g_k cos_k with the k sums in ascending k.
template <int KOPS>
__global__ __launch_bounds__(256) void contrast_cos_bwd_kernel(const float* __restrict__ f, const double* __restrict__ gamma,
                                                               const float* __restrict__ upstream, float inv_hw, float* __restrict__ da,
                                                               long hw, int c4, int b) {
  const int tid = threadIdx.x, lane = tid & 15, s = blockIdx.y;
  const long img4 = hw * c4;
  const float4* base = reinterpret_cast<const float4*>(f);
  float4* out = reinterpret_cast<float4*>(da) + (size_t)s * img4;
  float g[KOPS];
#pragma unroll
  for (int k = 0; k < KOPS; ++k) g[k] = (float)gamma[(size_t)s * KOPS + k] * upstream[0] * inv_hw;
  for (long pix = (long)blockIdx.x * 16 + (tid >> 4); pix < hw; pix += (long)gridDim.x * 16) {
    const float4* a = base + (size_t)s * img4 + pix * c4;
    float na = 0.f, dot[KOPS], nx[KOPS];
#pragma unroll
    for (int k = 0; k < KOPS; ++k) dot[k] = nx[k] = 0.f;
    for (int j = lane; j < c4; j += 16) {
      const float4 u = a[j];
      na += u.x * u.x + u.y * u.y + u.z * u.z + u.w * u.w;
#pragma unroll
      for (int k = 0; k < KOPS; ++k) {
        const float4 v = a[(size_t)(k + 1) * b * img4 + j];
        dot[k] += u.x * v.x + u.y * v.y + u.z * v.z + u.w * v.w;
        nx[k] += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
      }
    }
    const float nrm = sqrtf(ct_group16_sum(na));
    const float ra = 1.f / ct_clamp_eps(nrm);
    // below eps the clamp holds the norm, and nothing flows through it (a NaN norm fails the comparison and passes on)
    const float q = nrm <= CT_COS_EPS ? 0.f : ra / nrm;
    float gx[KOPS], gc = 0.f;
#pragma unroll
    for (int k = 0; k < KOPS; ++k) {
      const float rx = 1.f / ct_clamp_eps(sqrtf(ct_group16_sum(nx[k])));
      gx[k] = g[k] * rx;
      gc += g[k] * (ct_group16_sum(dot[k]) * ra * rx);
    }
    const float qa = q * gc;
    for (int j = lane; j < c4; j += 16) {
      const float4 u = a[j];
      float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int k = 0; k < KOPS; ++k) {
        const float4 v = a[(size_t)(k + 1) * b * img4 + j];
        t.x += gx[k] * v.x;
        t.y += gx[k] * v.y;
        t.z += gx[k] * v.z;
        t.w += gx[k] * v.w;
      }
      float4 o;
      o.x = u.x <= 0.f ? 0.f : ra * t.x - u.x * qa;
      o.y = u.y <= 0.f ? 0.f : ra * t.y - u.y * qa;
      o.z = u.z <= 0.f ? 0.f : ra * t.z - u.z * qa;
      o.w = u.w <= 0.f ? 0.f : ra * t.w - u.w * qa;
      out[pix * c4 + j] = o;
    }
  }
}

// Finish of the cosine kinds.  partial [CT_TAPS][b][kops][CT_COS_PARTS]; counts.v[t] = h w of tap t.  Per tap and sample, with m_k the
// spatial mean of cos_k and E_k = exp(m_k / T), T = 0.07:
//   form 0 (ContrastCosineLoss):           term = -log(E_p / (E_n + 1e-7))         ablation: term = -log(E_p)
//   form 1 (NContrastCosineLoss):          term = -log(E_p / (sum_j E_nj + E_p))
// loss = mean_s sum_t weight_t term;  gamma[t][s][k] = weight_t / b * d term / d m_k.  One block; item (t, s) -> thread (t b + s) % 256,
// then the items' terms are summed by thread 0 in ascending (t, s) order from the scratch the block shares.
__global__ __launch_bounds__(256) void contrast_cos_finish_kernel(const double* __restrict__ partial, int b, int kops, int form, int ablation,
                                                                  CtCounts counts, float* __restrict__ loss, double* __restrict__ gamma,
                                                                  double* __restrict__ terms) {
  const double weight[CT_TAPS] = {1.0 / 32, 1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0};
  const double T = 0.07;
  for (int it = threadIdx.x; it < CT_TAPS * b; it += 256) {
    const int t = it / b;
    double e[CT_MAX_OPS], den = 0.0;
    for (int k = 0; k < kops; ++k) {
      const double* src = partial + ((size_t)it * kops + k) * CT_COS_PARTS;
      double s = 0.0;
      for (int j = 0; j < CT_COS_PARTS; ++j) s += src[j];
      e[k] = exp(s / counts.v[t] / T);
    }
    double* gm = gamma + (size_t)it * kops;
    const double wb = weight[t] / (double)b;
    double term;
    if (form == 0 && ablation) {
      term = -log(e[0]);
      gm[0] = -wb / T;
      for (int k = 1; k < kops; ++k) gm[k] = 0.0;
    } else if (form == 0) {
      den = e[1] + 1e-7;
      term = -log(e[0] / den);
      gm[0] = -wb / T;
      gm[1] = wb * e[1] / (T * den);
    } else {
      for (int k = 1; k < kops; ++k) den += e[k];
      den += e[0];
      term = -log(e[0] / den);
      gm[0] = wb * (e[0] / den - 1.0) / T;
      for (int k = 1; k < kops; ++k) gm[k] = wb * e[k] / (T * den);
    }
    terms[it] = weight[t] * term;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double total = 0.0;
  for (int it = 0; it < CT_TAPS * b; ++it) total += terms[it];
  loss[0] = (float)(total / (double)b);
}

template <int KOPS>
static void launch_l1_fwd(const float* f, double* partial, long per4, hipStream_t st) {
  hipLaunchKernelGGL(contrast_l1_fwd_kernel<KOPS>, dim3(CT_L1_PARTS), dim3(256), 0, st, f, partial, per4);
}
template <int KOPS>
static void launch_l1_bwd(const float* f, const double* coef, const float* up, float* da, long per4, hipStream_t st) {
  hipLaunchKernelGGL(contrast_l1_bwd_kernel<KOPS>, dim3(cdiv(per4, 256)), dim3(256), 0, st, f, coef, up, da, per4);
}
template <int KOPS>
static void launch_cos_fwd(const float* f, double* partial, long hw, int c4, int b, hipStream_t st) {
  hipLaunchKernelGGL(contrast_cos_fwd_kernel<KOPS>, dim3(CT_COS_PARTS, b), dim3(256), 0, st, f, partial, hw, c4, b);
}
template <int KOPS>
static void launch_cos_bwd(const float* f, const double* gamma, const float* up, float inv_hw, float* da, long hw, int c4, int b,
                           hipStream_t st) {
  const int gx = (int)(hw < 16 * 256 ? (hw + 15) / 16 : 256);
  hipLaunchKernelGGL(contrast_cos_bwd_kernel<KOPS>, dim3(gx, b), dim3(256), 0, st, f, gamma, up, inv_hw, da, hw, c4, b);
}

#define CT_DISPATCH(kops, fn, ...) \
  switch (kops) {                  \
    case 1: fn<1>(__VA_ARGS__); break; \
    case 2: fn<2>(__VA_ARGS__); break; \
    case 3: fn<3>(__VA_ARGS__); break; \
    case 4: fn<4>(__VA_ARGS__); break; \
    case 5: fn<5>(__VA_ARGS__); break; \
    case 6: fn<6>(__VA_ARGS__); break; \
    case 7: fn<7>(__VA_ARGS__); break; \
    case 8: fn<8>(__VA_ARGS__); break; \
    default: fn<9>(__VA_ARGS__); break; \
  }

static bool ct_counts(const long* tap_counts, CtCounts* out) {
  for (int t = 0; t < CT_TAPS; ++t) {
    if (tap_counts[t] <= 0) return false;
    out->v[t] = (double)tap_counts[t];
  }
  return true;
}

}  // namespace srhip

using namespace srhip;

extern "C" {

int srhip_maxpool2x2_floor_fwd(const float* x, float* y, int n, int h, int w, int c, void* stream) {
  SRHIP_REQUIRE(x && y, "maxpool2x2_floor_fwd: null tensor");
  SRHIP_REQUIRE(n > 0 && c > 0 && c % 4 == 0 && h >= 2 && w >= 2, "maxpool2x2_floor_fwd: needs C %% 4 == 0 and H, W >= 2");
  const int ho = h / 2, wo = w / 2;
  const long total = (long)n * ho * wo * (c / 4);
  SRHIP_REQUIRE(total <= 2147483647L * 256, "maxpool2x2_floor_fwd: tensor too large");
  hipLaunchKernelGGL(maxpool2x2_floor_kernel, dim3(cdiv(total, 256)), dim3(256), 0, as_stream(stream), x, y, h, w, c / 4, ho, wo, total);
  return check_launch("maxpool2x2_floor_fwd");
}

int srhip_maxpool2x2_floor_bwd(const float* x, const float* dy, const float* residual, float* dx, int n, int h, int w, int c, int relu,
                               void* stream) {
  SRHIP_REQUIRE(x && dy && dx, "maxpool2x2_floor_bwd: null tensor");
  SRHIP_REQUIRE(n > 0 && c > 0 && c % 4 == 0 && h >= 2 && w >= 2, "maxpool2x2_floor_bwd: needs C %% 4 == 0 and H, W >= 2");
  const long total = (long)n * h * w * (c / 4);
  SRHIP_REQUIRE(total <= 2147483647L * 256, "maxpool2x2_floor_bwd: tensor too large");
  hipLaunchKernelGGL(maxpool2x2_floor_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, as_stream(stream), x, dy, residual, dx, h, w,
                     c / 4, h / 2, w / 2, relu, total);
  return check_launch("maxpool2x2_floor_bwd");
}

int srhip_contrast_l1_parts(void) { return CT_L1_PARTS; }
int srhip_contrast_cos_parts(void) { return CT_COS_PARTS; }

int srhip_contrast_l1_fwd(const float* f, double* partial, int b, int kops, int h, int w, int c, void* stream) {
  SRHIP_REQUIRE(f && partial, "contrast_l1_fwd: null tensor");
  SRHIP_REQUIRE(b > 0 && kops >= 1 && kops <= CT_MAX_OPS && h > 0 && w > 0 && c > 0 && c % 4 == 0,
                "contrast_l1_fwd: needs C %% 4 == 0 and 1 <= operands <= 9");
  const long per4 = (long)b * h * w * (c / 4);
  CT_DISPATCH(kops, launch_l1_fwd, f, partial, per4, as_stream(stream));
  return check_launch("contrast_l1_fwd");
}

int srhip_contrast_l1_bwd(const float* f, const double* coef, const float* upstream, float* da, int b, int kops, int h, int w, int c,
                          void* stream) {
  SRHIP_REQUIRE(f && coef && upstream && da, "contrast_l1_bwd: null tensor");
  SRHIP_REQUIRE(b > 0 && kops >= 1 && kops <= CT_MAX_OPS && h > 0 && w > 0 && c > 0 && c % 4 == 0,
                "contrast_l1_bwd: needs C %% 4 == 0 and 1 <= operands <= 9");
  const long per4 = (long)b * h * w * (c / 4);
  SRHIP_REQUIRE(per4 <= 2147483647L * 256, "contrast_l1_bwd: tensor too large");
  CT_DISPATCH(kops, launch_l1_bwd, f, coef, upstream, da, per4, as_stream(stream));
  return check_launch("contrast_l1_bwd");
}

int srhip_contrast_l1_finish(const double* partial, const long* tap_counts, int kops, int ablation, float* loss, double* coef,
                             void* stream) {
  SRHIP_REQUIRE(partial && tap_counts && loss && coef, "contrast_l1_finish: null pointer");
  SRHIP_REQUIRE(kops >= 2 && kops <= CT_MAX_OPS, "contrast_l1_finish: needs the positive and 1 to 8 negatives");
  CtCounts counts;
  SRHIP_REQUIRE(ct_counts(tap_counts, &counts), "contrast_l1_finish: empty tap");
  hipLaunchKernelGGL(contrast_l1_finish_kernel, dim3(1), dim3(256), 0, as_stream(stream), partial, kops, ablation, counts, loss, coef);
  return check_launch("contrast_l1_finish");
}

int srhip_contrast_cos_fwd(const float* f, double* partial, int b, int kops, int h, int w, int c, void* stream) {
  SRHIP_REQUIRE(f && partial, "contrast_cos_fwd: null tensor");
  SRHIP_REQUIRE(b > 0 && b <= 65535 && kops >= 1 && kops <= CT_MAX_OPS && h > 0 && w > 0 && c > 0 && c % 4 == 0,
                "contrast_cos_fwd: needs C %% 4 == 0, 1 <= operands <= 9 and B <= 65535");
  CT_DISPATCH(kops, launch_cos_fwd, f, partial, (long)h * w, c / 4, b, as_stream(stream));
  return check_launch("contrast_cos_fwd");
}

int srhip_contrast_cos_bwd(const float* f, const double* gamma, const float* upstream, float* da, int b, int kops, int h, int w, int c,
                           void* stream) {
  SRHIP_REQUIRE(f && gamma && upstream && da, "contrast_cos_bwd: null tensor");
  SRHIP_REQUIRE(b > 0 && b <= 65535 && kops >= 1 && kops <= CT_MAX_OPS && h > 0 && w > 0 && c > 0 && c % 4 == 0,
                "contrast_cos_bwd: needs C %% 4 == 0, 1 <= operands <= 9 and B <= 65535");
  const long hw = (long)h * w;
  CT_DISPATCH(kops, launch_cos_bwd, f, gamma, upstream, 1.f / (float)hw, da, hw, c / 4, b, as_stream(stream));
  return check_launch("contrast_cos_bwd");
}

int srhip_contrast_cos_finish(const double* partial, const long* tap_counts, int b, int kops, int form, int ablation, float* loss,
                              double* gamma, double* terms, void* stream) {
  SRHIP_REQUIRE(partial && tap_counts && loss && gamma && terms, "contrast_cos_finish: null pointer");
  SRHIP_REQUIRE(b > 0 && kops >= 1 && kops <= CT_MAX_OPS && (form == 0 || form == 1), "contrast_cos_finish: needs 1 <= operands <= 9");
  SRHIP_REQUIRE(form == 1 ? kops >= 2 : kops == 2, "contrast_cos_finish: form 0 takes one negative, form 1 at least one");
  CtCounts counts;
  SRHIP_REQUIRE(ct_counts(tap_counts, &counts), "contrast_cos_finish: empty tap");
  hipLaunchKernelGGL(contrast_cos_finish_kernel, dim3(1), dim3(256), 0, as_stream(stream), partial, b, kops, form, ablation, counts, loss,
                     gamma, terms);
  return check_launch("contrast_cos_finish");
}

}  // extern "C"
