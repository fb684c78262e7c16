// AMSSRN's attention and residual passes (SRADSGAN/model/amssrn.py:93-165, 280-334):
//   * non-local attention on image quadrants (Nonlocal_CA): the map is split at H1 = h / 2, W1 = w / 2 (unequal quadrants for odd
//     sizes) and every quadrant runs y = softmax(theta^T phi) g with 8 inter channels and unscaled energies.  The quadrant of a
//     pixel is found from its coordinates, so no quadrant is gathered; no N x N tensor is written.  One thread per query pixel walks
//     the keys of its quadrant with an online softmax in exact fp32 (expf); the forward keeps the row maximum m and the row sum l
//     per query for the backward.  Backward in two passes, no atomics (bit-identical reruns): per query i, D_i = dy_i . y_i and
//     dtheta_i = sum_j P_ij (dy_i . g_j - D_i) phi_j; per key j, dphi_j = sum_i P_ij (dy_i . g_j - D_i) theta_i and
//     dg_j = sum_i P_ij dy_i, with P_ij = exp(theta_i . phi_j - m_i) / l_i recomputed.
//   * the learned scalar residual x = block(x) + gamma * non_local_1 with gamma on the device, and its backward: db = gamma * g and
//     the fixed-order partials of sum(g * b) (reduced by srhip_prelu_slope_reduce).
// theta, phi, g, y and their gradients are NHWC tensors of 8 channels (32-byte pixel rows, 16-byte aligned).
#include "common.h"

namespace srhip {

constexpr int NL_C = 8;
constexpr int GAMMA_PARTS = 512;

__device__ __forceinline__ void load8(const float* p, float* v) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void store8(float* p, const float* v) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}
__device__ __forceinline__ float dot8(const float* a, const float* b) {
  float s = a[0] * b[0];
#pragma unroll
  for (int c = 1; c < NL_C; ++c) s += a[c] * b[c];
  return s;
}

struct Quad {
  int img, r0, r1, c0, c1;
};
__device__ __forceinline__ Quad quad_of(long p, int h, int w) {
  Quad q;
  q.img = (int)(p / ((long)h * w));
  const int r = (int)(p - (long)q.img * h * w), hh = r / w, ww = r - (r / w) * w;
  const int h1 = h / 2, w1 = w / 2;
  q.r0 = hh < h1 ? 0 : h1;
  q.r1 = hh < h1 ? h1 : h;
  q.c0 = ww < w1 ? 0 : w1;
  q.c1 = ww < w1 ? w1 : w;
  return q;
}

__global__ __launch_bounds__(256) void nl_quad_fwd_kernel(const float* __restrict__ th, const float* __restrict__ ph,
                                                          const float* __restrict__ g, float* __restrict__ y, float* __restrict__ ml,
                                                          int n, int h, int w) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long)n * h * w) return;
  const Quad q = quad_of(p, h, w);
  float t[NL_C], acc[NL_C], k[NL_C], v[NL_C];
  load8(th + p * NL_C, t);
#pragma unroll
  for (int c = 0; c < NL_C; ++c) acc[c] = 0.f;
  float m = -INFINITY, l = 0.f;
  for (int kr = q.r0; kr < q.r1; ++kr) {
    const long row = ((long)q.img * h + kr) * w;
    for (int kc = q.c0; kc < q.c1; ++kc) {
      const long j = row + kc;
      load8(ph + j * NL_C, k);
      const float s = dot8(t, k);
      if (s > m) {
        const float sc = expf(m - s);
        l *= sc;
#pragma unroll
        for (int c = 0; c < NL_C; ++c) acc[c] *= sc;
        m = s;
      }
      const float e = expf(s - m);
      l += e;
      load8(g + j * NL_C, v);
#pragma unroll
      for (int c = 0; c < NL_C; ++c) acc[c] += e * v[c];
    }
  }
#pragma unroll
  for (int c = 0; c < NL_C; ++c) acc[c] = acc[c] / l;
  store8(y + p * NL_C, acc);
  ml[2 * p] = m;
  ml[2 * p + 1] = l;
}

// per query i: D_i = dy_i . y_i, dtheta_i
__global__ __launch_bounds__(256) void nl_quad_bwd_q_kernel(const float* __restrict__ th, const float* __restrict__ ph,
                                                            const float* __restrict__ g, const float* __restrict__ y,
                                                            const float* __restrict__ ml, const float* __restrict__ dy,
                                                            float* __restrict__ dd, float* __restrict__ dth, int n, int h, int w) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long)n * h * w) return;
  const Quad q = quad_of(p, h, w);
  float t[NL_C], o[NL_C], k[NL_C], v[NL_C], acc[NL_C];
  load8(th + p * NL_C, t);
  load8(dy + p * NL_C, o);
  load8(y + p * NL_C, v);
  const float D = dot8(o, v);
  const float m = ml[2 * p], l = ml[2 * p + 1];
#pragma unroll
  for (int c = 0; c < NL_C; ++c) acc[c] = 0.f;
  for (int kr = q.r0; kr < q.r1; ++kr) {
    const long row = ((long)q.img * h + kr) * w;
    for (int kc = q.c0; kc < q.c1; ++kc) {
      const long j = row + kc;
      load8(ph + j * NL_C, k);
      load8(g + j * NL_C, v);
      const float P = expf(dot8(t, k) - m) / l;
      const float ds = P * (dot8(o, v) - D);
#pragma unroll
      for (int c = 0; c < NL_C; ++c) acc[c] += ds * k[c];
    }
  }
  store8(dth + p * NL_C, acc);
  dd[p] = D;
}

// per key j: dphi_j, dg_j
__global__ __launch_bounds__(256) void nl_quad_bwd_k_kernel(const float* __restrict__ th, const float* __restrict__ ph,
                                                            const float* __restrict__ g, const float* __restrict__ ml,
                                                            const float* __restrict__ dy, const float* __restrict__ dd,
                                                            float* __restrict__ dph, float* __restrict__ dg, int n, int h, int w) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long)n * h * w) return;
  const Quad q = quad_of(p, h, w);
  float k[NL_C], v[NL_C], t[NL_C], o[NL_C], ak[NL_C], av[NL_C];
  load8(ph + p * NL_C, k);
  load8(g + p * NL_C, v);
#pragma unroll
  for (int c = 0; c < NL_C; ++c) ak[c] = av[c] = 0.f;
  for (int qr = q.r0; qr < q.r1; ++qr) {
    const long row = ((long)q.img * h + qr) * w;
    for (int qc = q.c0; qc < q.c1; ++qc) {
      const long i = row + qc;
      load8(th + i * NL_C, t);
      load8(dy + i * NL_C, o);
      const float P = expf(dot8(t, k) - ml[2 * i]) / ml[2 * i + 1];
      const float ds = P * (dot8(o, v) - dd[i]);
#pragma unroll
      for (int c = 0; c < NL_C; ++c) {
        ak[c] += ds * t[c];
        av[c] += P * o[c];
      }
    }
  }
  store8(dph + p * NL_C, ak);
  store8(dg + p * NL_C, av);
}

__global__ __launch_bounds__(256) void gamma_res_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                            const float* __restrict__ gamma, float* __restrict__ out, long n4) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float s = *gamma;
  const float4 x = reinterpret_cast<const float4*>(a)[i], z = reinterpret_cast<const float4*>(b)[i];
  reinterpret_cast<float4*>(out)[i] = make_float4(x.x + s * z.x, x.y + s * z.y, x.z + s * z.z, x.w + s * z.w);
}

// db = gamma * g (db may be NULL), partials[block] = fixed-order sum of g * b over the block's items
__global__ __launch_bounds__(256) void gamma_res_bwd_kernel(const float* __restrict__ g, const float* __restrict__ b,
                                                            const float* __restrict__ gamma, float* __restrict__ db,
                                                            float* __restrict__ partials, long n4) {
  __shared__ float red[4];
  const float s = *gamma;
  float acc = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)GAMMA_PARTS * 256) {
    const float4 x = reinterpret_cast<const float4*>(g)[i], z = reinterpret_cast<const float4*>(b)[i];
    acc += x.x * z.x;
    acc += x.y * z.y;
    acc += x.z * z.z;
    acc += x.w * z.w;
    if (db) reinterpret_cast<float4*>(db)[i] = make_float4(s * x.x, s * x.y, s * x.z, s * x.w);
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

static bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

}  // namespace srhip

using namespace srhip;

extern "C" {

int srhip_nl_quad_fwd(const float* theta, const float* phi, const float* g, float* y, float* ml, int n, int h, int w, void* stream) {
  SRHIP_REQUIRE(theta && phi && g && y && ml, "nl_quad_fwd: null tensor");
  SRHIP_REQUIRE(n > 0 && h >= 2 && w >= 2, "nl_quad_fwd: needs n > 0, h >= 2, w >= 2 (four non-empty quadrants)");
  SRHIP_REQUIRE(al16(theta) && al16(phi) && al16(g) && al16(y), "nl_quad_fwd: 16-byte aligned tensors");
  const long px = (long)n * h * w;
  hipLaunchKernelGGL(nl_quad_fwd_kernel, dim3(cdiv(px, 256)), dim3(256), 0, as_stream(stream), theta, phi, g, y, ml, n, h, w);
  return check_launch("nl_quad_fwd");
}

int srhip_nl_quad_bwd(const float* theta, const float* phi, const float* g, const float* y, const float* ml, const float* dy, float* dd,
                      float* dtheta, float* dphi, float* dg, int n, int h, int w, void* stream) {
  SRHIP_REQUIRE(theta && phi && g && y && ml && dy && dd && dtheta && dphi && dg, "nl_quad_bwd: null tensor");
  SRHIP_REQUIRE(n > 0 && h >= 2 && w >= 2, "nl_quad_bwd: needs n > 0, h >= 2, w >= 2");
  SRHIP_REQUIRE(al16(theta) && al16(phi) && al16(g) && al16(y) && al16(dy) && al16(dtheta) && al16(dphi) && al16(dg),
                "nl_quad_bwd: 16-byte aligned tensors");
  const long px = (long)n * h * w;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(nl_quad_bwd_q_kernel, dim3(cdiv(px, 256)), dim3(256), 0, st, theta, phi, g, y, ml, dy, dd, dtheta, n, h, w);
  int rc = check_launch("nl_quad_bwd (queries)");
  if (rc) return rc;
  hipLaunchKernelGGL(nl_quad_bwd_k_kernel, dim3(cdiv(px, 256)), dim3(256), 0, st, theta, phi, g, ml, dy, dd, dphi, dg, n, h, w);
  return check_launch("nl_quad_bwd (keys)");
}

int srhip_gamma_parts(void) { return GAMMA_PARTS; }

int srhip_gamma_res_fwd(const float* a, const float* b, const float* gamma, float* out, long count, void* stream) {
  SRHIP_REQUIRE(a && b && gamma && out && count > 0 && count % 4 == 0 && al16(a) && al16(b) && al16(out),
                "gamma_res_fwd: dense 16-byte aligned tensors, count % 4 == 0");
  hipLaunchKernelGGL(gamma_res_fwd_kernel, dim3(cdiv(count / 4, 256)), dim3(256), 0, as_stream(stream), a, b, gamma, out, count / 4);
  return check_launch("gamma_res_fwd");
}

int srhip_gamma_res_bwd(const float* g, const float* b, const float* gamma, float* db, float* partials, long count, void* stream) {
  SRHIP_REQUIRE(g && b && gamma && partials && count > 0 && count % 4 == 0 && al16(g) && al16(b) && (!db || al16(db)),
                "gamma_res_bwd: dense 16-byte aligned tensors, count % 4 == 0");
  hipLaunchKernelGGL(gamma_res_bwd_kernel, dim3(GAMMA_PARTS), dim3(256), 0, as_stream(stream), g, b, gamma, db, partials, count / 4);
  return check_launch("gamma_res_bwd");
}

}  // extern "C"
