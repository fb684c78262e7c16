// Per-sample normalisations of the patch discriminator (+ the LeakyReLU that follows them), NHWC x[n][p][c], p = H * W
// (reference base_networks.py:1759-1767).  One family serves both kinds: `groups` groups of cpg = c / groups adjacent channels, one
// statistic over the m = p * cpg elements of one (sample, group).
//   instance norm (nn.InstanceNorm2d(C)): groups = c, biased variance, no affine (gamma = beta = null)
//   group norm (base_networks.py:12-31):  groups = 32, UNBIASED variance (x.var(-1)), per-channel weight and bias
// k = m / (m - 1) for the unbiased variance, 1 for the biased one; E = mean over one (sample, group):
//   forward    invstd = (k E[(x - mean)^2] + eps)^-1/2, xhat = (x - mean) invstd, z = xhat gamma_c + beta_c, y = lrelu(z)
//   backward   dz = dy lrelu'(z), a = dz gamma_c: dx = invstd (a - E[a] - k xhat E[a xhat]), dgamma_c = sum_{n,p} dz xhat, dbeta_c = sum dz
//   2nd order  (gradients of <u, dx>, mask constant) ubar = E[u], w = E[u xhat], pa = E[a], q = E[a xhat], T = E[u a] - ubar pa - k w q:
//              g_dy = gamma_c invstd (u - ubar - k xhat w) lrelu',  g_x = -k invstd^2 [q (u - ubar) + w (a - pa) + xhat (T - 2 k w q)],
//              g_gamma_c = sum_{n,p} dz invstd (u - ubar - k xhat w)
// Conventions are bn.hip's: the LeakyReLU mask is the sign of the pre-activation RECOMPUTED with the forward's own expression
// (gn_pre, contraction off: the same bits), so no pass reads y; forward = 2 reads + 1 write, backward = 4 reads + 1 write, second
// order = 6 reads + 2 writes.  Every pass is stage 1 (column sums per slab of <= rpb rows of ONE sample), stage 2 (one block per sample:
// the slabs in a fixed order -> column sums per (n, c) -> a fold of cpg adjacent columns per group), apply.  The geometry (gn_geom)
// depends on p alone and no sum crosses a sample, so y, dx, g_dy and g_x of a sample are bit-identical whatever else is in the batch;
// the per-channel parameter gradients are the (n, c) column sums added over n in a fixed order.  No atomics.
// The forward's sums are taken about a per-(sample, channel) shift (the sample's first row) and carried in fp64 (bn.hip's header
// comment explains why the shift alone is not enough); stage 2 moves them to the group mean in fp64.
#include "common.h"

namespace srhip {

constexpr int GN_ROWS = 64;        // rows of a stage-1 slab, until ...
constexpr int GN_MAXSLAB = 256;    // ... a sample would have more slabs than this
constexpr int GN_T2 = 1024;        // threads of a stage-2 block: c channels x (GN_T2 / c) slab lanes

struct GnGeom {
  int slabs;
  long rpb;
};
static GnGeom gn_geom(long p) {
  long s = (p + GN_ROWS - 1) / GN_ROWS;
  s = s > GN_MAXSLAB ? GN_MAXSLAB : (s < 1 ? 1 : s);
  const long rpb = (p + s - 1) / s;
  return {(int)((p + rpb - 1) / rpb), rpb};
}

// the forward's pre-activation; every pass that needs the LeakyReLU mask evaluates exactly this
__device__ __forceinline__ float gn_pre(float x, float mu, float is, float ga, float be) { return (x - mu) * is * ga + be; }

// what one thread needs about its four channels ch0 .. ch0 + 3 of sample n (a group may end inside the float4)
struct Gn4 {
  float mu[4], is[4], ga[4], be[4];
};
__device__ inline void gn_load4(Gn4& t, const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ gamma,
                                const float* __restrict__ beta, int n, int groups, int cpg, int ch0) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int g = n * groups + (ch0 + e) / cpg;
    t.mu[e] = mean[g];
    t.is[e] = invstd[g];
    t.ga[e] = gamma ? gamma[ch0 + e] : 1.f;
    t.be[e] = beta ? beta[ch0 + e] : 0.f;
  }
}

__device__ __forceinline__ void f4get(float (&o)[4], const float* p) {
  const float4 v = *reinterpret_cast<const float4*>(p);
  o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
}
__device__ __forceinline__ void f4put(float* p, const float (&o)[4]) { *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]); }

// the thread geometry of the stage-1 and apply kernels: grid (slabs, n), 256 threads = q channel quads x nrl row lanes
#define GN_LANES                                                                   \
  const int tid = threadIdx.x, n = blockIdx.y;                                     \
  const int q = c / 4, nrl = 256 / q;                                              \
  const int cq = tid % q, rl = tid / q;                                            \
  const long r0 = (long)blockIdx.x * rpb;                                          \
  const long r1 = r0 + rpb < p ? r0 + rpb : p;                                     \
  const size_t sample = (size_t)n * p * c

// block-wide: K sums of one thread's four channels -> partial[((n * slabs + slab) * K + k) * c + channel]
template <typename T, int K>
__device__ inline void gn_slab_write(T (&s)[K][4], T (*red)[256][4], T* __restrict__ partial, int tid, int q, int nrl, int c) {
  for (int k = 0; k < K; ++k)
    for (int e = 0; e < 4; ++e) red[k][tid][e] = s[k][e];
  __syncthreads();
  if (tid < q) {
    T* o = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * K * c;
    for (int k = 0; k < K; ++k)
      for (int e = 0; e < 4; ++e) {
        T a = s[k][e];
        for (int j = 1; j < nrl; ++j) a += red[k][j * q + tid][e];
        o[(size_t)k * c + tid * 4 + e] = a;
      }
  }
}

// stage 2, block-wide (GN_T2 threads): the K column sums of one sample over its slabs, in a fixed order -> col[k][channel]
template <typename T, int K>
__device__ inline void gn_colsum(const T* __restrict__ partial, int slabs, int c, T (*red)[GN_T2], T (*col)[GN_T2]) {
  const int t = threadIdx.x, nsub = GN_T2 / c, ch = t % c, sub = t / c;
  T a[K];
  for (int k = 0; k < K; ++k) a[k] = (T)0;
  if (sub < nsub)
    for (int s = sub; s < slabs; s += nsub)
      for (int k = 0; k < K; ++k) a[k] += partial[((size_t)s * K + k) * c + ch];
  for (int k = 0; k < K; ++k) red[k][t] = a[k];
  __syncthreads();
  if (t < c)
    for (int k = 0; k < K; ++k) {
      T v = red[k][t];
      for (int j = 1; j < nsub; ++j) v += red[k][j * c + t];
      col[k][t] = v;
    }
  __syncthreads();
}

// ---- forward, stage 1: per slab (sum d, sum d^2), d = x - shift exactly (fp64), shift = the sample's first row
__global__ __launch_bounds__(256) void gn_stats_stage1(const float* __restrict__ x, double* __restrict__ partial, long p, int c, long rpb) {
  __shared__ double red[2][256][4];
  GN_LANES;
  double s[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
  float sh[4];
  f4get(sh, x + sample + cq * 4);
  if (rl < nrl)
    for (long r = r0 + rl; r < r1; r += nrl) {
      float v[4];
      f4get(v, x + sample + (size_t)r * c + cq * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double d = (double)v[e] - (double)sh[e];
        s[0][e] += d;
        s[1][e] += d * d;
      }
    }
  gn_slab_write<double, 2>(s, red, partial, tid, q, nrl, c);
}

// ---- forward, stage 2: mean / invstd of every group of one sample
__global__ __launch_bounds__(GN_T2) void gn_stats_stage2(const double* __restrict__ partial, const float* __restrict__ x, float* __restrict__ mean,
                                                         float* __restrict__ invstd, int slabs, long p, int c, int groups, int unbiased, float eps) {
  __shared__ double red[2][GN_T2], col[2][GN_T2];
  const int n = blockIdx.x, t = threadIdx.x;
  gn_colsum<double, 2>(partial + (size_t)n * slabs * 2 * c, slabs, c, red, col);
  if (t < groups) {
    const int cpg = c / groups;
    const float* x0 = x + (size_t)n * p * c + t * cpg;        // the shifts of this group's channels
    const double m = (double)p * cpg;
    double tot = 0.0;
    for (int j = 0; j < cpg; ++j) tot += (double)x0[j] * (double)p + col[0][t * cpg + j];
    const double mu = tot / m;
    double ss = 0.0;                                           // sum (x - mu)^2 = sum_c [S2 - 2 (mu - shift) S1 + p (mu - shift)^2]
    for (int j = 0; j < cpg; ++j) {
      const double d = mu - (double)x0[j];
      ss += col[1][t * cpg + j] - 2.0 * d * col[0][t * cpg + j] + (double)p * d * d;
    }
    ss = ss > 0.0 ? ss : 0.0;
    const double var = ss / (unbiased ? m - 1.0 : m);
    mean[n * groups + t] = (float)mu;
    invstd[n * groups + t] = (float)(1.0 / sqrt(var + (double)eps));
  }
}

// ---- forward, apply
__global__ __launch_bounds__(256) void gn_apply_kernel(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ y, long p,
                                                       int c, long rpb, int groups, float slope, int act) {
  GN_LANES;
  if (rl >= nrl) return;
  Gn4 t;
  gn_load4(t, mean, invstd, gamma, beta, n, groups, c / groups, cq * 4);
  for (long r = r0 + rl; r < r1; r += nrl) {
    const size_t o = sample + (size_t)r * c + cq * 4;
    float v[4], out[4];
    f4get(v, x + o);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float z = gn_pre(v[e], t.mu[e], t.is[e], t.ga[e], t.be[e]);
      out[e] = (act && !(z > 0.f)) ? z * slope : z;
    }
    f4put(y + o, out);
  }
}

// ---- backward, stage 1: per slab and channel (sum dz, sum dz xhat)
__global__ __launch_bounds__(256) void gn_bwd_stage1(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ mean,
                                                     const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, float* __restrict__ partial, long p, int c, long rpb, int groups,
                                                     float slope, int act) {
  __shared__ float red[2][256][4];
  GN_LANES;
  Gn4 t;
  gn_load4(t, mean, invstd, gamma, beta, n, groups, c / groups, cq * 4);
  float s[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  if (rl < nrl)
    for (long r = r0 + rl; r < r1; r += nrl) {
      const size_t o = sample + (size_t)r * c + cq * 4;
      float g[4], v[4];
      f4get(g, dy + o);
      f4get(v, x + o);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xh = (v[e] - t.mu[e]) * t.is[e];
        const float dz = (act && !(gn_pre(v[e], t.mu[e], t.is[e], t.ga[e], t.be[e]) > 0.f)) ? g[e] * slope : g[e];
        s[0][e] += dz;
        s[1][e] += dz * xh;
      }
    }
  gn_slab_write<float, 2>(s, red, partial, tid, q, nrl, c);
}

// ---- backward, stage 2: coef[n][group] = (E[a], k E[a xhat]); csum[n][0 / 1][c] = the sample's (sum dz, sum dz xhat) per channel
__global__ __launch_bounds__(GN_T2) void gn_bwd_stage2(const float* __restrict__ partial, const float* __restrict__ gamma, float* __restrict__ coef,
                                                       float* __restrict__ csum, int slabs, long p, int c, int groups, float k) {
  __shared__ float red[2][GN_T2], col[2][GN_T2];
  const int n = blockIdx.x, t = threadIdx.x;
  gn_colsum<float, 2>(partial + (size_t)n * slabs * 2 * c, slabs, c, red, col);
  if (t < c && gamma != nullptr) {
    csum[((size_t)n * 2 + 0) * c + t] = col[0][t];
    csum[((size_t)n * 2 + 1) * c + t] = col[1][t];
  }
  if (t < groups) {
    const int cpg = c / groups;
    const float m = (float)p * (float)cpg;
    float pa = 0.f, qq = 0.f;
    for (int j = 0; j < cpg; ++j) {
      const float ga = gamma ? gamma[t * cpg + j] : 1.f;
      pa += ga * col[0][t * cpg + j];
      qq += ga * col[1][t * cpg + j];
    }
    coef[((size_t)n * groups + t) * 2 + 0] = pa / m;
    coef[((size_t)n * groups + t) * 2 + 1] = k * (qq / m);
  }
}

// out_j[c] = sum over the samples of csum[n][j][c], in the order of n; acc_j[c] += out_j[c] (this thread is the slot's only writer)
template <int K>
__global__ void gn_param_reduce(const float* __restrict__ csum, int nsamp, int c, float* __restrict__ out0, float* __restrict__ out1,
                                float* __restrict__ acc0, float* __restrict__ acc1) {
  const int ch = blockIdx.x * blockDim.x + threadIdx.x;
  if (ch >= c) return;
  float s[K];
  for (int j = 0; j < K; ++j) s[j] = 0.f;
  for (int n = 0; n < nsamp; ++n)
    for (int j = 0; j < K; ++j) s[j] += csum[((size_t)n * K + j) * c + ch];
  out0[ch] = s[0];
  if (acc0) acc0[ch] += s[0];
  if (K > 1) {
    out1[ch] = s[K - 1];
    if (acc1) acc1[ch] += s[K - 1];
  }
}

// ---- backward, apply: dx = invstd (a - E[a] - xhat k E[a xhat]) (+ addend, which may be dx itself)
__global__ __launch_bounds__(256) void gn_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ coef, const float* addend,
                                                           float* dx, long p, int c, long rpb, int groups, float slope, int act) {
  GN_LANES;
  if (rl >= nrl) return;
  const int cpg = c / groups;
  Gn4 t;
  gn_load4(t, mean, invstd, gamma, beta, n, groups, cpg, cq * 4);
  float pa[4], kq[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const size_t g = (size_t)n * groups + (cq * 4 + e) / cpg;
    pa[e] = coef[g * 2];
    kq[e] = coef[g * 2 + 1];
  }
  for (long r = r0 + rl; r < r1; r += nrl) {
    const size_t o = sample + (size_t)r * c + cq * 4;
    float g[4], v[4], out[4];
    f4get(g, dy + o);
    f4get(v, x + o);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float xh = (v[e] - t.mu[e]) * t.is[e];
      const float dz = (act && !(gn_pre(v[e], t.mu[e], t.is[e], t.ga[e], t.be[e]) > 0.f)) ? g[e] * slope : g[e];
      out[e] = t.is[e] * (dz * t.ga[e] - pa[e] - xh * kq[e]);
    }
    if (addend != nullptr) {
      float ad[4];
      f4get(ad, addend + o);
#pragma unroll
      for (int e = 0; e < 4; ++e) out[e] += ad[e];
    }
    f4put(dx + o, out);
  }
}

// ---- second order, stage 1: per slab and channel (sum u, sum u xhat, sum dz, sum dz xhat, sum u dz)
__global__ __launch_bounds__(256) void gn_bwd2_stage1(const float* __restrict__ u, const float* __restrict__ dy, const float* __restrict__ x,
                                                      const float* __restrict__ mean, const float* __restrict__ invstd,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ partial,
                                                      long p, int c, long rpb, int groups, float slope, int act) {
  __shared__ float red[5][256][4];
  GN_LANES;
  Gn4 t;
  gn_load4(t, mean, invstd, gamma, beta, n, groups, c / groups, cq * 4);
  float s[5][4];
  for (int k = 0; k < 5; ++k)
    for (int e = 0; e < 4; ++e) s[k][e] = 0.f;
  if (rl < nrl)
    for (long r = r0 + rl; r < r1; r += nrl) {
      const size_t o = sample + (size_t)r * c + cq * 4;
      float uu[4], g[4], v[4];
      f4get(uu, u + o);
      f4get(g, dy + o);
      f4get(v, x + o);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xh = (v[e] - t.mu[e]) * t.is[e];
        const float dz = (act && !(gn_pre(v[e], t.mu[e], t.is[e], t.ga[e], t.be[e]) > 0.f)) ? g[e] * slope : g[e];
        s[0][e] += uu[e];
        s[1][e] += uu[e] * xh;
        s[2][e] += dz;
        s[3][e] += dz * xh;
        s[4][e] += uu[e] * dz;
      }
    }
  gn_slab_write<float, 5>(s, red, partial, tid, q, nrl, c);
}

// ---- second order, stage 2: coef[n][group] = (ubar, w, pa, q, T - 2 k w q); gsum[n][c] = invstd (sum u dz - ubar sum dz - k w sum dz xhat)
__global__ __launch_bounds__(GN_T2) void gn_bwd2_stage2(const float* __restrict__ partial, const float* __restrict__ invstd,
                                                        const float* __restrict__ gamma, float* __restrict__ coef, float* __restrict__ gsum, int slabs,
                                                        long p, int c, int groups, float k) {
  __shared__ float red[5][GN_T2], col[5][GN_T2];
  const int n = blockIdx.x, t = threadIdx.x;
  const int cpg = c / groups;
  gn_colsum<float, 5>(partial + (size_t)n * slabs * 5 * c, slabs, c, red, col);      // (ends with a barrier: red is free again)
  if (t < groups) {
    const float m = (float)p * (float)cpg;
    float a[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < cpg; ++j) {
      const int ch = t * cpg + j;
      const float ga = gamma ? gamma[ch] : 1.f;
      a[0] += col[0][ch];
      a[1] += col[1][ch];
      a[2] += ga * col[2][ch];
      a[3] += ga * col[3][ch];
      a[4] += ga * col[4][ch];
    }
    const float ubar = a[0] / m, w = a[1] / m, pa = a[2] / m, qq = a[3] / m;
    const float T = a[4] / m - ubar * pa - k * w * qq;
    float* o = coef + ((size_t)n * groups + t) * 5;
    o[0] = ubar;
    o[1] = w;
    o[2] = pa;
    o[3] = qq;
    o[4] = T - 2.f * k * w * qq;
    red[0][t] = ubar;
    red[1][t] = w;
  }
  __syncthreads();
  if (t < c && gamma != nullptr) {
    const int g = t / cpg;
    gsum[(size_t)n * c + t] = invstd[n * groups + g] * (col[4][t] - red[0][g] * col[2][t] - k * red[1][g] * col[3][t]);
  }
}

// ---- second order, apply
__global__ __launch_bounds__(256) void gn_bwd2_apply_kernel(const float* __restrict__ u, const float* __restrict__ dy, const float* __restrict__ x,
                                                            const float* __restrict__ mean, const float* __restrict__ invstd,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const float* __restrict__ coef, float* __restrict__ g_dy, float* __restrict__ g_x, long p,
                                                            int c, long rpb, int groups, float k, float slope, int act) {
  GN_LANES;
  if (rl >= nrl) return;
  const int cpg = c / groups;
  Gn4 t;
  gn_load4(t, mean, invstd, gamma, beta, n, groups, cpg, cq * 4);
  float ub[4], ww[4], pa[4], qq[4], rr[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float* o = coef + ((size_t)n * groups + (cq * 4 + e) / cpg) * 5;
    ub[e] = o[0]; ww[e] = o[1]; pa[e] = o[2]; qq[e] = o[3]; rr[e] = o[4];
  }
  for (long r = r0 + rl; r < r1; r += nrl) {
    const size_t o = sample + (size_t)r * c + cq * 4;
    float uu[4], g[4], v[4], od[4], ox[4];
    f4get(uu, u + o);
    f4get(g, dy + o);
    f4get(v, x + o);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float xh = (v[e] - t.mu[e]) * t.is[e];
      const float mk = (act && !(gn_pre(v[e], t.mu[e], t.is[e], t.ga[e], t.be[e]) > 0.f)) ? slope : 1.f;
      const float a = g[e] * mk * t.ga[e];
      const float du = uu[e] - ub[e];
      od[e] = t.ga[e] * t.is[e] * (du - k * xh * ww[e]) * mk;
      ox[e] = -k * t.is[e] * t.is[e] * (qq[e] * du + ww[e] * (a - pa[e]) + xh * rr[e]);
    }
    f4put(g_dy + o, od);
    f4put(g_x + o, ox);
  }
}

#undef GN_LANES

// the workspace, in floats: [stage-1 partials: n slabs 5 c][coef: <= n c 5][per-(n, c) sums: n 2 c]; the forward's fp64 partials (n slabs
// 2 c doubles) fit the first region
static size_t gn_partial_floats(long n, long p, int c) { return (size_t)n * gn_geom(p).slabs * 5 * c; }

static int gn_check(const char* what, const void* ws, size_t ws_bytes, long n, long p, int c, int groups) {
  SRHIP_REQUIRE(n > 0 && n <= 65535 && p > 0, "%s: n must be in 1 .. 65535 and p positive", what);
  SRHIP_REQUIRE(c >= 4 && c % 4 == 0 && c <= 1024, "%s: C must be a multiple of 4, <= 1024", what);
  SRHIP_REQUIRE(groups > 0 && c % groups == 0, "%s: C must be a multiple of the groups", what);
  SRHIP_REQUIRE(p * (c / groups) >= 2, "%s: a statistic needs at least two elements (p * C / groups)", what);
  SRHIP_REQUIRE(ws && ((uintptr_t)ws & 15) == 0 && ws_bytes >= srhip_gn_workspace(n, p, c), "%s: workspace too small or not 16-byte aligned", what);
  return SRHIP_OK;
}

}  // namespace srhip

using namespace srhip;

extern "C" {

size_t srhip_gn_workspace(long n, long p, int c) {
  if (n <= 0 || p <= 0 || c <= 0) return 0;
  return (gn_partial_floats(n, p, c) + (size_t)n * c * 7) * sizeof(float);
}

int srhip_gn_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* invstd, void* workspace,
                 size_t workspace_bytes, long n, long p, int c, int groups, int unbiased, float eps, float slope, int apply_act, void* stream) {
  SRHIP_REQUIRE(x && y && mean && invstd, "gn_fwd: null tensor");
  SRHIP_REQUIRE((gamma == nullptr) == (beta == nullptr), "gn_fwd: gamma and beta are given or left out together");
  if (int rc = gn_check("gn_fwd", workspace, workspace_bytes, n, p, c, groups)) return rc;
  hipStream_t st = as_stream(stream);
  const GnGeom g = gn_geom(p);
  double* part = static_cast<double*>(workspace);
  const dim3 grid(g.slabs, (unsigned)n);
  hipLaunchKernelGGL(gn_stats_stage1, grid, dim3(256), 0, st, x, part, p, c, g.rpb);
  hipLaunchKernelGGL(gn_stats_stage2, dim3((unsigned)n), dim3(GN_T2), 0, st, part, x, mean, invstd, g.slabs, p, c, groups, unbiased, eps);
  hipLaunchKernelGGL(gn_apply_kernel, grid, dim3(256), 0, st, x, mean, invstd, gamma, beta, y, p, c, g.rpb, groups, slope, apply_act);
  return check_launch("gn_fwd");
}

int srhip_gn_bwd(const float* dy, const float* x, const float* gamma, const float* beta, const float* mean, const float* invstd,
                 const float* addend, float* dx, float* dgamma, float* dbeta, float* acc_gamma, float* acc_beta, void* workspace,
                 size_t workspace_bytes, long n, long p, int c, int groups, int unbiased, float slope, int apply_act, void* stream) {
  SRHIP_REQUIRE(dy && x && mean && invstd && dx, "gn_bwd: null tensor");
  SRHIP_REQUIRE((gamma == nullptr) == (beta == nullptr), "gn_bwd: gamma and beta are given or left out together");
  SRHIP_REQUIRE(gamma ? (dgamma && dbeta) : (!acc_gamma && !acc_beta), "gn_bwd: dgamma and dbeta go with gamma, no slots without it");
  if (int rc = gn_check("gn_bwd", workspace, workspace_bytes, n, p, c, groups)) return rc;
  hipStream_t st = as_stream(stream);
  const GnGeom g = gn_geom(p);
  float* part = static_cast<float*>(workspace);
  float* coef = part + gn_partial_floats(n, p, c);
  float* csum = coef + (size_t)n * c * 5;
  const float m = (float)p * (float)(c / groups);
  const float k = unbiased ? m / (m - 1.f) : 1.f;
  const dim3 grid(g.slabs, (unsigned)n);
  hipLaunchKernelGGL(gn_bwd_stage1, grid, dim3(256), 0, st, dy, x, mean, invstd, gamma, beta, part, p, c, g.rpb, groups, slope, apply_act);
  hipLaunchKernelGGL(gn_bwd_stage2, dim3((unsigned)n), dim3(GN_T2), 0, st, part, gamma, coef, csum, g.slabs, p, c, groups, k);
  if (gamma)
    hipLaunchKernelGGL(gn_param_reduce<2>, dim3(cdiv(c, 256)), dim3(256), 0, st, csum, (int)n, c, dbeta, dgamma, acc_beta, acc_gamma);
  hipLaunchKernelGGL(gn_bwd_apply_kernel, grid, dim3(256), 0, st, dy, x, mean, invstd, gamma, beta, coef, addend, dx, p, c, g.rpb, groups,
                     slope, apply_act);
  return check_launch("gn_bwd");
}

int srhip_gn_bwd_bwd(const float* u, const float* dy, const float* x, const float* gamma, const float* beta, const float* mean,
                     const float* invstd, float* g_dy, float* g_x, float* g_gamma, float* acc_gamma, void* workspace, size_t workspace_bytes,
                     long n, long p, int c, int groups, int unbiased, float slope, int apply_act, void* stream) {
  SRHIP_REQUIRE(u && dy && x && mean && invstd && g_dy && g_x, "gn_bwd_bwd: null tensor");
  SRHIP_REQUIRE((gamma == nullptr) == (beta == nullptr), "gn_bwd_bwd: gamma and beta are given or left out together");
  SRHIP_REQUIRE(gamma ? g_gamma != nullptr : !acc_gamma, "gn_bwd_bwd: g_gamma goes with gamma, no slot without it");
  if (int rc = gn_check("gn_bwd_bwd", workspace, workspace_bytes, n, p, c, groups)) return rc;
  hipStream_t st = as_stream(stream);
  const GnGeom g = gn_geom(p);
  float* part = static_cast<float*>(workspace);
  float* coef = part + gn_partial_floats(n, p, c);
  float* gsum = coef + (size_t)n * c * 5;
  const float m = (float)p * (float)(c / groups);
  const float k = unbiased ? m / (m - 1.f) : 1.f;
  const dim3 grid(g.slabs, (unsigned)n);
  hipLaunchKernelGGL(gn_bwd2_stage1, grid, dim3(256), 0, st, u, dy, x, mean, invstd, gamma, beta, part, p, c, g.rpb, groups, slope, apply_act);
  hipLaunchKernelGGL(gn_bwd2_stage2, dim3((unsigned)n), dim3(GN_T2), 0, st, part, invstd, gamma, coef, gsum, g.slabs, p, c, groups, k);
  if (gamma)
    hipLaunchKernelGGL(gn_param_reduce<1>, dim3(cdiv(c, 256)), dim3(256), 0, st, gsum, (int)n, c, g_gamma, (float*)nullptr, acc_gamma,
                       (float*)nullptr);
  hipLaunchKernelGGL(gn_bwd2_apply_kernel, grid, dim3(256), 0, st, u, dy, x, mean, invstd, gamma, beta, coef, g_dy, g_x, p, c, g.rpb, groups, k,
                     slope, apply_act);
  return check_launch("gn_bwd_bwd");
}

}  // extern "C"
