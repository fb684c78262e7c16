// Kernels of the diffusion model (model/gdp.py: the reference's GDP_x0 U-Net and GaussianDiffusion.p_sample_loop), gfx950.
// Everything here is exact fp32 (no atomics, fixed summation orders: re-runs are bit-identical) and does not
// move with srhip_set_conv_math.  Tensors are NHWC: `rows` pixel rows of `c` channels, with a row stride where a caller reads or
// writes a channel slice of a wider buffer.
//
//   GroupNorm(32, C) [+ (1 + scale) / shift modulation] [+ SiLU]   normalization(), ResBlock._forward with use_scale_shift_norm
//     stage 1  grid (chunks of 64 pixel rows, n): per group the chunk's mean and the sum of squares about THAT mean
//     stage 2  grid n: the chunks folded in a fixed order (Chan et al.'s pairwise update, fp64; 32 runs of chunks per group, then the
//              runs) -> mean, 1 / sqrt(var + eps)
//     apply    elementwise
//     A sample's statistics read that sample only, so its output does not depend on the batch it sits in.
//   2 x 2 average pool                                               Downsample(use_conv=False): ((a + b) + c + d) * 0.25
//   multi-head self-attention, flash style                           QKVAttentionLegacy on the qkv rows [n, t, heads * 3 * ch]
//     One wave owns 32 queries of one (sample, head) and walks the keys 32 at a time with v_mfma_f32_32x32x2_f32:
//       S^T[key][query] = K Q^T      A = K rows, B = Q rows, both scaled by ch^-1/4; lane half h contracts channels [h ch/2, (h+1) ch/2)
//       online soft-max per query    a query is a COLUMN of S^T, i.e. one lane of each half: 16 values in registers + one exchange
//       O^T[c][query] += V^T P^T     the accumulator tile P^T is the B operand as it stands (its row index = the key is the k index of
//                                    the lane half), A = V read by rows: no LDS, no T x T tensor anywhere
//     Keys past t are masked to -inf before the maximum, queries past t are computed on a clamped row and not stored.
//   sampler update                                                   p_mean_variance + p_sample in one pass, noise supplied or drawn
//   normal draws                                                     Philox4x32-10 keyed by (seed, step), counter = element / 4; Box-Muller
//   output quantisation                                              tensor2img: clamp, [0, 1], x 255, round half to even, uint8
// The second half of the file holds the backward kernels of the training step (model/gdp_train.py): GroupNorm, SiLU and average-pool
// backward, the attention forward's lse-emitting form (the same kernel body) with a two-kernel flash-style backward, and q_sample.
#include <cmath>

#include "common.h"
#include "philox.h"

namespace srhip {

constexpr int DG_GROUPS = 32;     // GroupNorm32(32, C)
constexpr int DG_ROWS = 64;       // pixel rows per stage-1 block
constexpr int DG_MAXC = 2048;     // the decoder's widest concatenated input
constexpr int DG_THREADS = 256;
constexpr int DG_SEGS = 32;       // stage 2: segments of the chunk list per group

// rows of a chunk are dealt to `nsub` interleaved sub-sums per channel; a function of C alone, so that the summation order (and with
// it every bit of the result) does not depend on which load width serves the tensor
__host__ __device__ inline int dg_nsub(int c) { return c >= 1024 ? 1 : 1024 / c; }

template <int V>
struct dg_vec;
template <>
struct dg_vec<1> {
  float v[1];
  __device__ __forceinline__ void load(const float* p) { v[0] = *p; }
};
template <>
struct dg_vec<4> {
  float v[4];
  __device__ __forceinline__ void load(const float* p) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  }
};

// ---- GroupNorm ----------------------------------------------------------------------------------------------------------- //
// part[((img * chunks + chunk) * 32 + g) * 2] = {mean, M2} of the chunk's rows x the group's channels.  V channels per thread.
template <int V>
__global__ void __launch_bounds__(DG_THREADS) diff_gn_stage1(const float* __restrict__ x, long ldx, float* __restrict__ part, long p, int c) {
  __shared__ float sh[DG_MAXC];
  __shared__ float gmean[DG_GROUPS];
  const int tid = threadIdx.x;
  const long chunk = blockIdx.x, img = blockIdx.y;
  const long r0 = chunk * DG_ROWS;
  const int rows = (int)(p - r0 < DG_ROWS ? p - r0 : DG_ROWS);
  const int cg = c / DG_GROUPS, nsub = dg_nsub(c), cv = c / V;
  const float* base = x + (img * p + r0) * ldx;
  for (int idx = tid; idx < cv * nsub; idx += DG_THREADS) {
    const int sub = idx / cv, ch = (idx - sub * cv) * V;
    float s[V];
#pragma unroll
    for (int k = 0; k < V; ++k) s[k] = 0.f;
#pragma unroll 4
    for (int r = sub; r < rows; r += nsub) {
      dg_vec<V> t;
      t.load(base + (long)r * ldx + ch);
#pragma unroll
      for (int k = 0; k < V; ++k) s[k] += t.v[k];
    }
#pragma unroll
    for (int k = 0; k < V; ++k) sh[sub * c + ch + k] = s[k];
  }
  __syncthreads();
  if (tid < DG_GROUPS) {
    float s = 0.f;
    for (int sub = 0; sub < nsub; ++sub)
      for (int j = 0; j < cg; ++j) s += sh[sub * c + tid * cg + j];
    gmean[tid] = s / (float)(rows * cg);
  }
  __syncthreads();
  for (int idx = tid; idx < cv * nsub; idx += DG_THREADS) {
    const int sub = idx / cv, ch = (idx - sub * cv) * V;
    float m[V], q[V];
#pragma unroll
    for (int k = 0; k < V; ++k) m[k] = gmean[(ch + k) / cg], q[k] = 0.f;
#pragma unroll 4
    for (int r = sub; r < rows; r += nsub) {
      dg_vec<V> t;
      t.load(base + (long)r * ldx + ch);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float d = t.v[k] - m[k];
        q[k] += d * d;
      }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) sh[sub * c + ch + k] = q[k];
  }
  __syncthreads();
  if (tid < DG_GROUPS) {
    float q = 0.f;
    for (int sub = 0; sub < nsub; ++sub)
      for (int j = 0; j < cg; ++j) q += sh[sub * c + tid * cg + j];
    float* o = part + ((img * gridDim.x + chunk) * DG_GROUPS + tid) * 2;
    o[0] = gmean[tid];
    o[1] = q;
  }
}

// Chan et al.'s update of (count, mean, M2) by another such triple, in fp64
__device__ __forceinline__ void dg_merge(double& na, double& mean, double& m2, double nb, double mb, double m2b) {
  if (nb == 0.0) return;
  const double delta = mb - mean, tot = na + nb;
  mean += delta * nb / tot;
  m2 += m2b + delta * delta * na * nb / tot;
  na = tot;
}

// stats[(img * 32 + g) * 2] = {mean, 1 / sqrt(biased variance + eps)}.  grid n, block 32 groups x DG_SEGS segments: a thread folds its
// contiguous run of chunks in chunk order, then one thread per group folds the segments in segment order.
__global__ void __launch_bounds__(DG_GROUPS* DG_SEGS) diff_gn_stage2(const float* __restrict__ part, float* __restrict__ stats, long p, int c,
                                                                     long chunks, float eps) {
  __shared__ double sn[DG_SEGS][DG_GROUPS], sm[DG_SEGS][DG_GROUPS], sq[DG_SEGS][DG_GROUPS];
  const int g = threadIdx.x % DG_GROUPS, seg = threadIdx.x / DG_GROUPS;
  const long img = blockIdx.x;
  const int cg = c / DG_GROUPS;
  const long per = (chunks + DG_SEGS - 1) / DG_SEGS;
  const long k0 = seg * per, k1 = k0 + per < chunks ? k0 + per : chunks;
  double na = 0.0, mean = 0.0, m2 = 0.0;
  for (long k = k0; k < k1; ++k) {
    const long r0 = k * DG_ROWS;
    const float* q = part + ((img * chunks + k) * DG_GROUPS + g) * 2;
    dg_merge(na, mean, m2, (double)((p - r0 < DG_ROWS ? p - r0 : DG_ROWS) * cg), (double)q[0], (double)q[1]);
  }
  sn[seg][g] = na, sm[seg][g] = mean, sq[seg][g] = m2;
  __syncthreads();
  if (seg == 0) {
    for (int s = 1; s < DG_SEGS; ++s) dg_merge(na, mean, m2, sn[s][g], sm[s][g], sq[s][g]);
    stats[(img * DG_GROUPS + g) * 2] = (float)mean;
    stats[(img * DG_GROUPS + g) * 2 + 1] = (float)(1.0 / sqrt(m2 / na + (double)eps));
  }
}

__device__ __forceinline__ float diff_silu(float v) { return v / (1.f + expf(-v)); }

// grid (blocks over the image's p * C / V vectors, n); V adjacent channels per thread
template <int V>
__global__ void diff_gn_apply(const float* __restrict__ x, long ldx, const float* __restrict__ stats, const float* __restrict__ gamma,
                              const float* __restrict__ beta, const float* __restrict__ scale, const float* __restrict__ shift,
                              long ldmod, float* __restrict__ y, long ldy, long p, int c, int silu) {
  const unsigned cv = (unsigned)c / V, cg = (unsigned)c / DG_GROUPS;
  const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;      // < p * C / V < 2^31 (host check)
  const unsigned row = idx / cv;
  if (row >= p) return;
  const unsigned ch = (idx - row * cv) * V;
  const long img = blockIdx.y;
  const long xo = (img * p + row) * ldx + ch, yo = (img * p + row) * ldy + ch;
  float v[V];
  if (V == 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(x + xo);
    v[0] = t.x, v[1 % V] = t.y, v[2 % V] = t.z, v[3 % V] = t.w;
  } else {
    v[0] = x[xo];
  }
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const float* st = stats + (img * DG_GROUPS + (ch + k) / cg) * 2;
    float u = (v[k] - st[0]) * st[1];
    u = u * gamma[ch + k] + beta[ch + k];
    if (scale) u = u * (1.f + scale[img * ldmod + ch + k]) + shift[img * ldmod + ch + k];
    v[k] = silu ? diff_silu(u) : u;
  }
  if (V == 4) {
    f32x4 t;
    t.x = v[0], t.y = v[1 % V], t.z = v[2 % V], t.w = v[3 % V];
    *reinterpret_cast<f32x4*>(y + yo) = t;
  } else {
    y[yo] = v[0];
  }
}

__global__ void diff_silu_kernel(const float* __restrict__ x, float* __restrict__ y, long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < total) y[idx] = diff_silu(x[idx]);
}

// ---- 2 x 2 average pool ---------------------------------------------------------------------------------------------------- //
__global__ void diff_avgpool2x2(const float* __restrict__ x, float* __restrict__ y, int h, int w, int c, long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;      // (img, oy, ox, ch), ch fastest
  if (idx >= total) return;
  const int ho = h / 2, wo = w / 2;
  const int ch = (int)(idx % c);
  long t = idx / c;
  const int ox = (int)(t % wo);
  t /= wo;
  const int oy = (int)(t % ho);
  const long img = t / ho;
  const float* s = x + ((img * h + 2 * oy) * w + 2 * ox) * c + ch;
  const long down = (long)w * c;
  y[idx] = (((s[0] + s[c]) + s[down]) + s[down + c]) * 0.25f;
}

// ---- attention ------------------------------------------------------------------------------------------------------------- //
__device__ __forceinline__ f32x16 diff_mfma(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// row of accumulator register i in lane half hh (column = lane & 31)
__device__ __forceinline__ int diff_acc_row(int i, int hh) { return (i >> 2) * 8 + hh * 4 + (i & 3); }

// grid (ceil(t / 32), n * heads), one wave per block
// LSE: also write lse[(img * heads + head) * t + query] = m + log l, what the backward rebuilds the soft-max rows from
template <int CH, bool LSE>
__global__ void __launch_bounds__(64) diff_attn_kernel(const float* __restrict__ qkv, float* __restrict__ out, float* __restrict__ lse, int t,
                                                       int heads, float scale) {
  constexpr int HALF = CH / 2;      // channels of the q.k contraction a lane half owns
  constexpr int CB = CH / 32;       // 32-channel blocks of the output
  const int lane = threadIdx.x, r = lane & 31, hh = lane >> 5;
  const int q0 = blockIdx.x * 32;
  const int img = blockIdx.y / heads, head = blockIdx.y - img * heads;
  const long c = (long)heads * CH, ld = 3 * c;
  const float* base = qkv + (long)img * t * ld + (long)head * 3 * CH;      // q | k | v of this head: three adjacent runs of CH

  float qf[HALF];
  {
    const int qrow = q0 + r < t ? q0 + r : t - 1;
    const f32x4* qp = reinterpret_cast<const f32x4*>(base + (long)qrow * ld + hh * HALF);
#pragma unroll
    for (int j = 0; j < HALF / 4; ++j) {
      const f32x4 v = qp[j];
      qf[4 * j] = v.x * scale;
      qf[4 * j + 1] = v.y * scale;
      qf[4 * j + 2] = v.z * scale;
      qf[4 * j + 3] = v.w * scale;
    }
  }
  f32x16 o[CB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[cb][i] = 0.f;
  float m = -INFINITY, l = 0.f;

  for (int k0 = 0; k0 < t; k0 += 32) {
    float kf[HALF];
    {
      const int krow = k0 + r < t ? k0 + r : t - 1;
      const f32x4* kp = reinterpret_cast<const f32x4*>(base + (long)krow * ld + CH + hh * HALF);
#pragma unroll
      for (int j = 0; j < HALF / 4; ++j) {
        const f32x4 v = kp[j];
        kf[4 * j] = v.x * scale;
        kf[4 * j + 1] = v.y * scale;
        kf[4 * j + 2] = v.z * scale;
        kf[4 * j + 3] = v.w * scale;
      }
    }
    f32x16 s;
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
    for (int j = 0; j < HALF; ++j) s = diff_mfma(kf[j], qf[j], s);      // s[i] = S^T[key k0 + acc_row(i, hh)][query q0 + r]

    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (k0 + diff_acc_row(i, hh) >= t) s[i] = -INFINITY;               // the key tail
      mx = fmaxf(mx, s[i]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));                              // key k0 is valid, so mx is finite
    const float mnew = fmaxf(m, mx);
    const float alpha = expf(m - mnew);                                  // 0 on the first tile (m = -inf)
    float ps = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      s[i] = expf(s[i] - mnew);
      ps += s[i];
    }
    ps += __shfl_xor(ps, 32, 64);
    l = l * alpha + ps;
    m = mnew;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int i = 0; i < 16; ++i) o[cb][i] *= alpha;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int key = k0 + diff_acc_row(i, hh);
      const float* vp = base + (long)(key < t ? key : t - 1) * ld + 2 * CH + r;      // masked keys: p = 0 times a finite value
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) o[cb] = diff_mfma(vp[cb * 32], s[i], o[cb]);
    }
  }

  if (q0 + r < t) {
    float* op = out + ((long)img * t + q0 + r) * c + (long)head * CH;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 v;
        v.x = o[cb][4 * g] / l;
        v.y = o[cb][4 * g + 1] / l;
        v.z = o[cb][4 * g + 2] / l;
        v.w = o[cb][4 * g + 3] / l;
        *reinterpret_cast<f32x4*>(op + cb * 32 + g * 8 + hh * 4) = v;      // channels acc_row(4g .. 4g+3, hh)
      }
    if (LSE && hh == 0) lse[(long)blockIdx.y * t + q0 + r] = m + logf(l);
  }
}

// ---- sampler --------------------------------------------------------------------------------------------------------------- //
// four standard normals of counter `group` (= element index / 4) under key (seed, step)
__device__ __forceinline__ void diff_normal4(unsigned long long seed, unsigned long long step, unsigned long long group, float z[4]) {
  philox_normal4(seed, step, group, z);            // philox.h: shared with augment.hip, which must draw the same bits
}

// a thread owns the four consecutive elements of one Philox counter; element e = row * ch + channel
__global__ void diff_randn_kernel(float* __restrict__ out, long ldo, long rows, int ch, unsigned long long seed, unsigned long long step) {
  const long grp = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = rows * ch;
  if (grp * 4 >= total) return;
  float z[4];
  diff_normal4(seed, step, (unsigned long long)grp, z);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long e = grp * 4 + k;
    if (e < total) out[(e / ch) * ldo + e % ch] = z[k];
  }
}

__global__ void diff_sampler_kernel(const float* __restrict__ x0, long ldx0, const float* xt, long ldxt, const float* __restrict__ noise,
                                    long ldn, float* out, long ldo, long rows, int ch, float c1, float c2, float sigma, int drawn,
                                    unsigned long long seed, unsigned long long step) {
  const long grp = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = rows * ch;
  if (grp * 4 >= total) return;
  float z[4] = {0.f, 0.f, 0.f, 0.f};
  if (drawn) diff_normal4(seed, step, (unsigned long long)grp, z);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long e = grp * 4 + k;
    if (e >= total) break;
    const long row = e / ch;
    const int cc = (int)(e % ch);
    const float xp = x0[row * ldx0 + cc];
    const float pred = xp < -1.f ? -1.f : (xp > 1.f ? 1.f : xp);   // clamp_ that keeps a NaN prediction NaN (fminf / fmaxf would return -1)
    float v = c1 * pred + c2 * xt[row * ldxt + cc];
    if (noise) v += sigma * noise[row * ldn + cc];
    else if (drawn) v += sigma * z[k];
    out[row * ldo + cc] = v;                       // in place (out == xt) is fine: the element is read above by this thread only
  }
}

__global__ void diff_quant_kernel(const float* __restrict__ x, long ldx, unsigned char* __restrict__ out, long rows, int ch, float lo,
                                  float hi) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * ch) return;
  float v = fminf(fmaxf(x[(idx / ch) * ldx + idx % ch], lo), hi);
  v = (v - lo) / (hi - lo);
  out[idx] = (unsigned char)rintf(v * 255.f);      // rintf: round half to even, as numpy's round
}

// ============================================================================================================================== //
// Backward kernels of the training step (model/gdp_train.py).  Same contract as above: exact fp32, no atomics, fixed orders.
// ============================================================================================================================== //
// d silu(z) / dz = sigma(z) (1 + z (1 - sigma(z)))
__device__ __forceinline__ float diff_dsilu(float z) {
  const float sg = 1.f / (1.f + expf(-z));
  return sg * (1.f + z * (1.f - sg));
}

// ---- GroupNorm backward ------------------------------------------------------------------------------------------------------ //
// With xh = (x - mean) rstd, z = (xh gamma + beta)(1 + s) + sh and dz = dy silu'(z) (dz = dy without SiLU):
//   A[n][c] = sum_p dz, B[n][c] = sum_p dz xh;  dshift = A, dscale = gamma B + beta A, dgamma = sum_n (1 + s) B, dbeta = sum_n (1 + s) A,
//   g = dz (1 + s) gamma, dx = rstd (g - mean_grp(g) - xh mean_grp(g xh)), the group means being sums of (1 + s) gamma {A, B}.
//   stage 1  grid (chunks of 64 rows, n): the chunk's A and B per channel, rows dealt to dg_nsub(C) interleaved sub-sums as in the forward
//   stage 2  grid n: chunks folded in chunk order in fp64 -> A, B, dscale, dshift, and the two group means
//   stage 3  grid C / 256: samples folded in sample order in fp64 -> dgamma, dbeta
//   apply    elementwise
struct dg_chan {
  float mean, rstd, ga, be, s1, sh;
};

__device__ __forceinline__ dg_chan dg_load_chan(const float* __restrict__ stats, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                const float* __restrict__ scale, const float* __restrict__ shift, long ldmod, long img, int ch,
                                                int cg) {
  dg_chan k;
  const float* st = stats + (img * DG_GROUPS + ch / cg) * 2;
  k.mean = st[0], k.rstd = st[1], k.ga = gamma[ch], k.be = beta[ch];
  k.s1 = scale ? 1.f + scale[img * ldmod + ch] : 1.f;
  k.sh = scale ? shift[img * ldmod + ch] : 0.f;
  return k;
}

// dz and xh of one element; z is rebuilt with the forward's own operations, so it has the forward's bits
__device__ __forceinline__ float dg_dz(const dg_chan& k, float x, float dy, bool mod, int silu, float& xh) {
  xh = (x - k.mean) * k.rstd;
  if (!silu) return dy;
  float u = xh * k.ga + k.be;
  if (mod) u = u * k.s1 + k.sh;
  return dy * diff_dsilu(u);
}

// part[((img * chunks + chunk) * C + ch) * 2] = {A, B} of the chunk
template <int V>
__global__ void __launch_bounds__(DG_THREADS)
    diff_gn_bwd_stage1(const float* __restrict__ dy, long lddy, const float* __restrict__ x, long ldx, const float* __restrict__ stats,
                       const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ scale,
                       const float* __restrict__ shift, long ldmod, float* __restrict__ part, long p, int c, int silu) {
  __shared__ float sa[DG_MAXC], sb[DG_MAXC];
  const int tid = threadIdx.x;
  const long chunk = blockIdx.x, img = blockIdx.y;
  const long r0 = chunk * DG_ROWS;
  const int rows = (int)(p - r0 < DG_ROWS ? p - r0 : DG_ROWS);
  const int cg = c / DG_GROUPS, nsub = dg_nsub(c), cv = c / V;
  const float* xb = x + (img * p + r0) * ldx;
  const float* db = dy + (img * p + r0) * lddy;
  const bool mod = scale != nullptr;
  for (int idx = tid; idx < cv * nsub; idx += DG_THREADS) {
    const int sub = idx / cv, ch = (idx - sub * cv) * V;
    dg_chan k[V];
    float a[V], b[V];
#pragma unroll
    for (int j = 0; j < V; ++j) k[j] = dg_load_chan(stats, gamma, beta, scale, shift, ldmod, img, ch + j, cg), a[j] = 0.f, b[j] = 0.f;
#pragma unroll 2
    for (int r = sub; r < rows; r += nsub) {
      dg_vec<V> tx, td;
      tx.load(xb + (long)r * ldx + ch);
      td.load(db + (long)r * lddy + ch);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float xh;
        const float dz = dg_dz(k[j], tx.v[j], td.v[j], mod, silu, xh);
        a[j] += dz;
        b[j] += dz * xh;
      }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) sa[sub * c + ch + j] = a[j], sb[sub * c + ch + j] = b[j];
  }
  __syncthreads();
  float* o = part + (img * gridDim.x + chunk) * c * 2;
  for (int ch = tid; ch < c; ch += DG_THREADS) {
    float a = 0.f, b = 0.f;
    for (int sub = 0; sub < nsub; ++sub) a += sa[sub * c + ch], b += sb[sub * c + ch];
    o[ch * 2] = a;
    o[ch * 2 + 1] = b;
  }
}

// ab[(img * C + ch) * 2] = (1 + s) {A, B};  gmeans[(img * 32 + g) * 2] = {mean_grp(g), mean_grp(g xh)};  dscale / dshift rows if modulated
__global__ void __launch_bounds__(DG_THREADS)
    diff_gn_bwd_stage2(const float* __restrict__ part, const float* __restrict__ gamma, const float* __restrict__ beta,
                       const float* __restrict__ scale, long ldmod, float* __restrict__ ab, float* __restrict__ gmeans,
                       float* __restrict__ dscale, float* __restrict__ dshift, long lddmod, long p, int c, long chunks) {
  __shared__ double ga[DG_MAXC], gb[DG_MAXC];
  const int tid = threadIdx.x;
  const long img = blockIdx.x;
  const int cg = c / DG_GROUPS;
  for (int ch = tid; ch < c; ch += DG_THREADS) {
    double a = 0.0, b = 0.0;
    const float* q = part + (img * chunks * c + ch) * 2;
    for (long k = 0; k < chunks; ++k) a += (double)q[k * c * 2], b += (double)q[k * c * 2 + 1];
    const double g = (double)gamma[ch];
    if (dscale) {
      dshift[img * lddmod + ch] = (float)a;
      dscale[img * lddmod + ch] = (float)(g * b + (double)beta[ch] * a);
    }
    const double s1 = scale ? 1.0 + (double)scale[img * ldmod + ch] : 1.0;
    ab[(img * c + ch) * 2] = (float)(s1 * a);
    ab[(img * c + ch) * 2 + 1] = (float)(s1 * b);
    ga[ch] = s1 * g * a;
    gb[ch] = s1 * g * b;
  }
  __syncthreads();
  if (tid < DG_GROUPS) {
    double a = 0.0, b = 0.0;
    for (int j = 0; j < cg; ++j) a += ga[tid * cg + j], b += gb[tid * cg + j];
    const double cnt = (double)p * cg;
    gmeans[(img * DG_GROUPS + tid) * 2] = (float)(a / cnt);
    gmeans[(img * DG_GROUPS + tid) * 2 + 1] = (float)(b / cnt);
  }
}

__global__ void diff_gn_bwd_stage3(const float* __restrict__ ab, float* __restrict__ dgamma, float* __restrict__ dbeta, long n, int c) {
  const int ch = blockIdx.x * blockDim.x + threadIdx.x;
  if (ch >= c) return;
  double a = 0.0, b = 0.0;
  for (long img = 0; img < n; ++img) a += (double)ab[(img * c + ch) * 2], b += (double)ab[(img * c + ch) * 2 + 1];
  dbeta[ch] = (float)a;
  dgamma[ch] = (float)b;
}

template <int V>
__global__ void diff_gn_bwd_apply(const float* __restrict__ dy, long lddy, const float* __restrict__ x, long ldx, const float* __restrict__ stats,
                                  const float* __restrict__ gmeans, const float* __restrict__ gamma, const float* __restrict__ beta,
                                  const float* __restrict__ scale, const float* __restrict__ shift, long ldmod, float* __restrict__ dx,
                                  long lddx, long p, int c, int silu) {
  const unsigned cv = (unsigned)c / V, cg = (unsigned)c / DG_GROUPS;
  const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;      // < p * C / V < 2^31 (host check)
  const unsigned row = idx / cv;
  if (row >= p) return;
  const unsigned ch = (idx - row * cv) * V;
  const long img = blockIdx.y;
  dg_vec<V> tx, td;
  tx.load(x + (img * p + row) * ldx + ch);
  td.load(dy + (img * p + row) * lddy + ch);
  float v[V];
  const bool mod = scale != nullptr;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const dg_chan k = dg_load_chan(stats, gamma, beta, scale, shift, ldmod, img, ch + j, cg);
    const float* gm = gmeans + (img * DG_GROUPS + (ch + j) / cg) * 2;
    float xh;
    const float dz = dg_dz(k, tx.v[j], td.v[j], mod, silu, xh);
    const float g = dz * k.s1 * k.ga;
    v[j] = k.rstd * ((g - gm[0]) - xh * gm[1]);
  }
  float* o = dx + (img * p + row) * lddx + ch;
  if (V == 4) {
    f32x4 t;
    t.x = v[0], t.y = v[1 % V], t.z = v[2 % V], t.w = v[3 % V];
    *reinterpret_cast<f32x4*>(o) = t;
  } else {
    o[0] = v[0];
  }
}

__global__ void diff_silu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dx, long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < total) dx[idx] = dy[idx] * diff_dsilu(x[idx]);
}

// dx [n][h][w][c] = 0.25 dy [n][h/2][w/2][c] over each 2 x 2 window
__global__ void diff_avgpool2x2_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int h, int w, int c, long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;      // (img, y, x, ch), ch fastest
  if (idx >= total) return;
  const int ch = (int)(idx % c);
  long t = idx / c;
  const int xx = (int)(t % w);
  t /= w;
  const int yy = (int)(t % h);
  const long img = t / h;
  dx[idx] = 0.25f * dy[((img * (h / 2) + yy / 2) * (w / 2) + xx / 2) * c + ch];
}

// ---- attention backward ------------------------------------------------------------------------------------------------------ //
// Both kernels keep the forward's register layout (one wave, 32 x 32 tiles, the owned token is the lane's column), rebuild the soft-max
// tile from lse and never hold a T x T tensor.  With P = exp(S - lse), dP = dO V^T, delta = rowsum(dO o O), dS = P o (dP - delta):
//   dQ = scale^2 dS K_raw,  dK = scale^2 dS^T Q_raw,  dV = P^T dO        (q and k were each scaled by ch^-1/4)
template <int HALF>
__device__ __forceinline__ void diff_load_half(const float* p, float scale, float (&f)[HALF]) {
  const f32x4* q = reinterpret_cast<const f32x4*>(p);
#pragma unroll
  for (int j = 0; j < HALF / 4; ++j) {
    const f32x4 v = q[j];
    f[4 * j] = v.x * scale;
    f[4 * j + 1] = v.y * scale;
    f[4 * j + 2] = v.z * scale;
    f[4 * j + 3] = v.w * scale;
  }
}

// store the accumulator tiles acc^T[c][token = lane column] times `mul` into row `dst` (CH channels)
template <int CB>
__device__ __forceinline__ void diff_store_tiles(const f32x16 (&acc)[CB], float mul, float* dst, int hh) {
#pragma unroll
  for (int cb = 0; cb < CB; ++cb)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f32x4 v;
      v.x = acc[cb][4 * g] * mul;
      v.y = acc[cb][4 * g + 1] * mul;
      v.z = acc[cb][4 * g + 2] * mul;
      v.w = acc[cb][4 * g + 3] * mul;
      *reinterpret_cast<f32x4*>(dst + cb * 32 + g * 8 + hh * 4) = v;
    }
}

// grid (ceil(t / 32), n * heads), one wave: dq rows of 32 queries, and delta[(img * heads + head) * t + query]
template <int CH>
__global__ void __launch_bounds__(64)
    diff_attn_bwd_dq(const float* __restrict__ qkv, const float* __restrict__ out, const float* __restrict__ dout, const float* __restrict__ lse,
                     float* __restrict__ delta, float* __restrict__ dqkv, int t, int heads, float scale) {
  constexpr int HALF = CH / 2, CB = CH / 32;
  const int lane = threadIdx.x, r = lane & 31, hh = lane >> 5;
  const int q0 = blockIdx.x * 32;
  const int img = blockIdx.y / heads, head = blockIdx.y - img * heads;
  const long c = (long)heads * CH, ld = 3 * c;
  const float* base = qkv + (long)img * t * ld + (long)head * 3 * CH;
  const int qrow = q0 + r < t ? q0 + r : t - 1;
  float qf[HALF], dof[HALF];
  diff_load_half<HALF>(base + (long)qrow * ld + hh * HALF, scale, qf);
  diff_load_half<HALF>(dout + ((long)img * t + qrow) * c + (long)head * CH + hh * HALF, 1.f, dof);
  float dl = 0.f;
  {
    float of[HALF];
    diff_load_half<HALF>(out + ((long)img * t + qrow) * c + (long)head * CH + hh * HALF, 1.f, of);
#pragma unroll
    for (int j = 0; j < HALF; ++j) dl += dof[j] * of[j];
    dl += __shfl_xor(dl, 32, 64);
  }
  const float ls = lse[(long)blockIdx.y * t + qrow];
  if (hh == 0 && q0 + r < t) delta[(long)blockIdx.y * t + q0 + r] = dl;
  f32x16 dq[CB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb)
#pragma unroll
    for (int i = 0; i < 16; ++i) dq[cb][i] = 0.f;

  for (int k0 = 0; k0 < t; k0 += 32) {
    const int krow = k0 + r < t ? k0 + r : t - 1;
    f32x16 s, dp;
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] = 0.f, dp[i] = 0.f;
    {
      float kf[HALF];
      diff_load_half<HALF>(base + (long)krow * ld + CH + hh * HALF, scale, kf);
#pragma unroll
      for (int j = 0; j < HALF; ++j) s = diff_mfma(kf[j], qf[j], s);        // S^T[key][query]
    }
    {
      float vf[HALF];
      diff_load_half<HALF>(base + (long)krow * ld + 2 * CH + hh * HALF, 1.f, vf);
#pragma unroll
      for (int j = 0; j < HALF; ++j) dp = diff_mfma(vf[j], dof[j], dp);     // dP^T[key][query]
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float pr = k0 + diff_acc_row(i, hh) < t ? expf(s[i] - ls) : 0.f;
      s[i] = pr * (dp[i] - dl);                                            // dS^T
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int key = k0 + diff_acc_row(i, hh);
      const float* kp = base + (long)(key < t ? key : t - 1) * ld + CH + r;
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) dq[cb] = diff_mfma(kp[cb * 32], s[i], dq[cb]);      // dQ^T[c][query] += K^T dS^T
    }
  }
  if (q0 + r < t) diff_store_tiles<CB>(dq, scale * scale, dqkv + ((long)img * t + q0 + r) * ld + (long)head * 3 * CH, hh);
}

// grid (ceil(t / 32), n * heads), one wave: dk and dv rows of 32 keys
template <int CH>
__global__ void __launch_bounds__(64)
    diff_attn_bwd_dkv(const float* __restrict__ qkv, const float* __restrict__ dout, const float* __restrict__ lse,
                      const float* __restrict__ delta, float* __restrict__ dqkv, int t, int heads, float scale) {
  constexpr int HALF = CH / 2, CB = CH / 32;
  const int lane = threadIdx.x, r = lane & 31, hh = lane >> 5;
  const int k0 = blockIdx.x * 32;
  const int img = blockIdx.y / heads, head = blockIdx.y - img * heads;
  const long c = (long)heads * CH, ld = 3 * c;
  const float* base = qkv + (long)img * t * ld + (long)head * 3 * CH;
  const float* dob = dout + (long)img * t * c + (long)head * CH;
  const float* lsb = lse + (long)blockIdx.y * t;
  const float* dlb = delta + (long)blockIdx.y * t;
  const int krow = k0 + r < t ? k0 + r : t - 1;
  float kf[HALF], vf[HALF];
  diff_load_half<HALF>(base + (long)krow * ld + CH + hh * HALF, scale, kf);
  diff_load_half<HALF>(base + (long)krow * ld + 2 * CH + hh * HALF, 1.f, vf);
  f32x16 dk[CB], dv[CB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb)
#pragma unroll
    for (int i = 0; i < 16; ++i) dk[cb][i] = 0.f, dv[cb][i] = 0.f;

  for (int q0 = 0; q0 < t; q0 += 32) {
    const int qrow = q0 + r < t ? q0 + r : t - 1;
    f32x16 s, dp;
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] = 0.f, dp[i] = 0.f;
    {
      float qf[HALF];
      diff_load_half<HALF>(base + (long)qrow * ld + hh * HALF, scale, qf);
#pragma unroll
      for (int j = 0; j < HALF; ++j) s = diff_mfma(qf[j], kf[j], s);        // S[query][key]
    }
    {
      float dof[HALF];
      diff_load_half<HALF>(dob + (long)qrow * c + hh * HALF, 1.f, dof);
#pragma unroll
      for (int j = 0; j < HALF; ++j) dp = diff_mfma(dof[j], vf[j], dp);     // dP[query][key]
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int q = q0 + diff_acc_row(i, hh);
      const int qc = q < t ? q : t - 1;
      const float pr = q < t ? expf(s[i] - lsb[qc]) : 0.f;                  // queries past t contribute nothing
      s[i] = pr;
      dp[i] = pr * (dp[i] - dlb[qc]);                                       // dS
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int q = q0 + diff_acc_row(i, hh);
      const long qc = q < t ? q : t - 1;
      const float* dop = dob + qc * c + r;
      const float* qp = base + qc * ld + r;
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        dv[cb] = diff_mfma(dop[cb * 32], s[i], dv[cb]);                     // dV^T[c][key] += dO^T P
        dk[cb] = diff_mfma(qp[cb * 32], dp[i], dk[cb]);                     // dK^T[c][key] += Q^T dS
      }
    }
  }
  if (k0 + r < t) {
    float* dst = dqkv + ((long)img * t + k0 + r) * ld + (long)head * 3 * CH;
    diff_store_tiles<CB>(dk, scale * scale, dst + CH, hh);
    diff_store_tiles<CB>(dv, 1.f, dst + 2 * CH, hh);
  }
}

// ---- forward diffusion --------------------------------------------------------------------------------------------------------- //
// out = sqrt_ac[t_b] x0 + sqrt_1mac[t_b] eps, b = row / rows_per_sample; eps supplied or srhip_diff_randn(seed, step)'s draws
__global__ void diff_q_sample_kernel(const float* __restrict__ x0, long ldx0, const float* __restrict__ noise, long ldn, float* __restrict__ out,
                                     long ldo, const long long* __restrict__ tt, const float* __restrict__ sqrt_ac,
                                     const float* __restrict__ sqrt_1mac, int steps, long rows, long rows_per_sample, int ch,
                                     unsigned long long seed, unsigned long long step) {
  const long grp = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = rows * ch;
  if (grp * 4 >= total) return;
  float z[4] = {0.f, 0.f, 0.f, 0.f};
  if (!noise) diff_normal4(seed, step, (unsigned long long)grp, z);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long e = grp * 4 + k;
    if (e >= total) break;
    const long row = e / ch;
    const int cc = (int)(e % ch);
    long long ti = tt[row / rows_per_sample];
    ti = ti < 0 ? 0 : (ti >= steps ? steps - 1 : ti);                      // a timestep outside the schedule must not read past it
    const float eps = noise ? noise[row * ldn + cc] : z[k];
    out[row * ldo + cc] = sqrt_ac[ti] * x0[row * ldx0 + cc] + sqrt_1mac[ti] * eps;
  }
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace srhip

using namespace srhip;

extern "C" {

size_t srhip_diff_gn_workspace(long n, long p) {
  if (n <= 0 || p <= 0) return 0;
  const long chunks = (p + DG_ROWS - 1) / DG_ROWS;
  return (size_t)(n * chunks + n) * DG_GROUPS * 2 * sizeof(float);
}

int srhip_diff_gn_fwd(const float* x, long ldx, const float* gamma, const float* beta, const float* scale, const float* shift, long ldmod,
                      float* y, long ldy, void* workspace, size_t workspace_bytes, long n, long p, int c, float eps, int silu,
                      void* stream) {
  SRHIP_REQUIRE(x && gamma && beta && y && workspace, "diff_gn_fwd: null tensor");
  SRHIP_REQUIRE(n > 0 && n <= 65535 && p > 0 && c > 0 && c <= DG_MAXC && c % DG_GROUPS == 0,
                "diff_gn_fwd: needs 0 < n <= 65535, p > 0, C %% 32 == 0 and C <= %d (got n %ld, p %ld, C %d)", DG_MAXC, n, p, c);
  SRHIP_REQUIRE(ldx >= c && ldy >= c, "diff_gn_fwd: row strides must be >= C");
  SRHIP_REQUIRE((scale == nullptr) == (shift == nullptr) && (!scale || ldmod >= c), "diff_gn_fwd: scale and shift come together, stride >= C");
  SRHIP_REQUIRE(n * p * (long)c < (1L << 38), "diff_gn_fwd: tensor too large");
  if (workspace_bytes < srhip_diff_gn_workspace(n, p)) {
    set_error("diff_gn_fwd: workspace of %zu bytes, %zu needed", workspace_bytes, srhip_diff_gn_workspace(n, p));
    return SRHIP_ERR_WORKSPACE;
  }
  const long chunks = (p + DG_ROWS - 1) / DG_ROWS;
  SRHIP_REQUIRE(chunks <= 0x7fffffffL && p * c < (1L << 31), "diff_gn_fwd: image too large (p * C must stay below 2^31)");
  float* part = static_cast<float*>(workspace);
  float* stats = part + n * chunks * DG_GROUPS * 2;
  hipStream_t st = as_stream(stream);
  // float4 loads where every row start is 16-byte aligned; the result is the same bit for bit either way
  const bool vec_in = ldx % 4 == 0 && aligned16(x);
  const bool vec_io = vec_in && ldy % 4 == 0 && aligned16(y);
  if (vec_in)
    hipLaunchKernelGGL(diff_gn_stage1<4>, dim3((unsigned)chunks, (unsigned)n), dim3(DG_THREADS), 0, st, x, ldx, part, p, c);
  else
    hipLaunchKernelGGL(diff_gn_stage1<1>, dim3((unsigned)chunks, (unsigned)n), dim3(DG_THREADS), 0, st, x, ldx, part, p, c);
  hipLaunchKernelGGL(diff_gn_stage2, dim3((unsigned)n), dim3(DG_GROUPS * DG_SEGS), 0, st, part, stats, p, c, chunks, eps);
  if (vec_io)
    hipLaunchKernelGGL(diff_gn_apply<4>, dim3((unsigned)cdiv(p * c / 4, 256), (unsigned)n), dim3(256), 0, st, x, ldx, stats, gamma, beta,
                       scale, shift, ldmod, y, ldy, p, c, silu);
  else
    hipLaunchKernelGGL(diff_gn_apply<1>, dim3((unsigned)cdiv(p * c, 256), (unsigned)n), dim3(256), 0, st, x, ldx, stats, gamma, beta, scale,
                       shift, ldmod, y, ldy, p, c, silu);
  return check_launch("diff_gn_fwd");
}

int srhip_diff_silu_fwd(const float* x, float* y, long count, void* stream) {
  SRHIP_REQUIRE(x && y && count > 0 && count < (1L << 38), "diff_silu_fwd: bad argument");
  hipLaunchKernelGGL(diff_silu_kernel, dim3((unsigned)cdiv(count, 256)), dim3(256), 0, as_stream(stream), x, y, count);
  return check_launch("diff_silu_fwd");
}

int srhip_diff_avgpool2x2_fwd(const float* x, float* y, int n, int h, int w, int c, void* stream) {
  SRHIP_REQUIRE(x && y && n > 0 && h > 0 && w > 0 && c > 0, "diff_avgpool2x2_fwd: bad argument");
  SRHIP_REQUIRE(h % 2 == 0 && w % 2 == 0, "diff_avgpool2x2_fwd: H and W must be even (got %d x %d)", h, w);
  const long total = (long)n * (h / 2) * (w / 2) * c;
  SRHIP_REQUIRE(total < (1L << 38), "diff_avgpool2x2_fwd: tensor too large");
  hipLaunchKernelGGL(diff_avgpool2x2, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, as_stream(stream), x, y, h, w, c, total);
  return check_launch("diff_avgpool2x2_fwd");
}

static int attn_fwd(const char* what, const float* qkv, float* out, float* lse, int n, int t, int heads, int ch, void* stream) {
  SRHIP_REQUIRE(qkv && out, "%s: null tensor", what);
  SRHIP_REQUIRE(ch == 32 || ch == 64, "%s: head width must be 32 or 64 (got %d)", what, ch);
  SRHIP_REQUIRE(n > 0 && t > 0 && heads > 0 && (long)n * heads <= 65535, "%s: needs n, t, heads > 0 and n * heads <= 65535", what);
  SRHIP_REQUIRE(aligned16(qkv) && aligned16(out), "%s: tensors must be 16-byte aligned", what);
  const float scale = 1.f / sqrtf(sqrtf((float)ch));
  const dim3 grid((unsigned)cdiv(t, 32), (unsigned)(n * heads));
  hipStream_t st = as_stream(stream);
  if (ch == 32 && lse)
    hipLaunchKernelGGL((diff_attn_kernel<32, true>), grid, dim3(64), 0, st, qkv, out, lse, t, heads, scale);
  else if (ch == 32)
    hipLaunchKernelGGL((diff_attn_kernel<32, false>), grid, dim3(64), 0, st, qkv, out, lse, t, heads, scale);
  else if (lse)
    hipLaunchKernelGGL((diff_attn_kernel<64, true>), grid, dim3(64), 0, st, qkv, out, lse, t, heads, scale);
  else
    hipLaunchKernelGGL((diff_attn_kernel<64, false>), grid, dim3(64), 0, st, qkv, out, lse, t, heads, scale);
  return check_launch(what);
}

int srhip_diff_attn_fwd(const float* qkv, float* out, int n, int t, int heads, int ch, void* stream) {
  return attn_fwd("diff_attn_fwd", qkv, out, nullptr, n, t, heads, ch, stream);
}

int srhip_diff_attn_fwd_lse(const float* qkv, float* out, float* lse, int n, int t, int heads, int ch, void* stream) {
  SRHIP_REQUIRE(lse, "diff_attn_fwd_lse: null tensor");
  return attn_fwd("diff_attn_fwd_lse", qkv, out, lse, n, t, heads, ch, stream);
}

int srhip_diff_randn(float* out, long ldo, long rows, int ch, unsigned long long seed, unsigned long long step, void* stream) {
  SRHIP_REQUIRE(out && rows > 0 && ch > 0 && ldo >= ch && rows * ch < (1L << 38), "diff_randn: bad argument");
  const long groups = (rows * ch + 3) / 4;
  hipLaunchKernelGGL(diff_randn_kernel, dim3((unsigned)cdiv(groups, 256)), dim3(256), 0, as_stream(stream), out, ldo, rows, ch, seed, step);
  return check_launch("diff_randn");
}

int srhip_diff_sampler_step(const float* x0, long ldx0, const float* xt, long ldxt, const float* noise, long ldn, float* out, long ldo,
                            long rows, int ch, float c1, float c2, float logvar, int t_nonzero, unsigned long long seed,
                            unsigned long long step, void* stream) {
  SRHIP_REQUIRE(x0 && xt && out, "diff_sampler_step: null tensor");
  SRHIP_REQUIRE(rows > 0 && ch > 0 && rows * ch < (1L << 38), "diff_sampler_step: bad size");
  SRHIP_REQUIRE(ldx0 >= ch && ldxt >= ch && ldo >= ch && (!noise || ldn >= ch), "diff_sampler_step: row strides must be >= channels");
  const float sigma = expf(0.5f * logvar);
  const long groups = (rows * ch + 3) / 4;
  hipLaunchKernelGGL(diff_sampler_kernel, dim3((unsigned)cdiv(groups, 256)), dim3(256), 0, as_stream(stream), x0, ldx0, xt, ldxt,
                     t_nonzero ? noise : nullptr, ldn, out, ldo, rows, ch, c1, c2, sigma, (t_nonzero && !noise) ? 1 : 0, seed, step);
  return check_launch("diff_sampler_step");
}

int srhip_diff_quant_u8(const float* x, long ldx, unsigned char* out, long rows, int ch, float lo, float hi, void* stream) {
  SRHIP_REQUIRE(x && out && rows > 0 && ch > 0 && ldx >= ch && rows * ch < (1L << 38), "diff_quant_u8: bad argument");
  SRHIP_REQUIRE(hi > lo, "diff_quant_u8: needs lo < hi");
  hipLaunchKernelGGL(diff_quant_kernel, dim3((unsigned)cdiv(rows * ch, 256)), dim3(256), 0, as_stream(stream), x, ldx, out, rows, ch, lo, hi);
  return check_launch("diff_quant_u8");
}

// ---- backward entry points --------------------------------------------------------------------------------------------------- //
size_t srhip_diff_gn_stats_offset(long n, long p) {
  if (n <= 0 || p <= 0) return 0;
  return (size_t)(n * ((p + DG_ROWS - 1) / DG_ROWS)) * DG_GROUPS * 2 * sizeof(float);
}

size_t srhip_diff_gn_bwd_workspace(long n, long p, int c) {
  if (n <= 0 || p <= 0 || c <= 0) return 0;
  const long chunks = (p + DG_ROWS - 1) / DG_ROWS;
  return (size_t)(n * chunks * c * 2 + n * c * 2 + n * DG_GROUPS * 2) * sizeof(float);
}

int srhip_diff_gn_bwd(const float* dy, long lddy, const float* x, long ldx, const float* stats, const float* gamma, const float* beta,
                      const float* scale, const float* shift, long ldmod, float* dx, long lddx, float* dgamma, float* dbeta, float* dscale,
                      float* dshift, long lddmod, void* workspace, size_t workspace_bytes, long n, long p, int c, int silu, void* stream) {
  SRHIP_REQUIRE(dy && x && stats && gamma && beta && dx && dgamma && dbeta && workspace, "diff_gn_bwd: null tensor");
  SRHIP_REQUIRE(n > 0 && n <= 65535 && p > 0 && c > 0 && c <= DG_MAXC && c % DG_GROUPS == 0,
                "diff_gn_bwd: needs 0 < n <= 65535, p > 0, C %% 32 == 0 and C <= %d (got n %ld, p %ld, C %d)", DG_MAXC, n, p, c);
  SRHIP_REQUIRE(ldx >= c && lddy >= c && lddx >= c, "diff_gn_bwd: row strides must be >= C");
  SRHIP_REQUIRE((scale == nullptr) == (shift == nullptr) && (!scale || ldmod >= c), "diff_gn_bwd: scale and shift come together, stride >= C");
  SRHIP_REQUIRE((dscale == nullptr) == (scale == nullptr) && (dshift == nullptr) == (scale == nullptr) && (!dscale || lddmod >= c),
                "diff_gn_bwd: dscale and dshift come with scale and shift, stride >= C");
  SRHIP_REQUIRE(n * p * (long)c < (1L << 38), "diff_gn_bwd: tensor too large");
  if (workspace_bytes < srhip_diff_gn_bwd_workspace(n, p, c)) {
    set_error("diff_gn_bwd: workspace of %zu bytes, %zu needed", workspace_bytes, srhip_diff_gn_bwd_workspace(n, p, c));
    return SRHIP_ERR_WORKSPACE;
  }
  const long chunks = (p + DG_ROWS - 1) / DG_ROWS;
  SRHIP_REQUIRE(chunks <= 0x7fffffffL && p * c < (1L << 31), "diff_gn_bwd: image too large (p * C must stay below 2^31)");
  float* part = static_cast<float*>(workspace);
  float* ab = part + n * chunks * c * 2;
  float* gmeans = ab + n * c * 2;
  hipStream_t st = as_stream(stream);
  const dim3 g1((unsigned)chunks, (unsigned)n);
  // float4 loads where every row start is 16-byte aligned; the result is the same bit for bit either way
  const bool vec_in = ldx % 4 == 0 && lddy % 4 == 0 && aligned16(x) && aligned16(dy);
  const bool vec_io = vec_in && lddx % 4 == 0 && aligned16(dx);
  if (vec_in)
    hipLaunchKernelGGL(diff_gn_bwd_stage1<4>, g1, dim3(DG_THREADS), 0, st, dy, lddy, x, ldx, stats, gamma, beta, scale, shift, ldmod, part, p,
                       c, silu);
  else
    hipLaunchKernelGGL(diff_gn_bwd_stage1<1>, g1, dim3(DG_THREADS), 0, st, dy, lddy, x, ldx, stats, gamma, beta, scale, shift, ldmod, part, p,
                       c, silu);
  hipLaunchKernelGGL(diff_gn_bwd_stage2, dim3((unsigned)n), dim3(DG_THREADS), 0, st, part, gamma, beta, scale, ldmod, ab, gmeans, dscale, dshift,
                     lddmod, p, c, chunks);
  hipLaunchKernelGGL(diff_gn_bwd_stage3, dim3((unsigned)cdiv(c, 256)), dim3(256), 0, st, ab, dgamma, dbeta, n, c);
  if (vec_io)
    hipLaunchKernelGGL(diff_gn_bwd_apply<4>, dim3((unsigned)cdiv(p * c / 4, 256), (unsigned)n), dim3(256), 0, st, dy, lddy, x, ldx, stats, gmeans,
                       gamma, beta, scale, shift, ldmod, dx, lddx, p, c, silu);
  else
    hipLaunchKernelGGL(diff_gn_bwd_apply<1>, dim3((unsigned)cdiv(p * c, 256), (unsigned)n), dim3(256), 0, st, dy, lddy, x, ldx, stats, gmeans,
                       gamma, beta, scale, shift, ldmod, dx, lddx, p, c, silu);
  return check_launch("diff_gn_bwd");
}

int srhip_diff_silu_bwd(const float* dy, const float* x, float* dx, long count, void* stream) {
  SRHIP_REQUIRE(dy && x && dx && count > 0 && count < (1L << 38), "diff_silu_bwd: bad argument");
  hipLaunchKernelGGL(diff_silu_bwd_kernel, dim3((unsigned)cdiv(count, 256)), dim3(256), 0, as_stream(stream), dy, x, dx, count);
  return check_launch("diff_silu_bwd");
}

int srhip_diff_avgpool2x2_bwd(const float* dy, float* dx, int n, int h, int w, int c, void* stream) {
  SRHIP_REQUIRE(dy && dx && n > 0 && h > 0 && w > 0 && c > 0, "diff_avgpool2x2_bwd: bad argument");
  SRHIP_REQUIRE(h % 2 == 0 && w % 2 == 0, "diff_avgpool2x2_bwd: H and W must be even (got %d x %d)", h, w);
  const long total = (long)n * h * w * c;
  SRHIP_REQUIRE(total < (1L << 38), "diff_avgpool2x2_bwd: tensor too large");
  hipLaunchKernelGGL(diff_avgpool2x2_bwd_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, as_stream(stream), dy, dx, h, w, c, total);
  return check_launch("diff_avgpool2x2_bwd");
}

size_t srhip_diff_attn_bwd_workspace(int n, int t, int heads) {
  if (n <= 0 || t <= 0 || heads <= 0) return 0;
  return (size_t)n * heads * t * sizeof(float);
}

int srhip_diff_attn_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, void* workspace,
                        size_t workspace_bytes, int n, int t, int heads, int ch, void* stream) {
  SRHIP_REQUIRE(qkv && out && dout && lse && dqkv && workspace, "diff_attn_bwd: null tensor");
  SRHIP_REQUIRE(ch == 32 || ch == 64, "diff_attn_bwd: head width must be 32 or 64 (got %d)", ch);
  SRHIP_REQUIRE(n > 0 && t > 0 && heads > 0 && (long)n * heads <= 65535, "diff_attn_bwd: needs n, t, heads > 0 and n * heads <= 65535");
  SRHIP_REQUIRE(aligned16(qkv) && aligned16(out) && aligned16(dout) && aligned16(dqkv), "diff_attn_bwd: tensors must be 16-byte aligned");
  if (workspace_bytes < srhip_diff_attn_bwd_workspace(n, t, heads)) {
    set_error("diff_attn_bwd: workspace of %zu bytes, %zu needed", workspace_bytes, srhip_diff_attn_bwd_workspace(n, t, heads));
    return SRHIP_ERR_WORKSPACE;
  }
  float* delta = static_cast<float*>(workspace);
  const float scale = 1.f / sqrtf(sqrtf((float)ch));
  const dim3 grid((unsigned)cdiv(t, 32), (unsigned)(n * heads));
  hipStream_t st = as_stream(stream);
  if (ch == 32) {
    hipLaunchKernelGGL(diff_attn_bwd_dq<32>, grid, dim3(64), 0, st, qkv, out, dout, lse, delta, dqkv, t, heads, scale);
    hipLaunchKernelGGL(diff_attn_bwd_dkv<32>, grid, dim3(64), 0, st, qkv, dout, lse, delta, dqkv, t, heads, scale);
  } else {
    hipLaunchKernelGGL(diff_attn_bwd_dq<64>, grid, dim3(64), 0, st, qkv, out, dout, lse, delta, dqkv, t, heads, scale);
    hipLaunchKernelGGL(diff_attn_bwd_dkv<64>, grid, dim3(64), 0, st, qkv, dout, lse, delta, dqkv, t, heads, scale);
  }
  return check_launch("diff_attn_bwd");
}

int srhip_diff_q_sample(const float* x0, long ldx0, const float* noise, long ldn, float* out, long ldo, const long long* t,
                        const float* sqrt_ac, const float* sqrt_1mac, int steps, long n, long rows_per_sample, int ch,
                        unsigned long long seed, unsigned long long step, void* stream) {
  SRHIP_REQUIRE(x0 && out && t && sqrt_ac && sqrt_1mac, "diff_q_sample: null tensor");
  SRHIP_REQUIRE(n > 0 && rows_per_sample > 0 && ch > 0 && steps > 0 && n * rows_per_sample * ch < (1L << 38), "diff_q_sample: bad size");
  SRHIP_REQUIRE(ldx0 >= ch && ldo >= ch && (!noise || ldn >= ch), "diff_q_sample: row strides must be >= channels");
  const long rows = n * rows_per_sample;
  const long groups = (rows * ch + 3) / 4;
  hipLaunchKernelGGL(diff_q_sample_kernel, dim3((unsigned)cdiv(groups, 256)), dim3(256), 0, as_stream(stream), x0, ldx0, noise, ldn, out, ldo, t,
                     sqrt_ac, sqrt_1mac, steps, rows, rows_per_sample, ch, seed, step);
  return check_launch("diff_q_sample");
}

}  // extern "C"
