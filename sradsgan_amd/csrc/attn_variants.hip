// The local-attention tail of RAB / ResGroup for every ablation of the reference (sradsgan.py:101-151, 215-324): the order of
// the two gates (la_mode) and the pools each gate sees (pool_mode).  attn_tail.hip is the one point 'CA-SA' / 'Avg|Max' / addconv
// with its own training and inference fusions; this file states the forward of all the others (and of that point) in the same
// arithmetic, so that no variant materialises the gated activations, and their backward (second half of the file).
//
//     Chan_P(a):  avg_c = mean_p a, mx_c = max_p a (first pixel attaining it),  s = sigmoid(sum_{q in P} fc2 relu(fc1 stat_q))
//     Spat_P(a):  pa_p = mean_c a, pm_p = max_c a (first channel attaining it), m = sigmoid(conv7x7(present maps, Avg first))
//
//     order 0  CA-SA   s = Chan(u),   m = Spat(s u),  z = m (s u)
//     order 1  SA-CA   m = Spat(u),   s = Chan(m u),  z = s (m u)
//     order 2  CA      s = Chan(u),                   z = s u
//     order 3  SA      m = Spat(u),                   z = m u
//     order 4  CA|SA   s = Chan(u),   m = Spat(u),    z = cat[s u, m u]
//
// u is NHWC [n][hw][64]: a pixel is 256 contiguous bytes.  The pixel pooling keeps a wave on whole pixels (64 channels, one per
// lane) and reduces over pixels in per-lane accumulators, then across the 4 waves of a block and across blocks through segment
// partials in a fixed order; the channel pooling gives a pixel to 16 lanes (float4 each) and reduces across them.  No atomics:
// the same input gives the same bits.  Exact fp32, whatever the conv arithmetic.  Only what the pool set asks for is reduced.
// The closing kernels serve the variants without a 1x1 conv of their own shape: out = gates * u + skip, and the gated cat that is
// the x operand of CA|SA's 128 -> 64 conv.  The conv-closed sequential modes need neither: the 1x1 conv takes m and s as its row
// and channel scales.
#include <math.h>

#include "common.h"

namespace srhip {

constexpr int VC = 64;           // channels
constexpr int VSEG = 32;         // pixel-pooling segments per image
constexpr int POOL_AVG = 1, POOL_MAX = 2;

template <int N>
__device__ __forceinline__ float var_ror16(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x120 + N, 0xF, 0xF, false));
}
// sum over the 16 lanes of a row, every lane gets the total
__device__ inline float var_sum16(float v) {
  v += var_ror16<8>(v);
  v += var_ror16<4>(v);
  v += var_ror16<2>(v);
  v += var_ror16<1>(v);
  return v;
}

// ---- pixel pooling: per (image, segment) partial sum / max / first arg-max of a = gate_p * u over the segment's pixels ------- //
// block = 4 waves; wave rl visits pixels p0 + rl, p0 + rl + 4, ...; lane = channel.  gate: [n][hw] or null.
template <bool GATED>
__global__ __launch_bounds__(256) void var_pool_pix_kernel(const float* __restrict__ u, const float* __restrict__ gate,
                                                           float* __restrict__ psum, float* __restrict__ pmax,
                                                           int* __restrict__ parg, int hw, int pools) {
  __shared__ float ssum[4][VC], smax[4][VC];
  __shared__ int sarg[4][VC];
  const int b = blockIdx.x / VSEG, seg = blockIdx.x % VSEG;
  const int per = (hw + VSEG - 1) / VSEG;
  const int p0 = seg * per, p1 = min(p0 + per, hw);
  const int c = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const bool do_avg = pools & POOL_AVG, do_max = pools & POOL_MAX;
  const float* base = u + (size_t)b * hw * VC + c;
  const float* gb = GATED ? gate + (size_t)b * hw : nullptr;
  float s = 0.f, mx = -INFINITY;
  int am = 0x7fffffff;
#pragma unroll 4
  for (int p = p0 + rl; p < p1; p += 4) {
    float v = base[(size_t)p * VC];
    if (GATED) v = gb[p] * v;
    if (do_avg) s += v;
    if (do_max && pool_takes(v, mx)) {               // strict >: the first maximum of this wave's increasing pixels; NaN propagates
      mx = v;
      am = p;
    }
  }
  ssum[rl][c] = s;
  smax[rl][c] = mx;
  sarg[rl][c] = am;
  __syncthreads();
  if (rl == 0) {
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      s += ssum[k][c];
      const float v = smax[k][c];
      const int a = sarg[k][c];
      if (pool_merge_takes(v, a, mx, am)) {
        mx = v;
        am = a;
      }
    }
    const int o = (b * VSEG + seg) * VC + c;
    psum[o] = s;
    pmax[o] = mx;
    parg[o] = am;
  }
}

// ---- merge the segments, shared MLP 64 -> hidden -> 64 on the present rows, sigmoid ----------------------------------------- //
// one block of 256 per image: 4 lanes per channel walk the segments, 16 lanes per hidden unit do the 64-long dot products
__global__ __launch_bounds__(256) void var_mlp_kernel(const float* __restrict__ psum, const float* __restrict__ pmax,
                                                      const int* __restrict__ parg, const float* __restrict__ fc1,
                                                      const float* __restrict__ fc2, float* __restrict__ avg, float* __restrict__ mx,
                                                      int* __restrict__ arg, float* __restrict__ s, int hw, int hidden, int pools) {
  __shared__ float sa[VC], sm[VC], ha[16], hm[16], qs[4][VC], qm[4][VC];
  __shared__ int qa[4][VC];
  const int b = blockIdx.x, c = threadIdx.x & 63, q = threadIdx.x >> 6;
  const bool do_avg = pools & POOL_AVG, do_max = pools & POOL_MAX;
  float sum = 0.f, m = -INFINITY;
  int am = 0x7fffffff;
  for (int k = q; k < VSEG; k += 4) {
    const int o = (b * VSEG + k) * VC + c;
    sum += psum[o];
    const float v = pmax[o];
    const int a = parg[o];
    if (pool_merge_takes(v, a, m, am)) {
      m = v;
      am = a;
    }
  }
  qs[q][c] = sum;
  qm[q][c] = m;
  qa[q][c] = am;
  __syncthreads();
  if (q == 0) {
    sum = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) sum += qs[k][c];      // segment order: (0,4,8,..) + (1,5,..) + ...
    m = qm[0][c];
    am = qa[0][c];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      const float v = qm[k][c];
      const int a = qa[k][c];
      if (pool_merge_takes(v, a, m, am)) {
        m = v;
        am = a;
      }
    }
    const float a_ = sum / (float)hw;
    if (do_avg) avg[b * VC + c] = a_;
    if (do_max) {
      mx[b * VC + c] = m;
      arg[b * VC + c] = am;
    }
    sa[c] = a_;
    sm[c] = do_max ? m : 0.f;                          // an absent row is a row of zeros: relu(fc1 0) = 0 adds +0 to the logit
  }
  __syncthreads();
  {
    const int j = threadIdx.x >> 4, part = threadIdx.x & 15;   // hidden unit j (<= 16), 4 inputs per lane
    float x0 = 0.f, x1 = 0.f;
    if (j < hidden) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float w = fc1[j * VC + part * 4 + k];
        x0 += w * sa[part * 4 + k];
        x1 += w * sm[part * 4 + k];
      }
    }
    x0 = var_sum16(x0);
    x1 = var_sum16(x1);
    if (j < hidden && part == 0) {
      ha[j] = x0 < 0.f ? 0.f : x0;                     // ReLU that lets a NaN through like ATen's
      hm[j] = x1 < 0.f ? 0.f : x1;
    }
  }
  __syncthreads();
  if (q == 0) {
    float l0 = 0.f, l1 = 0.f;
    for (int j = 0; j < hidden; ++j) {
      const float w = fc2[c * hidden + j];
      l0 += w * ha[j];
      l1 += w * hm[j];
    }
    const float l = do_avg ? (do_max ? l0 + l1 : l0) : l1;
    s[b * VC + c] = 1.f / (1.f + expf(-l));
  }
}

// ---- channel pooling of a = s_c * u: pooled[pix][present maps, Avg first], argc[pix] = first arg-max channel ------------------ //
template <bool SCALED>
__global__ __launch_bounds__(256) void var_pool_chan_kernel(const float* __restrict__ u, const float* __restrict__ s,
                                                            float* __restrict__ pooled, int* __restrict__ argc, int hw, long npix,
                                                            int pools) {
  const long pix = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int cq = threadIdx.x & 15;
  if (pix >= npix) return;                             // whole 16-lane rows leave together: the row reductions below stay complete
  const bool do_avg = pools & POOL_AVG, do_max = pools & POOL_MAX;
  float4 v = *reinterpret_cast<const float4*>(u + pix * VC + cq * 4);
  if (SCALED) {
    const float4 sc = *reinterpret_cast<const float4*>(s + (pix / hw) * VC + cq * 4);
    v.x *= sc.x; v.y *= sc.y; v.z *= sc.z; v.w *= sc.w;
  }
  const int np = do_avg && do_max ? 2 : 1;
  if (do_avg) {
    const float sum = var_sum16((v.x + v.y) + (v.z + v.w));
    if (cq == 0) pooled[pix * np] = sum / (float)VC;
  }
  if (do_max) {
    float mx = v.x;
    int am = cq * 4;
    if (pool_takes(v.y, mx)) { mx = v.y; am = cq * 4 + 1; }
    if (pool_takes(v.z, mx)) { mx = v.z; am = cq * 4 + 2; }
    if (pool_takes(v.w, mx)) { mx = v.w; am = cq * 4 + 3; }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
      const float ov = __shfl_xor(mx, o, 16);
      const int oa = __shfl_xor(am, o, 16);
      if (pool_merge_takes(ov, oa, mx, am)) {
        mx = ov;
        am = oa;
      }
    }
    if (cq == 0) {
      pooled[pix * np + np - 1] = mx;
      argc[pix] = am;
    }
  }
}

// ---- m = sigmoid(conv7x7 pad 3 (NP -> 1, no bias)(pooled)) ---------------------------------------------------------------------- //
template <int NP>
__global__ __launch_bounds__(256) void var_conv7_kernel(const float* __restrict__ pooled, const float* __restrict__ w7,
                                                        float* __restrict__ m, int h, int w, long npix) {
  __shared__ float sw[NP * 49];
  if (threadIdx.x < NP * 49) sw[threadIdx.x] = w7[threadIdx.x];        // [map][kh][kw]
  __syncthreads();
  const long pix = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= npix) return;
  const int hw = h * w;
  const long b = pix / hw;
  const int rem = (int)(pix - b * hw);
  const int y = rem / w, x = rem - y * w;
  const float* img = pooled + b * hw * NP;
  float acc = 0.f;
  // a tap outside the image reads a clamped address and contributes w * 0: the same sum as skipping it, without a divergent branch
#pragma unroll
  for (int kh = 0; kh < 7; ++kh) {
    const int yy = y + kh - 3;
    const bool oky = yy >= 0 && yy < h;
    const int yc = min(max(yy, 0), h - 1);
#pragma unroll
    for (int kw = 0; kw < 7; ++kw) {
      const int xx = x + kw - 3;
      const bool ok = oky && xx >= 0 && xx < w;
      const int xc = min(max(xx, 0), w - 1);
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        float p = img[(yc * w + xc) * NP + k];
        if (!ok) p = 0.f;
        acc += sw[k * 49 + kh * 7 + kw] * p;
      }
    }
  }
  m[pix] = 1.f / (1.f + expf(-acc));
}

// ---- closing kernels ------------------------------------------------------------------------------------------------------------ //
// out = z + skip;  z = m (s u) (S_FIRST: the channel gate was applied first, CA-SA), s (m u) (SA-CA), s u or m u
template <bool HAS_S, bool HAS_M, bool S_FIRST>
__global__ __launch_bounds__(256) void var_gate_add_kernel(const float* __restrict__ u, const float* __restrict__ s,
                                                           const float* __restrict__ m, const float* __restrict__ skip,
                                                           float* __restrict__ out, int hw, long total4) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long)gridDim.x * 256) {
    const long pix = i >> 4;
    const int q = (int)(i & 15);
    float4 v = reinterpret_cast<const float4*>(u)[i];
    const float4 k = reinterpret_cast<const float4*>(skip)[i];
    float4 sc = make_float4(1.f, 1.f, 1.f, 1.f);
    float g = 1.f;
    if (HAS_S) sc = *reinterpret_cast<const float4*>(s + (pix / hw) * VC + q * 4);
    if (HAS_M) g = m[pix];
    if (HAS_S && HAS_M && S_FIRST) {
      v.x = g * (sc.x * v.x); v.y = g * (sc.y * v.y); v.z = g * (sc.z * v.z); v.w = g * (sc.w * v.w);
    } else if (HAS_S && HAS_M) {
      v.x = sc.x * (g * v.x); v.y = sc.y * (g * v.y); v.z = sc.z * (g * v.z); v.w = sc.w * (g * v.w);
    } else if (HAS_S) {
      v.x = sc.x * v.x; v.y = sc.y * v.y; v.z = sc.z * v.z; v.w = sc.w * v.w;
    } else {
      v.x = g * v.x; v.y = g * v.y; v.z = g * v.z; v.w = g * v.w;
    }
    v.x += k.x; v.y += k.y; v.z += k.z; v.w += k.w;
    reinterpret_cast<float4*>(out)[i] = v;
  }
}

// cat[pix][0:64] = s u, cat[pix][64:128] = m u (the reference's torch.cat([caout, saout], 1))
__global__ __launch_bounds__(256) void var_gated_cat_kernel(const float* __restrict__ u, const float* __restrict__ s,
                                                            const float* __restrict__ m, float* __restrict__ cat, int hw,
                                                            long total4) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long)gridDim.x * 256) {
    const long pix = i >> 4;
    const int q = (int)(i & 15);
    const float4 v = reinterpret_cast<const float4*>(u)[i];
    const float4 sc = *reinterpret_cast<const float4*>(s + (pix / hw) * VC + q * 4);
    const float g = m[pix];
    float4* o = reinterpret_cast<float4*>(cat + pix * (2 * VC));
    o[q] = make_float4(sc.x * v.x, sc.y * v.y, sc.z * v.z, sc.w * v.w);
    o[16 + q] = make_float4(g * v.x, g * v.y, g * v.z, g * v.w);
  }
}

// ---- backward ------------------------------------------------------------------------------------------------------------------- //
// With ChanBwd(ds; a) = [Avg] davg_c / hw + [p = arg_c] dmx_c (davg, dmx from ds through the shared MLP) and
// SpatBwd(dm; a) = [Avg] dpa_p / 64 + [c = argc_p] dpm_p (dpooled = conv7^T(dm m (1 - m))), the gradient dz at z becomes
//     CA-SA  dm = sum_c dz s u;  dy = m dz + SpatBwd;  ds = sum_p dy u;  du = s dy + ChanBwd
//     SA-CA  ds = sum_p dz m u;  dy = s dz + ChanBwd;  dm = sum_c dy u;  du = m dy + SpatBwd
//     CA     ds = sum_p dz u;    du = s dz + ChanBwd          SA   dm = sum_c dz u;   du = m dz + SpatBwd
//     CA|SA  ds = sum_p dz_c u,  dm = sum_c dz_s u;           du = s dz_c + m dz_s + ChanBwd + SpatBwd
// Every line is one call of var_bwd_pass_kernel -- a pass over (dz, u) that forms v = [s_c][m_p] dz (+ a term), takes the dot
// products with u over channels (-> dA = dm m (1 - m)) and / or over a segment's pixels (-> partials), and / or writes
// du = [s_c][m_p] v (+ terms) -- with small kernels between the passes.  Nothing tensor-sized is written but du.
constexpr int BSEG = 32;         // pixel segments per image of a backward pass

struct VarPass {
  const float* dza;              // dz (CA|SA: its channel half), row stride ld
  const float* dzb;              // CA|SA: the spatial half of dz, else null
  const float *u, *s, *m;
  const float *davg, *dmx;       // ChanBwd sources [n][64]
  const int* arg;
  const float* dpooled;          // SpatBwd source [n][hw][|P|]
  const int* argc;
  float *dsp, *dA, *du;          // outputs: segment partials [n][BSEG][64], dA [n][hw], du [n][hw][64]
  int ld, hw, pools;
  int pre_s, pre_m;              // v = [s_c][m_p] dza
  int pre_chan, pre_spat;        // v += ChanBwd / SpatBwd
  int dot_row, row_s, row_b;     // dm_p = sum_c (row_b ? dzb : v) u [s_c]
  int dot_col, col_m;            // partial_c = sum_p v u [m_p]
  int write, post_s, post_m;     // du = [s_c][m_p] v
  int post_b, post_chan, post_spat;   // du += m_p dzb, ChanBwd, SpatBwd
};

__device__ __forceinline__ float4 var_chan_term(const VarPass& a, int b, int p, int q) {
  float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
  if (a.pools & POOL_AVG) {
    const float4 d = *reinterpret_cast<const float4*>(a.davg + b * VC + q * 4);
    const float inv = 1.f / (float)a.hw;
    t = make_float4(d.x * inv, d.y * inv, d.z * inv, d.w * inv);
  }
  if (a.pools & POOL_MAX) {
    const int4 ix = *reinterpret_cast<const int4*>(a.arg + b * VC + q * 4);
    const float4 d = *reinterpret_cast<const float4*>(a.dmx + b * VC + q * 4);
    if (ix.x == p) t.x += d.x;
    if (ix.y == p) t.y += d.y;
    if (ix.z == p) t.z += d.z;
    if (ix.w == p) t.w += d.w;
  }
  return t;
}

__device__ __forceinline__ float4 var_spat_term(const VarPass& a, long pix, int q) {
  float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
  const int np = a.pools == 3 ? 2 : 1;
  if (a.pools & POOL_AVG) {
    const float d = a.dpooled[pix * np] * (1.f / (float)VC);
    t = make_float4(d, d, d, d);
  }
  if (a.pools & POOL_MAX) {
    const int ix = a.argc[pix] - q * 4;
    const float d = a.dpooled[pix * np + np - 1];
    if (ix == 0) t.x += d;
    if (ix == 1) t.y += d;
    if (ix == 2) t.z += d;
    if (ix == 3) t.w += d;
  }
  return t;
}

// grid (BSEG, n), 256 threads = 16 pixel lanes x 16 channel quads; du may alias dza (the fix-up pass of CA-SA): no __restrict__
__global__ __launch_bounds__(256) void var_bwd_pass_kernel(const VarPass a) {
  __shared__ float sacc[16][VC];
  const int b = blockIdx.y, seg = blockIdx.x;
  const int per = (a.hw + BSEG - 1) / BSEG;
  const int p0 = seg * per, p1 = min(p0 + per, a.hw);
  const int g = threadIdx.x >> 4, q = threadIdx.x & 15;
  float4 sc = make_float4(1.f, 1.f, 1.f, 1.f);
  if (a.s) sc = *reinterpret_cast<const float4*>(a.s + b * VC + q * 4);
  float4 col = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int p = p0 + g; p < p1; p += 16) {            // a 16-lane row stays together: the row reduction below is complete
    const long pix = (long)b * a.hw + p;
    float4 v = *reinterpret_cast<const float4*>(a.dza + pix * a.ld + q * 4);
    float4 uu = make_float4(0.f, 0.f, 0.f, 0.f);       // only the dot products read u (the fix-up pass of CA-SA takes neither)
    if (a.dot_row || a.dot_col) uu = *reinterpret_cast<const float4*>(a.u + pix * VC + q * 4);
    const float mp = a.m ? a.m[pix] : 1.f;
    float4 vb = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.dzb) vb = *reinterpret_cast<const float4*>(a.dzb + pix * a.ld + q * 4);
    if (a.pre_s) { v.x *= sc.x; v.y *= sc.y; v.z *= sc.z; v.w *= sc.w; }
    if (a.pre_m) { v.x *= mp; v.y *= mp; v.z *= mp; v.w *= mp; }
    if (a.pre_chan) { const float4 t = var_chan_term(a, b, p, q); v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w; }
    if (a.pre_spat) { const float4 t = var_spat_term(a, pix, q); v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w; }
    if (a.dot_row) {
      const float4 r = a.row_b ? vb : v;
      float4 w = uu;
      if (a.row_s) { w.x *= sc.x; w.y *= sc.y; w.z *= sc.z; w.w *= sc.w; }
      const float dm = var_sum16((r.x * w.x + r.y * w.y) + (r.z * w.z + r.w * w.w));
      if (q == 0) a.dA[pix] = dm * (mp * (1.f - mp));
    }
    if (a.dot_col) {
      float4 w = uu;
      if (a.col_m) { w.x *= mp; w.y *= mp; w.z *= mp; w.w *= mp; }
      col.x += v.x * w.x; col.y += v.y * w.y; col.z += v.z * w.z; col.w += v.w * w.w;
    }
    if (a.write) {
      float4 o = v;
      if (a.post_s) { o.x *= sc.x; o.y *= sc.y; o.z *= sc.z; o.w *= sc.w; }
      if (a.post_m) { o.x *= mp; o.y *= mp; o.z *= mp; o.w *= mp; }
      if (a.post_b) { o.x += mp * vb.x; o.y += mp * vb.y; o.z += mp * vb.z; o.w += mp * vb.w; }
      if (a.post_chan) { const float4 t = var_chan_term(a, b, p, q); o.x += t.x; o.y += t.y; o.z += t.z; o.w += t.w; }
      if (a.post_spat) { const float4 t = var_spat_term(a, pix, q); o.x += t.x; o.y += t.y; o.z += t.z; o.w += t.w; }
      *reinterpret_cast<float4*>(a.du + pix * VC + q * 4) = o;
    }
  }
  if (a.dot_col) {
    *reinterpret_cast<float4*>(&sacc[g][q * 4]) = col;
    __syncthreads();
    if (threadIdx.x < VC) {
      float t = 0.f;
#pragma unroll
      for (int k = 0; k < 16; ++k) t += sacc[k][threadIdx.x];
      a.dsp[((size_t)b * BSEG + seg) * VC + threadIdx.x] = t;
    }
  }
}

// ds = sum of the segment partials; dl = ds s (1 - s) through the shared MLP: davg, dmx [n][64] and this image's share of dfc1 / dfc2
__global__ __launch_bounds__(256) void var_bwd_mlp_kernel(const float* __restrict__ dsp, const float* __restrict__ s,
                                                          const float* __restrict__ avg, const float* __restrict__ mx,
                                                          const float* __restrict__ fc1, const float* __restrict__ fc2,
                                                          float* __restrict__ davg, float* __restrict__ dmx, float* __restrict__ pw1,
                                                          float* __restrict__ pw2, int hidden, int pools) {
  __shared__ float sl[VC], sa[VC], sm[VC], xa[16], xm[16], dpa[16], dpm[16];
  const int b = blockIdx.x, t = threadIdx.x;
  const bool do_avg = pools & POOL_AVG, do_max = pools & POOL_MAX;
  if (t < VC) {
    float ds = 0.f;
    for (int k = 0; k < BSEG; ++k) ds += dsp[((size_t)b * BSEG + k) * VC + t];
    const float sv = s[b * VC + t];
    sl[t] = ds * (sv * (1.f - sv));
    sa[t] = do_avg ? avg[b * VC + t] : 0.f;
    sm[t] = do_max ? mx[b * VC + t] : 0.f;
  }
  __syncthreads();
  {
    const int j = t >> 4, part = t & 15;
    float x0 = 0.f, x1 = 0.f;
    if (j < hidden) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float w = fc1[j * VC + part * 4 + k];
        x0 += w * sa[part * 4 + k];
        x1 += w * sm[part * 4 + k];
      }
    }
    x0 = var_sum16(x0);
    x1 = var_sum16(x1);
    if (j < hidden && part == 0) {
      xa[j] = x0;
      xm[j] = x1;
    }
  }
  __syncthreads();
  if (t < hidden) {
    float dh = 0.f;
    for (int c = 0; c < VC; ++c) dh += sl[c] * fc2[c * hidden + t];
    dpa[t] = (do_avg && xa[t] > 0.f) ? dh : 0.f;
    dpm[t] = (do_max && xm[t] > 0.f) ? dh : 0.f;
  }
  __syncthreads();
  if (t < VC) {
    float da = 0.f, dm = 0.f;
    for (int j = 0; j < hidden; ++j) {
      const float w = fc1[j * VC + t];
      da += dpa[j] * w;
      dm += dpm[j] * w;
      pw1[((size_t)b * hidden + j) * VC + t] = dpa[j] * sa[t] + dpm[j] * sm[t];
      const float ra = (do_avg && xa[j] > 0.f) ? xa[j] : 0.f, rm = (do_max && xm[j] > 0.f) ? xm[j] : 0.f;
      pw2[((size_t)b * VC + t) * hidden + j] = sl[t] * (ra + rm);
    }
    if (do_avg) davg[b * VC + t] = da;
    if (do_max) dmx[b * VC + t] = dm;
  }
}

// out[i] = (acc ? out[i] : 0) + sum over images of part[b][i], in image order
__global__ void var_bwd_sum_kernel(const float* __restrict__ part, float* __restrict__ out, int n, int count, int acc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  float t = 0.f;
  for (int b = 0; b < n; ++b) t += part[(size_t)b * count + i];
  out[i] = acc ? out[i] + t : t;
}

// dpooled = conv7^T(dA): dpooled[pix][k] = sum over taps of w7[k][kh][kw] dA[y + 3 - kh][x + 3 - kw]
template <int NP>
__global__ __launch_bounds__(256) void var_bwd_conv7_dgrad_kernel(const float* __restrict__ dA, const float* __restrict__ w7,
                                                                  float* __restrict__ dpooled, int h, int w, long npix) {
  __shared__ float sw[NP * 49];
  if (threadIdx.x < NP * 49) sw[threadIdx.x] = w7[threadIdx.x];
  __syncthreads();
  const long pix = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= npix) return;
  const int hw = h * w;
  const long b = pix / hw;
  const int rem = (int)(pix - b * hw);
  const int y = rem / w, x = rem - y * w;
  const float* img = dA + b * hw;
  float acc[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) acc[k] = 0.f;
#pragma unroll
  for (int kh = 0; kh < 7; ++kh) {
    const int yy = y + 3 - kh;
    const bool oky = yy >= 0 && yy < h;
    const int yc = min(max(yy, 0), h - 1);
#pragma unroll
    for (int kw = 0; kw < 7; ++kw) {
      const int xx = x + 3 - kw;
      const bool ok = oky && xx >= 0 && xx < w;
      const int xc = min(max(xx, 0), w - 1);
      float d = img[yc * w + xc];
      if (!ok) d = 0.f;
#pragma unroll
      for (int k = 0; k < NP; ++k) acc[k] += sw[k * 49 + kh * 7 + kw] * d;
    }
  }
#pragma unroll
  for (int k = 0; k < NP; ++k) dpooled[pix * NP + k] = acc[k];
}

// dw7[k][kh][kw] = sum over images and pixels of dA[y][x] pooled[y + kh - 3][x + kw - 3][k]: one block per tap, fixed tree
__global__ __launch_bounds__(256) void var_bwd_conv7_wgrad_kernel(const float* __restrict__ dA, const float* __restrict__ pooled,
                                                                  float* __restrict__ dw7, int np, int h, int w, long npix, int acc) {
  __shared__ float sred[256];
  const int k = blockIdx.x / 49, tap = blockIdx.x % 49, kh = tap / 7, kw = tap % 7;
  const int hw = h * w;
  float t = 0.f;
  for (long pix = threadIdx.x; pix < npix; pix += 256) {
    const long b = pix / hw;
    const int rem = (int)(pix - b * hw);
    const int y = rem / w, x = rem - y * w;
    const int yy = y + kh - 3, xx = x + kw - 3;
    if (yy >= 0 && yy < h && xx >= 0 && xx < w) t += dA[pix] * pooled[(b * hw + yy * w + xx) * np + k];
  }
  sred[threadIdx.x] = t;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) sred[threadIdx.x] += sred[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) dw7[blockIdx.x] = acc ? dw7[blockIdx.x] + sred[0] : sred[0];
}

static inline int var_ew_blocks(long total4) {
  const long b = (total4 + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

static inline bool var_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace srhip

using namespace srhip;

extern "C" {

size_t srhip_attn_var_workspace(int n) { return n > 0 ? (size_t)n * VSEG * VC * 3 * sizeof(float) : 0; }

int srhip_attn_var_fwd(const float* u, const float* fc1, const float* fc2, const float* w7, float* avg, float* mx, int* arg, float* s,
                       float* pooled, int* argc, float* m, float* ws, size_t ws_bytes, int n, int h, int w, int c, int hidden,
                       int order, int pools, void* stream) {
  SRHIP_REQUIRE(n > 0 && h > 0 && w > 0, "attn_var_fwd: needs n, h, w > 0, got %d / %d / %d", n, h, w);
  SRHIP_REQUIRE(c == VC, "attn_var_fwd: built for C = 64, got %d", c);
  SRHIP_REQUIRE(order >= SRHIP_ATTN_CA_SA && order <= SRHIP_ATTN_CA_PAR_SA, "attn_var_fwd: order must be 0 .. 4, got %d", order);
  SRHIP_REQUIRE(pools >= 1 && pools <= 3, "attn_var_fwd: pools must be 1 (Avg), 2 (Max) or 3, got %d", pools);
  SRHIP_REQUIRE((long)n * h * w < (1L << 31) / VC, "attn_var_fwd: more than 2^31 elements");
  const bool has_c = order != SRHIP_ATTN_SA, has_s = order != SRHIP_ATTN_CA;
  const bool do_avg = pools & POOL_AVG, do_max = pools & POOL_MAX;
  SRHIP_REQUIRE(u && var_aligned(u), "attn_var_fwd: u is null or not 16-byte aligned");
  if (has_c) {
    SRHIP_REQUIRE(hidden >= 1 && hidden <= 16, "attn_var_fwd: hidden must be 1 .. 16, got %d", hidden);
    SRHIP_REQUIRE(fc1 && fc2 && s && var_aligned(s), "attn_var_fwd: fc1 / fc2 / s are null (or s unaligned) for a variant with a channel gate");
    SRHIP_REQUIRE((!do_avg || avg) && (!do_max || (mx && arg)), "attn_var_fwd: a statistic of the channel gate's pool set has no output");
    SRHIP_REQUIRE(ws && ws_bytes >= srhip_attn_var_workspace(n), "attn_var_fwd: workspace too small (%zu bytes)", ws_bytes);
  }
  if (has_s)
    SRHIP_REQUIRE(w7 && pooled && m && (!do_max || argc), "attn_var_fwd: w7 / pooled / m / argc are null for a variant with a spatial gate");
  const int hw = h * w;
  const long npix = (long)n * hw;
  hipStream_t st = as_stream(stream);
  float* psum = ws;
  float* pmax = ws + (size_t)n * VSEG * VC;
  int* parg = reinterpret_cast<int*>(ws + (size_t)2 * n * VSEG * VC);

  auto spatial = [&](const float* scale) {
    if (scale)
      hipLaunchKernelGGL(var_pool_chan_kernel<true>, dim3(cdiv(npix, 16)), dim3(256), 0, st, u, scale, pooled, argc, hw, npix, pools);
    else
      hipLaunchKernelGGL(var_pool_chan_kernel<false>, dim3(cdiv(npix, 16)), dim3(256), 0, st, u, scale, pooled, argc, hw, npix, pools);
    if (pools == 3)
      hipLaunchKernelGGL(var_conv7_kernel<2>, dim3(cdiv(npix, 256)), dim3(256), 0, st, pooled, w7, m, h, w, npix);
    else
      hipLaunchKernelGGL(var_conv7_kernel<1>, dim3(cdiv(npix, 256)), dim3(256), 0, st, pooled, w7, m, h, w, npix);
  };
  auto channel = [&](const float* gate) {
    if (gate)
      hipLaunchKernelGGL(var_pool_pix_kernel<true>, dim3(n * VSEG), dim3(256), 0, st, u, gate, psum, pmax, parg, hw, pools);
    else
      hipLaunchKernelGGL(var_pool_pix_kernel<false>, dim3(n * VSEG), dim3(256), 0, st, u, gate, psum, pmax, parg, hw, pools);
    hipLaunchKernelGGL(var_mlp_kernel, dim3(n), dim3(256), 0, st, psum, pmax, parg, fc1, fc2, avg, mx, arg, s, hw, hidden, pools);
  };
  switch (order) {
    case SRHIP_ATTN_CA_SA: channel(nullptr); spatial(s); break;
    case SRHIP_ATTN_SA_CA: spatial(nullptr); channel(m); break;
    case SRHIP_ATTN_CA: channel(nullptr); break;
    case SRHIP_ATTN_SA: spatial(nullptr); break;
    default: channel(nullptr); spatial(nullptr); break;
  }
  return check_launch("attn_var_fwd");
}

int srhip_attn_var_close(const float* u, const float* s, const float* m, const float* skip, float* out, int n, int hw, int c, int order,
                         int cat, void* stream) {
  SRHIP_REQUIRE(n > 0 && hw > 0, "attn_var_close: needs n, hw > 0, got %d / %d", n, hw);
  SRHIP_REQUIRE(c == VC, "attn_var_close: built for C = 64, got %d", c);
  SRHIP_REQUIRE(order >= SRHIP_ATTN_CA_SA && order <= SRHIP_ATTN_CA_PAR_SA, "attn_var_close: order must be 0 .. 4, got %d", order);
  SRHIP_REQUIRE((cat != 0) == (order == SRHIP_ATTN_CA_PAR_SA), "attn_var_close: the gated cat is CA|SA's closing form and only its");
  SRHIP_REQUIRE((long)n * hw < (1L << 31) / (2 * VC), "attn_var_close: more than 2^31 elements");
  const bool has_c = order != SRHIP_ATTN_SA, has_s = order != SRHIP_ATTN_CA;
  SRHIP_REQUIRE(u && out && var_aligned(u) && var_aligned(out), "attn_var_close: u / out null or not 16-byte aligned");
  SRHIP_REQUIRE((!has_c || (s && var_aligned(s))) && (!has_s || m), "attn_var_close: a gate of this variant is null (or s unaligned)");
  SRHIP_REQUIRE(cat || (skip && var_aligned(skip)), "attn_var_close: skip null or not 16-byte aligned");
  const long total4 = (long)n * hw * (VC / 4);
  const dim3 grid(var_ew_blocks(total4)), block(256);
  hipStream_t st = as_stream(stream);
  switch (order) {
    case SRHIP_ATTN_CA_SA: hipLaunchKernelGGL((var_gate_add_kernel<true, true, true>), grid, block, 0, st, u, s, m, skip, out, hw, total4); break;
    case SRHIP_ATTN_SA_CA: hipLaunchKernelGGL((var_gate_add_kernel<true, true, false>), grid, block, 0, st, u, s, m, skip, out, hw, total4); break;
    case SRHIP_ATTN_CA: hipLaunchKernelGGL((var_gate_add_kernel<true, false, true>), grid, block, 0, st, u, s, m, skip, out, hw, total4); break;
    case SRHIP_ATTN_SA: hipLaunchKernelGGL((var_gate_add_kernel<false, true, true>), grid, block, 0, st, u, s, m, skip, out, hw, total4); break;
    default: hipLaunchKernelGGL(var_gated_cat_kernel, grid, block, 0, st, u, s, m, out, hw, total4); break;
  }
  return check_launch("attn_var_close");
}

size_t srhip_attn_var_bwd_workspace(int n, int h, int w, int hidden) {
  if (n <= 0 || h <= 0 || w <= 0 || hidden < 0) return 0;
  const size_t hw = (size_t)h * w;
  return ((size_t)n * BSEG * VC + 2 * (size_t)n * VC + 3 * (size_t)n * hw + 2 * (size_t)n * (hidden > 0 ? hidden : 1) * VC) * sizeof(float);
}

int srhip_attn_var_bwd(const float* dz, const float* u, const float* s, const float* m, const float* avg, const float* mx, const int* arg,
                       const float* pooled, const int* argc, const float* w7, const float* fc1, const float* fc2, float* du, float* dw7,
                       int accumulate_dw7, float* dfc1, float* dfc2, int accumulate_dfc, float* ws, size_t ws_bytes, int n, int h, int w,
                       int c, int hidden, int order, int pools, void* stream) {
  SRHIP_REQUIRE(n > 0 && h > 0 && w > 0, "attn_var_bwd: needs n, h, w > 0, got %d / %d / %d", n, h, w);
  SRHIP_REQUIRE(c == VC, "attn_var_bwd: built for C = 64, got %d", c);
  SRHIP_REQUIRE(order >= SRHIP_ATTN_CA_SA && order <= SRHIP_ATTN_CA_PAR_SA, "attn_var_bwd: order must be 0 .. 4, got %d", order);
  SRHIP_REQUIRE(pools >= 1 && pools <= 3, "attn_var_bwd: pools must be 1 (Avg), 2 (Max) or 3, got %d", pools);
  SRHIP_REQUIRE((long)n * h * w < (1L << 31) / (2 * VC), "attn_var_bwd: more than 2^31 elements");
  const bool has_c = order != SRHIP_ATTN_SA, has_s = order != SRHIP_ATTN_CA;
  const bool do_avg = pools & POOL_AVG, do_max = pools & POOL_MAX;
  SRHIP_REQUIRE(dz && u && du && var_aligned(dz) && var_aligned(u) && var_aligned(du), "attn_var_bwd: dz / u / du null or not 16-byte aligned");
  if (has_c) {
    SRHIP_REQUIRE(hidden >= 1 && hidden <= 16, "attn_var_bwd: hidden must be 1 .. 16, got %d", hidden);
    SRHIP_REQUIRE(s && fc1 && fc2 && dfc1 && dfc2 && var_aligned(s), "attn_var_bwd: s / fc1 / fc2 / dfc1 / dfc2 null (or s unaligned) for a variant with a channel gate");
    SRHIP_REQUIRE((!do_avg || avg) && (!do_max || (mx && arg && var_aligned(arg))), "attn_var_bwd: a saved statistic of the channel gate's pool set is null");
  }
  if (has_s)
    SRHIP_REQUIRE(m && pooled && w7 && dw7 && (!do_max || argc), "attn_var_bwd: m / pooled / w7 / dw7 / argc null for a variant with a spatial gate");
  SRHIP_REQUIRE(ws && var_aligned(ws) && ws_bytes >= srhip_attn_var_bwd_workspace(n, h, w, hidden),
                "attn_var_bwd: workspace null, not 16-byte aligned or too small (%zu bytes)", ws_bytes);
  const int hw = h * w;
  const long npix = (long)n * hw;
  hipStream_t st = as_stream(stream);
  const int hid = hidden > 0 ? hidden : 1;
  float* dsp = ws;                                    // every section a multiple of 64 floats or at the end: 16-byte aligned rows
  float* davg = dsp + (size_t)n * BSEG * VC;
  float* dmx = davg + (size_t)n * VC;
  float* pw1 = dmx + (size_t)n * VC;
  float* pw2 = pw1 + (size_t)n * hid * VC;
  float* dA = pw2 + (size_t)n * hid * VC;
  float* dpooled = dA + npix;
  const int np = pools == 3 ? 2 : 1;
  const int ld = order == SRHIP_ATTN_CA_PAR_SA ? 2 * VC : VC;

  VarPass base = {};
  base.dza = dz; base.u = u; base.s = has_c ? s : nullptr; base.m = has_s ? m : nullptr;
  base.davg = davg; base.dmx = dmx; base.arg = arg; base.dpooled = dpooled; base.argc = argc;
  base.dsp = dsp; base.dA = dA; base.du = du; base.ld = ld; base.hw = hw; base.pools = pools;
  auto pass = [&](const VarPass& p) { hipLaunchKernelGGL(var_bwd_pass_kernel, dim3(BSEG, n), dim3(256), 0, st, p); };
  auto mlp = [&]() {
    hipLaunchKernelGGL(var_bwd_mlp_kernel, dim3(n), dim3(256), 0, st, dsp, s, avg, mx, fc1, fc2, davg, dmx, pw1, pw2, hidden, pools);
    hipLaunchKernelGGL(var_bwd_sum_kernel, dim3(cdiv(hidden * VC, 256)), dim3(256), 0, st, pw1, dfc1, n, hidden * VC, accumulate_dfc);
    hipLaunchKernelGGL(var_bwd_sum_kernel, dim3(cdiv(hidden * VC, 256)), dim3(256), 0, st, pw2, dfc2, n, hidden * VC, accumulate_dfc);
  };
  auto conv7 = [&]() {
    if (np == 2)
      hipLaunchKernelGGL(var_bwd_conv7_dgrad_kernel<2>, dim3(cdiv(npix, 256)), dim3(256), 0, st, dA, w7, dpooled, h, w, npix);
    else
      hipLaunchKernelGGL(var_bwd_conv7_dgrad_kernel<1>, dim3(cdiv(npix, 256)), dim3(256), 0, st, dA, w7, dpooled, h, w, npix);
    hipLaunchKernelGGL(var_bwd_conv7_wgrad_kernel, dim3(np * 49), dim3(256), 0, st, dA, pooled, dw7, np, h, w, npix, accumulate_dw7);
  };
  VarPass p = base;
  switch (order) {
    case SRHIP_ATTN_CA_SA:
      p.dot_row = 1; p.row_s = 1; pass(p);
      conv7();
      p = base; p.pre_m = 1; p.pre_spat = 1; p.dot_col = 1; p.write = 1; p.post_s = 1; pass(p);
      mlp();
      p = base; p.dza = du; p.s = nullptr; p.m = nullptr; p.write = 1; p.post_chan = 1; pass(p);
      break;
    case SRHIP_ATTN_SA_CA:
      p.dot_col = 1; p.col_m = 1; pass(p);
      mlp();
      p = base; p.pre_s = 1; p.pre_chan = 1; p.dot_row = 1; pass(p);
      conv7();
      p = base; p.pre_s = 1; p.pre_chan = 1; p.write = 1; p.post_m = 1; p.post_spat = 1; pass(p);
      break;
    case SRHIP_ATTN_CA:
      p.dot_col = 1; pass(p);
      mlp();
      p = base; p.pre_s = 1; p.write = 1; p.post_chan = 1; pass(p);
      break;
    case SRHIP_ATTN_SA:
      p.dot_row = 1; pass(p);
      conv7();
      p = base; p.pre_m = 1; p.write = 1; p.post_spat = 1; pass(p);
      break;
    default:
      p.dzb = dz + VC; p.dot_col = 1; p.dot_row = 1; p.row_b = 1; pass(p);
      mlp();
      conv7();
      p = base; p.dzb = dz + VC; p.pre_s = 1; p.write = 1; p.post_b = 1; p.post_chan = 1; p.post_spat = 1; pass(p);
      break;
  }
  return check_launch("attn_var_bwd");
}

}  // extern "C"
