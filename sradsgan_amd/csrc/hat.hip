// HAT (reference model/hat.py): the window transformer's passes.  Tokens are NHWC rows of C = 96 floats (the reference's
// [b, h*w, c] sequence is the channels_last image itself, so patch embed / unembed are free).
//   * LayerNorm over the 96 channels of a token (eps 1e-5): forward, and backward with dgamma / dbeta from per-block partials
//     reduced in a fixed order;
//   * GELU (exact erf): forward and backward, element-wise;
//   * window attention, one kernel family for HAB's (shifted) window self-attention (SA) and OCAB's overlapping cross-attention
//     (OCA), head dimension 16, q / k / v read straight from the [tokens, 288] rows of the qkv Linear.  Roll, window partition,
//     unfold (zero padding) and window reverse are address arithmetic; the relative-position bias table is indexed modulo its
//     size (the reference's rpi_oca holds negative indices that table[idx] wraps); the shift mask adds -100.  The backward
//     recomputes P from the forward's per-row log-sum-exp (dS = P (dP - rowsum(dO O))), accumulates dS per (query, key) in the
//     block's LDS (one row per thread) and folds it into the table gradient in a fixed order; OCA's overlapping dK / dV go to
//     per-window slabs that a gather pass folds per pixel in a fixed order;
//   * HAB's combine out = x + k_b a + cs (s[b,c] u) (drop-path factor k_b, channel-attention scale s of CAB's output u) with the
//     channel attention at any C <= 128 (hidden <= 16, with biases), and its backward; the same kernels with 384 threads serve the
//     published widths 128 < C <= 192 (srhip_hatw_ca_fwd / srhip_hatw_combine_bwd; the rest of that family is hat_wide.hip).
// fp32 throughout; no atomics: every result is bit-identical from run to run.
#include "common.h"

namespace srhip {

constexpr int HAT_C = 96;          // embedding width
constexpr int HAT_HEADS = 6;       // heads of 16 channels
constexpr int HAT_D = 16;
constexpr int HAT_QKV = 3 * HAT_C; // qkv row
constexpr float HAT_LN_EPS = 1e-5f;
constexpr int HAT_BWD_BLOCKS = 64; // attention backward: most blocks per head (each walks windows g, g + G, ...)
constexpr int HAT_CA_MAXC = 128, HAT_CA_MAXHID = 16;
constexpr int HAT_CA_WIDE_MAXC = 192;   // the published widths (144, 180): 8 pixel lanes x C / 4 quads need 384 threads

// ---------------------------------------------------------------------------------------------------------------------------- //
// LayerNorm: one wave per token, lane l holds channels l and 64 + l (l < 32)
// ---------------------------------------------------------------------------------------------------------------------------- //

__global__ __launch_bounds__(256) void hat_ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                         const float* __restrict__ b, float* __restrict__ y,
                                                         float* __restrict__ mean, float* __restrict__ rstd, long tokens) {
  const long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= tokens) return;
  const int l = threadIdx.x & 63;
  const bool two = l < HAT_C - 64;
  const float* xr = x + t * HAT_C;
  const float x0 = xr[l], x1 = two ? xr[64 + l] : 0.f;
  const float mu = wave_sum(x0 + x1) / (float)HAT_C;
  const float d0 = x0 - mu, d1 = two ? x1 - mu : 0.f;
  const float var = wave_sum(d0 * d0 + d1 * d1) / (float)HAT_C;
  const float r = 1.f / sqrtf(var + HAT_LN_EPS);
  float* yr = y + t * HAT_C;
  yr[l] = d0 * r * g[l] + b[l];
  if (two) yr[64 + l] = d1 * r * g[64 + l] + b[64 + l];
  if (l == 0) {
    mean[t] = mu;
    rstd[t] = r;
  }
}

static int hat_ln_parts(long tokens) { const long b = (tokens + 3) / 4; return (int)(b < 512 ? b : 512); }

// dx = r (dy g - mean(dy g) - xhat mean(dy g xhat)) [+ dadd]; part[blk][0..95] = sum dy xhat, part[blk][96..191] = sum dy
__global__ __launch_bounds__(256) void hat_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                         const float* __restrict__ g, const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, const float* __restrict__ dadd,
                                                         float* __restrict__ dx, float* __restrict__ part, long tokens) {
  __shared__ float red[4][2 * HAT_C];
  const int wv = threadIdx.x >> 6, l = threadIdx.x & 63;
  const bool two = l < HAT_C - 64;
  const float g0 = g[l], g1 = two ? g[64 + l] : 0.f;
  float ag0 = 0.f, ag1 = 0.f, ab0 = 0.f, ab1 = 0.f;
  for (long t = (long)blockIdx.x * 4 + wv; t < tokens; t += (long)gridDim.x * 4) {
    const float* xr = x + t * HAT_C;
    const float* dr = dy + t * HAT_C;
    const float mu = mean[t], r = rstd[t];
    const float h0 = (xr[l] - mu) * r, h1 = two ? (xr[64 + l] - mu) * r : 0.f;
    const float e0 = dr[l], e1 = two ? dr[64 + l] : 0.f;
    const float q0 = e0 * g0, q1 = e1 * g1;
    const float c1 = wave_sum(q0 * h0 + q1 * h1) / (float)HAT_C;
    const float c2 = wave_sum(q0 + q1) / (float)HAT_C;
    float* o = dx + t * HAT_C;
    float v0 = r * (q0 - c2 - h0 * c1);
    if (dadd) v0 += dadd[t * HAT_C + l];
    o[l] = v0;
    if (two) {
      float v1 = r * (q1 - c2 - h1 * c1);
      if (dadd) v1 += dadd[t * HAT_C + 64 + l];
      o[64 + l] = v1;
    }
    ag0 += e0 * h0;
    ag1 += e1 * h1;
    ab0 += e0;
    ab1 += e1;
  }
  red[wv][l] = ag0;
  red[wv][HAT_C + l] = ab0;
  if (two) {
    red[wv][64 + l] = ag1;
    red[wv][HAT_C + 64 + l] = ab1;
  }
  __syncthreads();
  if (threadIdx.x < 2 * HAT_C) {
    const int c = threadIdx.x;
    part[(size_t)blockIdx.x * 2 * HAT_C + c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
  }
}

// out[c] = sum over the nparts rows of part[.][c]: one wave per column c, lane l walks rows l, l + 64, ... in order, then the
// wave's fixed butterfly (c < width; columns below `split` go to out0, the others to out1)
__global__ __launch_bounds__(64) void hat_sum_rows_kernel(const float* __restrict__ part, float* __restrict__ out0,
                                                          float* __restrict__ out1, int nparts, int width, int split) {
  const int c = blockIdx.x, l = threadIdx.x;
  float s = 0.f;
  for (int k = l; k < nparts; k += 64) s += part[(size_t)k * width + c];
  s = wave_sum(s);
  if (l != 0) return;
  if (c < split) {
    if (out0) out0[c] = s;
  } else if (out1) {
    out1[c - split] = s;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------- //
// GELU (erf), as nn.GELU(): y = x 0.5 (1 + erf(x / sqrt 2))
// ---------------------------------------------------------------------------------------------------------------------------- //

__device__ __forceinline__ float gelu_f(float x) { return x * 0.5f * (1.f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_d(float x) {
  const float cdf = 0.5f * (1.f + erff(x * 0.70710678118654752f));
  const float pdf = expf(-0.5f * x * x) * 0.39894228040143268f;
  return cdf + x * pdf;
}

__global__ __launch_bounds__(256) void hat_gelu_fwd_kernel(const float4* __restrict__ x, float4* __restrict__ y, long quads) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < quads; i += (long)gridDim.x * 256) {
    const float4 v = x[i];
    y[i] = make_float4(gelu_f(v.x), gelu_f(v.y), gelu_f(v.z), gelu_f(v.w));
  }
}

__global__ __launch_bounds__(256) void hat_gelu_bwd_kernel(const float4* __restrict__ dy, const float4* __restrict__ x,
                                                           float4* __restrict__ dx, long quads) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < quads; i += (long)gridDim.x * 256) {
    const float4 v = x[i], d = dy[i];
    dx[i] = make_float4(d.x * gelu_d(v.x), d.y * gelu_d(v.y), d.z * gelu_d(v.z), d.w * gelu_d(v.w));
  }
}

// ---------------------------------------------------------------------------------------------------------------------------- //
// Window attention
// ---------------------------------------------------------------------------------------------------------------------------- //

template <int OCA, int WS>
struct AttnGeom {
  static constexpr int NQ = WS * WS;
  static constexpr int OWS = WS + WS / 2;                // int(ws * 0.5) + ws (overlap_ratio 0.5)
  static constexpr int PAD = (OWS - WS) / 2;             // nn.Unfold padding
  static constexpr int KW = OCA ? OWS : WS;              // keys per row of the key window
  static constexpr int NK = KW * KW;
  static constexpr int L = OCA ? WS + OWS - 1 : 2 * WS - 1;
  static constexpr int T = L * L;                        // bias table rows
  static constexpr int C0 = OCA ? WS - OWS + 1 : WS - 1; // offset of the relative coordinate

  // table row of (query i, key j); the reference's table[rpi.view(-1)] wraps negative OCA indices
  __device__ static int bias_row(int i, int j) {
    const int qy = i / WS, qx = i % WS, ky = j / KW, kx = j % KW;
    int idx = OCA ? (ky - qy + C0) * L + (kx - qx + C0) : (qy - ky + C0) * L + (qx - kx + C0);
    return idx < 0 ? idx + T : idx;
  }
};

// region label of a shifted-window coordinate (calculate_mask: slices [0, H - ws), [H - ws, H - shift), [H - shift, H))
__device__ __forceinline__ int mask_label(int r, int n, int ws, int shift) { return r < n - ws ? 0 : (r < n - shift ? 1 : 2); }

// pixel (row index in [0, n*h*w)) of query / key slot j of window (bimg, wy, wx), or -1 for an OCA key in the zero padding
template <int OCA, int WS>
__device__ __forceinline__ long key_pixel(int j, int bimg, int wy, int wx, int h, int w, int shift) {
  using G = AttnGeom<OCA, WS>;
  const int ky = j / G::KW, kx = j % G::KW;
  int y, x;
  if (OCA) {
    y = wy * WS - G::PAD + ky;
    x = wx * WS - G::PAD + kx;
    if (y < 0 || y >= h || x < 0 || x >= w) return -1;
  } else {
    y = wy * WS + ky + shift;
    x = wx * WS + kx + shift;
    if (y >= h) y -= h;
    if (x >= w) x -= w;
  }
  return ((long)bimg * h + y) * w + x;
}

template <int WS>
__device__ __forceinline__ long query_pixel(int i, int bimg, int wy, int wx, int h, int w, int shift) {
  int y = wy * WS + i / WS + shift, x = wx * WS + i % WS + shift;
  if (y >= h) y -= h;
  if (x >= w) x -= w;
  return ((long)bimg * h + y) * w + x;
}

// -100 where query i and key j of a shifted window lie in different regions (SA with shift > 0 only)
template <int WS>
__device__ __forceinline__ float shift_mask(int i, int j, int wy, int wx, int h, int w, int shift) {
  const int li = 3 * mask_label(wy * WS + i / WS, h, WS, shift) + mask_label(wx * WS + i % WS, w, WS, shift);
  const int lj = 3 * mask_label(wy * WS + j / WS, h, WS, shift) + mask_label(wx * WS + j % WS, w, WS, shift);
  return li == lj ? 0.f : -100.f;
}

__device__ __forceinline__ float dot16(const float* a, const float* b) {
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < HAT_D; ++d) s += a[d] * b[d];
  return s;
}

// one block per (window, head); thread i < NQ owns query i (online softmax over the keys in order)
template <int OCA, int WS>
__global__ __launch_bounds__(192) void hat_attn_fwd_kernel(const float* __restrict__ qkv, const float* __restrict__ table,
                                                           float* __restrict__ out, float* __restrict__ lse, int h, int w,
                                                           int shift) {
  using G = AttnGeom<OCA, WS>;
  __shared__ __attribute__((aligned(16))) float ks[G::NK][HAT_D];
  __shared__ __attribute__((aligned(16))) float vs[G::NK][HAT_D];
  __shared__ float tab[G::T];
  const int head = blockIdx.y, nwx = w / WS, nwy = h / WS;
  const int win = blockIdx.x, bimg = win / (nwy * nwx), wy = (win / nwx) % nwy, wx = win % nwx;
  for (int e = threadIdx.x; e < G::NK * 4; e += blockDim.x) {
    const int j = e >> 2, q = e & 3;
    const long p = key_pixel<OCA, WS>(j, bimg, wy, wx, h, w, shift);
    float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
    if (p >= 0) {
      const float4* row = reinterpret_cast<const float4*>(qkv + p * HAT_QKV + head * HAT_D);
      kv = row[HAT_C / 4 + q];
      vv = row[2 * HAT_C / 4 + q];
    }
    reinterpret_cast<float4*>(&ks[j][0])[q] = kv;
    reinterpret_cast<float4*>(&vs[j][0])[q] = vv;
  }
  for (int e = threadIdx.x; e < G::T; e += blockDim.x) tab[e] = table[(long)e * HAT_HEADS + head];
  __syncthreads();
  const int i = threadIdx.x;
  if (i >= G::NQ) return;
  const long pq = OCA ? query_pixel<WS>(i, bimg, wy, wx, h, w, 0) : query_pixel<WS>(i, bimg, wy, wx, h, w, shift);
  float q[HAT_D];
  const float* qr = qkv + pq * HAT_QKV + head * HAT_D;
#pragma unroll
  for (int d = 0; d < HAT_D; ++d) q[d] = qr[d] * 0.25f;  // q * head_dim ** -0.5
  const bool masked = !OCA && shift > 0;
  float m = -INFINITY, lsum = 0.f, acc[HAT_D];
#pragma unroll
  for (int d = 0; d < HAT_D; ++d) acc[d] = 0.f;
  for (int j = 0; j < G::NK; ++j) {
    float s = dot16(q, ks[j]) + tab[G::bias_row(i, j)];
    if (masked) s += shift_mask<WS>(i, j, wy, wx, h, w, shift);
    if (s > m) {
      const float corr = expf(m - s);
      lsum *= corr;
#pragma unroll
      for (int d = 0; d < HAT_D; ++d) acc[d] *= corr;
      m = s;
    }
    const float p = expf(s - m);
    lsum += p;
#pragma unroll
    for (int d = 0; d < HAT_D; ++d) acc[d] += p * vs[j][d];
  }
  const float inv = 1.f / lsum;
  float* o = out + pq * HAT_C + head * HAT_D;
#pragma unroll
  for (int d = 0; d < HAT_D; ++d) o[d] = acc[d] * inv;
  lse[pq * HAT_HEADS + head] = m + logf(lsum);
}

// Backward, grid (G, heads): block g walks windows g, g + G, ...  Phase 1 (thread = query i): P, dS, dq, and the block's dS sums
// acc[i][j] (row i belongs to thread i: no atomics).  Phase 2 (thread = key j): dv = sum_i P dO_i, dk = sum_i dS q_i.
template <int OCA, int WS>
__global__ __launch_bounds__(192) void hat_attn_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ table,
                                                           const float* __restrict__ out, const float* __restrict__ dout,
                                                           const float* __restrict__ lse, float* __restrict__ dqkv,
                                                           float* __restrict__ slab, float* __restrict__ part, int nwin, int h,
                                                           int w, int shift) {
  using G = AttnGeom<OCA, WS>;
  __shared__ __attribute__((aligned(16))) float qs[G::NQ][HAT_D];
  __shared__ __attribute__((aligned(16))) float dos[G::NQ][HAT_D];
  __shared__ float dd[G::NQ];
  __shared__ __attribute__((aligned(16))) float ks[G::NK][HAT_D];
  __shared__ __attribute__((aligned(16))) float vs[G::NK][HAT_D];
  __shared__ float pm[G::NQ][G::NK];
  __shared__ float acc[G::NQ][G::NK];
  __shared__ float tab[G::T];
  const int head = blockIdx.y, nwx = w / WS, nwy = h / WS;
  const int t = threadIdx.x;
  for (int e = t; e < G::NQ * G::NK; e += blockDim.x) (&acc[0][0])[e] = 0.f;
  for (int e = t; e < G::T; e += blockDim.x) tab[e] = table[(long)e * HAT_HEADS + head];
  const bool masked = !OCA && shift > 0;
  for (int win = blockIdx.x; win < nwin; win += gridDim.x) {
    const int bimg = win / (nwy * nwx), wy = (win / nwx) % nwy, wx = win % nwx;
    __syncthreads();                                   // the previous window's phase 2 is done with ks / vs / pm
    for (int e = t; e < G::NK * 4; e += blockDim.x) {
      const int j = e >> 2, q = e & 3;
      const long p = key_pixel<OCA, WS>(j, bimg, wy, wx, h, w, shift);
      float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
      if (p >= 0) {
        const float4* row = reinterpret_cast<const float4*>(qkv + p * HAT_QKV + head * HAT_D);
        kv = row[HAT_C / 4 + q];
        vv = row[2 * HAT_C / 4 + q];
      }
      reinterpret_cast<float4*>(&ks[j][0])[q] = kv;
      reinterpret_cast<float4*>(&vs[j][0])[q] = vv;
    }
    long pq = 0;
    float l_i = 0.f;
    if (t < G::NQ) {
      pq = OCA ? query_pixel<WS>(t, bimg, wy, wx, h, w, 0) : query_pixel<WS>(t, bimg, wy, wx, h, w, shift);
      const float* qr = qkv + pq * HAT_QKV + head * HAT_D;
      const float* orow = out + pq * HAT_C + head * HAT_D;
      const float* gr = dout + pq * HAT_C + head * HAT_D;
      float di = 0.f;
#pragma unroll
      for (int d = 0; d < HAT_D; ++d) {
        qs[t][d] = qr[d] * 0.25f;
        dos[t][d] = gr[d];
        di += gr[d] * orow[d];
      }
      dd[t] = di;
      l_i = lse[pq * HAT_HEADS + head];
    }
    __syncthreads();
    if (t < G::NQ) {
      float q[HAT_D], g[HAT_D], dq[HAT_D];
#pragma unroll
      for (int d = 0; d < HAT_D; ++d) {
        q[d] = qs[t][d];
        g[d] = dos[t][d];
        dq[d] = 0.f;
      }
      const float di = dd[t];
      for (int j = 0; j < G::NK; ++j) {
        float s = dot16(q, ks[j]) + tab[G::bias_row(t, j)];
        if (masked) s += shift_mask<WS>(t, j, wy, wx, h, w, shift);
        const float p = expf(s - l_i);
        pm[t][j] = p;
        const float ds = p * (dot16(g, vs[j]) - di);
        acc[t][j] += ds;
#pragma unroll
        for (int d = 0; d < HAT_D; ++d) dq[d] += ds * ks[j][d];
      }
      float* o = dqkv + pq * HAT_QKV + head * HAT_D;
#pragma unroll
      for (int d = 0; d < HAT_D; ++d) o[d] = dq[d] * 0.25f;
    }
    __syncthreads();
    if (t < G::NK) {
      float v[HAT_D], dk[HAT_D], dv[HAT_D];
#pragma unroll
      for (int d = 0; d < HAT_D; ++d) {
        v[d] = vs[t][d];
        dk[d] = 0.f;
        dv[d] = 0.f;
      }
      for (int i = 0; i < G::NQ; ++i) {
        const float p = pm[i][t];
        const float ds = p * (dot16(dos[i], v) - dd[i]);
#pragma unroll
        for (int d = 0; d < HAT_D; ++d) {
          dv[d] += p * dos[i][d];
          dk[d] += ds * qs[i][d];
        }
      }
      float* o;
      if (OCA) {
        o = slab + ((long)win * G::NK + t) * 2 * HAT_C + head * HAT_D;
      } else {
        o = dqkv + key_pixel<OCA, WS>(t, bimg, wy, wx, h, w, shift) * HAT_QKV + HAT_C + head * HAT_D;
      }
#pragma unroll
      for (int d = 0; d < HAT_D; ++d) {
        o[d] = dk[d];
        o[HAT_C + d] = dv[d];
      }
    }
  }
  __syncthreads();
  float* pb = part + ((long)head * gridDim.x + blockIdx.x) * G::NQ * G::NK;
  for (int e = t; e < G::NQ * G::NK; e += blockDim.x) pb[e] = (&acc[0][0])[e];
}

// part[head][0][e] = sum_g part[head][g][e], blocks in order (in place: every thread owns its column e)
__global__ __launch_bounds__(256) void hat_attn_part_reduce_kernel(float* __restrict__ part, int nblk, long per_head, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long head = i / per_head, e = i % per_head;
  float* col = part + head * nblk * per_head + e;
  float s = 0.f;
  for (int g = 0; g < nblk; ++g) s += col[(long)g * per_head];
  col[0] = s;
}

// dtable[r][head] = sum over the (i, j) with bias_row(i, j) == r (i, then j ascending) of the reduced part[head][0][i][j]
template <int OCA, int WS>
__global__ __launch_bounds__(64) void hat_attn_table_grad_kernel(const float* __restrict__ part, float* __restrict__ dtable,
                                                                 int nblk) {
  using G = AttnGeom<OCA, WS>;
  const int r = blockIdx.x * 64 + threadIdx.x, head = blockIdx.y;
  if (r >= G::T) return;
  // the one relative offset (dy, dx) that maps to r: raw = r or r - T, raw = a L + b with b in [bmin, bmin + L)
  const int bmin = OCA ? G::C0 - (WS - 1) : 0;
  float s = 0.f;
  for (int cand = 0; cand < 2; ++cand) {
    const int raw = cand ? r - G::T : r;
    int a = (raw - bmin) >= 0 ? (raw - bmin) / G::L : -((bmin - raw + G::L - 1) / G::L);
    const int bb = raw - a * G::L;
    if (a < bmin || a >= bmin + G::L) continue;
    // SA: qy - ky = a - C0; OCA: ky - qy = a - C0
    const int oy = a - G::C0, ox = bb - G::C0;
    for (int qy = 0; qy < WS; ++qy) {
      const int ky = OCA ? qy + oy : qy - oy;
      if (ky < 0 || ky >= G::KW) continue;
      for (int qx = 0; qx < WS; ++qx) {
        const int kx = OCA ? qx + ox : qx - ox;
        if (kx < 0 || kx >= G::KW) continue;
        const long e = (long)(qy * WS + qx) * G::NK + ky * G::KW + kx;
        s += part[(long)head * nblk * G::NQ * G::NK + e];           // block 0's slot holds the sum over the blocks
      }
    }
  }
  dtable[(long)r * HAT_HEADS + head] = s;
}

// OCA: dqkv[p][96 + c] = sum over the windows whose 13 x 13 (12 x 12) region holds pixel p (wy, then wx ascending) of the slab
template <int WS>
__global__ __launch_bounds__(192) void hat_oca_fold_kernel(const float* __restrict__ slab, float* __restrict__ dqkv, int h, int w,
                                                           long pixels) {
  using G = AttnGeom<1, WS>;
  const long p = blockIdx.x;
  if (p >= pixels) return;
  const int c = threadIdx.x;
  const int x = (int)(p % w), y = (int)((p / w) % h), bimg = (int)(p / ((long)w * h));
  const int nwx = w / WS, nwy = h / WS;
  float s = 0.f;
  for (int wy = 0; wy < nwy; ++wy) {
    const int ky = y - wy * WS + G::PAD;
    if (ky < 0 || ky >= G::OWS) continue;
    for (int wx = 0; wx < nwx; ++wx) {
      const int kx = x - wx * WS + G::PAD;
      if (kx < 0 || kx >= G::OWS) continue;
      const long win = ((long)bimg * nwy + wy) * nwx + wx;
      s += slab[(win * G::NK + ky * G::OWS + kx) * 2 * HAT_C + c];
    }
  }
  dqkv[p * HAT_QKV + HAT_C + c] = s;
}

static int attn_blocks(int nwin) { return nwin < HAT_BWD_BLOCKS ? nwin : HAT_BWD_BLOCKS; }

template <int OCA, int WS>
static size_t attn_ws_bytes(int nwin) {
  using G = AttnGeom<OCA, WS>;
  size_t part = (size_t)HAT_HEADS * attn_blocks(nwin) * G::NQ * G::NK * 4;
  size_t slab = OCA ? (size_t)nwin * G::NK * 2 * HAT_C * 4 : 0;
  return ((part + 255) & ~(size_t)255) + slab;
}

template <int OCA, int WS>
static int attn_fwd_launch(const float* qkv, const float* table, float* out, float* lse, int n, int h, int w, int shift,
                           hipStream_t st) {
  const int nwin = n * (h / WS) * (w / WS);
  hat_attn_fwd_kernel<OCA, WS><<<dim3(nwin, HAT_HEADS), 192, 0, st>>>(qkv, table, out, lse, h, w, shift);
  return check_launch("hat_attn_fwd");
}

template <int OCA, int WS>
static int attn_bwd_launch(const float* qkv, const float* table, const float* out, const float* dout, const float* lse, float* dqkv,
                           float* dtable, void* ws, size_t ws_bytes, int n, int h, int w, int shift, hipStream_t st) {
  using G = AttnGeom<OCA, WS>;
  const int nwin = n * (h / WS) * (w / WS), nblk = attn_blocks(nwin);
  const size_t need = attn_ws_bytes<OCA, WS>(nwin);
  if (ws_bytes < need) {
    set_error("hat_attn_bwd: workspace %zu bytes < required %zu", ws_bytes, need);
    return SRHIP_ERR_WORKSPACE;
  }
  float* part = static_cast<float*>(ws);
  const size_t part_bytes = ((size_t)HAT_HEADS * nblk * G::NQ * G::NK * 4 + 255) & ~(size_t)255;
  float* slab = OCA ? reinterpret_cast<float*>(static_cast<char*>(ws) + part_bytes) : nullptr;
  hat_attn_bwd_kernel<OCA, WS><<<dim3(nblk, HAT_HEADS), 192, 0, st>>>(qkv, table, out, dout, lse, dqkv, slab, part, nwin, h, w,
                                                                      shift);
  int rc = check_launch("hat_attn_bwd");
  if (rc) return rc;
  const long per_head = (long)G::NQ * G::NK;
  hat_attn_part_reduce_kernel<<<cdiv(HAT_HEADS * per_head, 256), 256, 0, st>>>(part, nblk, per_head, HAT_HEADS * per_head);
  rc = check_launch("hat_attn_part_reduce");
  if (rc) return rc;
  hat_attn_table_grad_kernel<OCA, WS><<<dim3(cdiv(G::T, 64), HAT_HEADS), 64, 0, st>>>(part, dtable, nblk);
  rc = check_launch("hat_attn_table_grad");
  if (rc || !OCA) return rc;
  const long pixels = (long)n * h * w;
  hat_oca_fold_kernel<WS><<<(unsigned)pixels, 2 * HAT_C, 0, st>>>(slab, dqkv, h, w, pixels);
  return check_launch("hat_oca_fold");
}

// ---------------------------------------------------------------------------------------------------------------------------- //
// Channel attention of CAB (C <= 128, hidden <= 16, with biases) and HAB's combine
// ---------------------------------------------------------------------------------------------------------------------------- //

// per image: sum over the pixels of a[p,c] (PROD: a[p,c] b[p,c]) by 8 pixel lanes x C/4 channel quads, lanes combined in order
template <bool PROD, int MAXC>
__device__ void chan_sum(const float* __restrict__ a, const float* __restrict__ b, long hw, int c, float* __restrict__ out,
                         float4 (*red)[MAXC / 4]) {
  const int cq = c / 4, q = threadIdx.x % cq, r = threadIdx.x / cq;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (r < 8) {
    const float4* av = reinterpret_cast<const float4*>(a) + (long)blockIdx.x * hw * cq + q;
    const float4* bv = PROD ? reinterpret_cast<const float4*>(b) + (long)blockIdx.x * hw * cq + q : nullptr;
    for (long p = r; p < hw; p += 8) {
      float4 v = av[p * cq];
      if (PROD) {
        const float4 u = bv[p * cq];
        v.x *= u.x; v.y *= u.y; v.z *= u.z; v.w *= u.w;
      }
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    red[r][q] = acc;
  }
  __syncthreads();
  if (threadIdx.x < c) {
    const int ch = threadIdx.x, qq = ch / 4, cc = ch % 4;
    float s = 0.f;
    for (int k = 0; k < 8; ++k) {
      const float4 t = red[k][qq];
      s += cc == 0 ? t.x : (cc == 1 ? t.y : (cc == 2 ? t.z : t.w));
    }
    out[ch] = s;
  }
  __syncthreads();
}

// one block per image: m = mean_hw u, z = relu(w1 m + b1), s = sigmoid(w2 z + b2); mz[b] = [m (c) | z (hid)]
// (MAXC 128: 256 threads; MAXC 192: 384 threads, so that every channel quad has its 8 pixel lanes)
template <int MAXC>
__global__ __launch_bounds__(2 * MAXC) void hat_ca_fwd_kernel(const float* __restrict__ u, const float* __restrict__ w1,
                                                              const float* __restrict__ b1, const float* __restrict__ w2,
                                                              const float* __restrict__ b2, float* __restrict__ s,
                                                              float* __restrict__ mz, long hw, int c, int hid) {
  __shared__ float4 red[8][MAXC / 4];
  __shared__ float sm[MAXC], sz[HAT_CA_MAXHID];
  const int b = blockIdx.x, t = threadIdx.x;
  chan_sum<false, MAXC>(u, nullptr, hw, c, sm, red);
  if (t < c) {
    sm[t] = sm[t] / (float)hw;
    mz[(long)b * (c + hid) + t] = sm[t];
  }
  __syncthreads();
  if (t < hid) {
    float d = b1 ? b1[t] : 0.f;
    for (int k = 0; k < c; ++k) d += w1[t * c + k] * sm[k];
    const float z = d < 0.f ? 0.f : d;                    // ReLU that lets a NaN through like ATen's (fmaxf would return 0)
    sz[t] = z;
    mz[(long)b * (c + hid) + c + t] = z;
  }
  __syncthreads();
  if (t < c) {
    float l = b2 ? b2[t] : 0.f;
    for (int k = 0; k < hid; ++k) l += w2[t * hid + k] * sz[k];
    s[(long)b * c + t] = 1.f / (1.f + expf(-l));
  }
}

// out = (x + kb[b] a) + cs (s[b,c] u)   (kb NULL: 1; u NULL: no third term)
__global__ __launch_bounds__(256) void hat_combine_fwd_kernel(const float4* __restrict__ x, const float4* __restrict__ a,
                                                              const float* __restrict__ kb, const float4* __restrict__ u,
                                                              const float4* __restrict__ s, float4* __restrict__ out, float cs,
                                                              long quads, long per_image, int cq) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < quads; i += (long)gridDim.x * 256) {
    const long b = i / per_image;
    const float k = kb ? kb[b] : 1.f;
    const float4 xv = x[i], av = a[i];
    float4 o = make_float4(xv.x + k * av.x, xv.y + k * av.y, xv.z + k * av.z, xv.w + k * av.w);
    if (u) {
      const float4 uv = u[i], sv = s[b * cq + (i % cq)];
      o.x += cs * (sv.x * uv.x); o.y += cs * (sv.y * uv.y); o.z += cs * (sv.z * uv.z); o.w += cs * (sv.w * uv.w);
    }
    out[i] = o;
  }
}

// per image: dsig[c] = cs sum_p g u, dl = dsig s (1 - s), dz = [z > 0] w2^T dl, dm = w1^T dz / hw.
// scratch per image: [dl (c) | dz (hid) | dm / hw (c)]
template <int MAXC>
__global__ __launch_bounds__(2 * MAXC) void hat_ca_bwd_kernel(const float* __restrict__ g, const float* __restrict__ u,
                                                              const float* __restrict__ s, const float* __restrict__ mz,
                                                              const float* __restrict__ w1, const float* __restrict__ w2,
                                                              float* __restrict__ scratch, float cs, long hw, int c, int hid) {
  __shared__ float4 red[8][MAXC / 4];
  __shared__ float sd[MAXC], sdl[MAXC], sdz[HAT_CA_MAXHID];
  const int b = blockIdx.x, t = threadIdx.x;
  const int row = 2 * c + hid;
  chan_sum<true, MAXC>(g, u, hw, c, sd, red);
  if (t < c) {
    const float sv = s[(long)b * c + t];
    const float dl = (cs * sd[t]) * sv * (1.f - sv);
    sdl[t] = dl;
    scratch[(long)b * row + t] = dl;
  }
  __syncthreads();
  if (t < hid) {
    float d = 0.f;
    for (int k = 0; k < c; ++k) d += w2[k * hid + t] * sdl[k];
    d = mz[(long)b * (c + hid) + c + t] > 0.f ? d : 0.f;
    sdz[t] = d;
    scratch[(long)b * row + c + t] = d;
  }
  __syncthreads();
  if (t < c) {
    float d = 0.f;
    for (int k = 0; k < hid; ++k) d += w1[k * c + t] * sdz[k];
    scratch[(long)b * row + c + hid + t] = d / (float)hw;
  }
}

// parameter gradients summed over the images in order: dw2[c][k] = sum_b dl z, db2 = sum_b dl, dw1[k][c] = sum_b dz m, db1 = sum_b dz
__global__ __launch_bounds__(256) void hat_ca_wgrad_kernel(const float* __restrict__ scratch, const float* __restrict__ mz,
                                                           float* __restrict__ dw1, float* __restrict__ db1, float* __restrict__ dw2,
                                                           float* __restrict__ db2, int n, int c, int hid) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int row = 2 * c + hid, mrow = c + hid;
  const int n_w2 = c * hid, n_w1 = hid * c;
  if (e >= n_w2 + c + n_w1 + hid) return;
  float acc = 0.f;
  if (e < n_w2) {
    const int ch = e / hid, k = e % hid;
    for (int b = 0; b < n; ++b) acc += scratch[(long)b * row + ch] * mz[(long)b * mrow + c + k];
    if (dw2) dw2[e] = acc;
  } else if (e < n_w2 + c) {
    const int ch = e - n_w2;
    for (int b = 0; b < n; ++b) acc += scratch[(long)b * row + ch];
    if (db2) db2[ch] = acc;
  } else if (e < n_w2 + c + n_w1) {
    const int f = e - n_w2 - c, k = f / c, ch = f % c;
    for (int b = 0; b < n; ++b) acc += scratch[(long)b * row + c + k] * mz[(long)b * mrow + ch];
    if (dw1) dw1[f] = acc;
  } else {
    const int k = e - n_w2 - c - n_w1;
    for (int b = 0; b < n; ++b) acc += scratch[(long)b * row + c + k];
    if (db1) db1[k] = acc;
  }
}

// da = kb[b] g (kb NULL: g);  du = cs s g + dm[b,c] / hw   (du only when it is not NULL)
__global__ __launch_bounds__(256) void hat_combine_bwd_kernel(const float4* __restrict__ g, const float* __restrict__ kb,
                                                              const float4* __restrict__ s, const float* __restrict__ scratch,
                                                              float4* __restrict__ da, float4* __restrict__ du, float cs, long quads,
                                                              long per_image, int cq, int row, int off) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < quads; i += (long)gridDim.x * 256) {
    const long b = i / per_image;
    const float4 gv = g[i];
    if (da) {
      const float k = kb ? kb[b] : 1.f;
      da[i] = make_float4(k * gv.x, k * gv.y, k * gv.z, k * gv.w);
    }
    if (du) {
      const int q = (int)(i % cq);
      const float4 sv = s[b * cq + q];
      const float* dm = scratch + b * row + off + 4 * q;          // [n][row]: not 16-byte aligned in general
      du[i] = make_float4((cs * sv.x) * gv.x + dm[0], (cs * sv.y) * gv.y + dm[1], (cs * sv.z) * gv.z + dm[2],
                          (cs * sv.w) * gv.w + dm[3]);
    }
  }
}

static unsigned ew_grid(long quads) { const long b = (quads + 255) / 256; return (unsigned)(b < 4096 ? b : 4096); }

}  // namespace srhip

using namespace srhip;

static bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

extern "C" {

int srhip_hat_ln_parts(long tokens) { return tokens > 0 ? hat_ln_parts(tokens) : 0; }

int srhip_hat_ln_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, long tokens,
                     void* stream) {
  SRHIP_REQUIRE(x && gamma && beta && y && mean && rstd && tokens > 0, "hat_ln_fwd: bad arguments");
  hat_ln_fwd_kernel<<<(unsigned)((tokens + 3) / 4), 256, 0, as_stream(stream)>>>(x, gamma, beta, y, mean, rstd, tokens);
  return check_launch("hat_ln_fwd");
}

int srhip_hat_ln_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, const float* dadd,
                     float* dx, float* part, float* dgamma, float* dbeta, long tokens, void* stream) {
  SRHIP_REQUIRE(dy && x && gamma && mean && rstd && dx && part && tokens > 0, "hat_ln_bwd: bad arguments");
  const int np = hat_ln_parts(tokens);
  hipStream_t st = as_stream(stream);
  hat_ln_bwd_kernel<<<np, 256, 0, st>>>(dy, x, gamma, mean, rstd, dadd, dx, part, tokens);
  int rc = check_launch("hat_ln_bwd");
  if (rc) return rc;
  hat_sum_rows_kernel<<<2 * HAT_C, 64, 0, st>>>(part, dgamma, dbeta, np, 2 * HAT_C, HAT_C);
  return check_launch("hat_ln_bwd_reduce");
}

int srhip_hat_gelu_fwd(const float* x, float* y, long count, void* stream) {
  SRHIP_REQUIRE(x && y && count > 0 && count % 4 == 0 && aligned16(x) && aligned16(y),
                "hat_gelu_fwd: count % 4 == 0, 16-byte aligned tensors");
  hat_gelu_fwd_kernel<<<ew_grid(count / 4), 256, 0, as_stream(stream)>>>(reinterpret_cast<const float4*>(x),
                                                                         reinterpret_cast<float4*>(y), count / 4);
  return check_launch("hat_gelu_fwd");
}

int srhip_hat_gelu_bwd(const float* dy, const float* x, float* dx, long count, void* stream) {
  SRHIP_REQUIRE(dy && x && dx && count > 0 && count % 4 == 0 && aligned16(dy) && aligned16(x) && aligned16(dx),
                "hat_gelu_bwd: count % 4 == 0, 16-byte aligned tensors");
  hat_gelu_bwd_kernel<<<ew_grid(count / 4), 256, 0, as_stream(stream)>>>(
      reinterpret_cast<const float4*>(dy), reinterpret_cast<const float4*>(x), reinterpret_cast<float4*>(dx), count / 4);
  return check_launch("hat_gelu_bwd");
}

static int attn_check(const char* who, int kind, int n, int h, int w, int ws, int shift) {
  SRHIP_REQUIRE(kind == 0 || kind == 1, "%s: kind 0 (SA) or 1 (OCA)", who);
  SRHIP_REQUIRE(ws == 8 || ws == 9, "%s: window 8 or 9, got %d", who, ws);
  SRHIP_REQUIRE(n > 0 && h > 0 && w > 0 && h % ws == 0 && w % ws == 0, "%s: %d images of %d x %d are not multiples of the window %d",
                who, n, h, w, ws);
  SRHIP_REQUIRE(shift == 0 || (kind == 0 && shift == ws / 2), "%s: shift 0 or ws / 2 (SA only), got %d", who, shift);
  SRHIP_REQUIRE((long)n * (h / ws) * (w / ws) < (1L << 31), "%s: too many windows", who);
  return SRHIP_OK;
}

int srhip_hat_attn_fwd(const float* qkv, const float* table, float* out, float* lse, int kind, int n, int h, int w, int ws, int shift,
                       void* stream) {
  SRHIP_REQUIRE(qkv && table && out && lse && aligned16(qkv), "hat_attn_fwd: bad arguments");
  int rc = attn_check("hat_attn_fwd", kind, n, h, w, ws, shift);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  if (kind == 0) return ws == 9 ? attn_fwd_launch<0, 9>(qkv, table, out, lse, n, h, w, shift, st)
                                : attn_fwd_launch<0, 8>(qkv, table, out, lse, n, h, w, shift, st);
  return ws == 9 ? attn_fwd_launch<1, 9>(qkv, table, out, lse, n, h, w, 0, st)
                 : attn_fwd_launch<1, 8>(qkv, table, out, lse, n, h, w, 0, st);
}

size_t srhip_hat_attn_bwd_workspace(int kind, int n, int h, int w, int ws) {
  if ((kind != 0 && kind != 1) || (ws != 8 && ws != 9) || n <= 0 || h % ws || w % ws) return 0;
  const int nwin = n * (h / ws) * (w / ws);
  if (kind == 0) return ws == 9 ? attn_ws_bytes<0, 9>(nwin) : attn_ws_bytes<0, 8>(nwin);
  return ws == 9 ? attn_ws_bytes<1, 9>(nwin) : attn_ws_bytes<1, 8>(nwin);
}

int srhip_hat_attn_bwd(const float* qkv, const float* table, const float* out, const float* dout, const float* lse, float* dqkv,
                       float* dtable, void* workspace, size_t workspace_bytes, int kind, int n, int h, int w, int ws, int shift,
                       void* stream) {
  SRHIP_REQUIRE(qkv && table && out && dout && lse && dqkv && dtable && aligned16(qkv) && aligned16(workspace),
                "hat_attn_bwd: bad arguments");
  int rc = attn_check("hat_attn_bwd", kind, n, h, w, ws, shift);
  if (rc) return rc;
  if (!workspace) {
    set_error("hat_attn_bwd: workspace is NULL");
    return SRHIP_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  if (kind == 0)
    return ws == 9 ? attn_bwd_launch<0, 9>(qkv, table, out, dout, lse, dqkv, dtable, workspace, workspace_bytes, n, h, w, shift, st)
                   : attn_bwd_launch<0, 8>(qkv, table, out, dout, lse, dqkv, dtable, workspace, workspace_bytes, n, h, w, shift, st);
  return ws == 9 ? attn_bwd_launch<1, 9>(qkv, table, out, dout, lse, dqkv, dtable, workspace, workspace_bytes, n, h, w, 0, st)
                 : attn_bwd_launch<1, 8>(qkv, table, out, dout, lse, dqkv, dtable, workspace, workspace_bytes, n, h, w, 0, st);
}

static int ca_check(const char* who, int n, long hw, int c, int hid) {
  SRHIP_REQUIRE(n > 0 && hw > 0 && c % 4 == 0 && c >= 4 && c <= HAT_CA_MAXC && hid >= 1 && hid <= HAT_CA_MAXHID,
                "%s: C %% 4 == 0, C <= %d, 1 <= hidden <= %d (got %d, %d)", who, HAT_CA_MAXC, HAT_CA_MAXHID, c, hid);
  return SRHIP_OK;
}

// the published widths: 128 < C <= 192
static int ca_wide_check(const char* who, int n, long hw, int c, int hid) {
  SRHIP_REQUIRE(n > 0 && hw > 0 && c % 4 == 0 && c > HAT_CA_MAXC && c <= HAT_CA_WIDE_MAXC && hid >= 1 && hid <= HAT_CA_MAXHID,
                "%s: C %% 4 == 0, %d < C <= %d, 1 <= hidden <= %d (got %d, %d)", who, HAT_CA_MAXC, HAT_CA_WIDE_MAXC, HAT_CA_MAXHID, c,
                hid);
  return SRHIP_OK;
}

int srhip_hat_ca_fwd(const float* u, const float* w1, const float* b1, const float* w2, const float* b2, float* s, float* mz, int n,
                     long hw, int c, int hid, void* stream) {
  SRHIP_REQUIRE(u && w1 && w2 && s && mz && aligned16(u), "hat_ca_fwd: bad arguments");
  int rc = ca_check("hat_ca_fwd", n, hw, c, hid);
  if (rc) return rc;
  hat_ca_fwd_kernel<HAT_CA_MAXC><<<n, 256, 0, as_stream(stream)>>>(u, w1, b1, w2, b2, s, mz, hw, c, hid);
  return check_launch("hat_ca_fwd");
}

int srhip_hat_combine_fwd(const float* x, const float* a, const float* kb, const float* u, const float* s, float* out, float cs, int n,
                          long hw, int c, void* stream) {
  SRHIP_REQUIRE(x && a && out && n > 0 && hw > 0 && c % 4 == 0 && c > 0 && (!u || s), "hat_combine_fwd: bad arguments");
  SRHIP_REQUIRE(aligned16(x) && aligned16(a) && aligned16(out) && (!u || (aligned16(u) && aligned16(s))),
                "hat_combine_fwd: 16-byte aligned tensors");
  const long per = hw * c / 4, quads = per * n;
  hat_combine_fwd_kernel<<<ew_grid(quads), 256, 0, as_stream(stream)>>>(
      reinterpret_cast<const float4*>(x), reinterpret_cast<const float4*>(a), kb, reinterpret_cast<const float4*>(u),
      reinterpret_cast<const float4*>(s), reinterpret_cast<float4*>(out), cs, quads, per, c / 4);
  return check_launch("hat_combine_fwd");
}

size_t srhip_hat_combine_bwd_workspace(int n, int c, int hid) { return (size_t)n * (2 * c + hid) * 4; }

}  // extern "C"

template <bool WIDE>
static int combine_bwd(const float* g, const float* kb, const float* u, const float* s, const float* mz, const float* w1,
                       const float* w2, float* da, float* du, float* dw1, float* db1, float* dw2, float* db2, void* workspace,
                       size_t workspace_bytes, float cs, int n, long hw, int c, int hid, void* stream) {
  const char* who = WIDE ? "hatw_combine_bwd" : "hat_combine_bwd";
  SRHIP_REQUIRE(g && n > 0 && hw > 0 && c % 4 == 0 && c > 0 && aligned16(g) && (!da || aligned16(da)),
                "%s: bad arguments", who);
  hipStream_t st = as_stream(stream);
  const long per = hw * c / 4, quads = per * n;
  if (!du) {
    hat_combine_bwd_kernel<<<ew_grid(quads), 256, 0, st>>>(reinterpret_cast<const float4*>(g), kb, nullptr, nullptr,
                                                           reinterpret_cast<float4*>(da), nullptr, cs, quads, per, c / 4, 0, 0);
    return check_launch(who);
  }
  int rc = WIDE ? ca_wide_check(who, n, hw, c, hid) : ca_check(who, n, hw, c, hid);
  if (rc) return rc;
  SRHIP_REQUIRE(u && s && mz && w1 && w2 && aligned16(u) && aligned16(s) && aligned16(du) && aligned16(workspace),
                "%s: bad channel-attention arguments", who);
  if (!workspace || workspace_bytes < srhip_hat_combine_bwd_workspace(n, c, hid)) {
    set_error("%s: workspace %zu bytes < required %zu", who, workspace_bytes, srhip_hat_combine_bwd_workspace(n, c, hid));
    return SRHIP_ERR_WORKSPACE;
  }
  float* scratch = static_cast<float*>(workspace);
  if (WIDE)
    hat_ca_bwd_kernel<HAT_CA_WIDE_MAXC><<<n, 2 * HAT_CA_WIDE_MAXC, 0, st>>>(g, u, s, mz, w1, w2, scratch, cs, hw, c, hid);
  else
    hat_ca_bwd_kernel<HAT_CA_MAXC><<<n, 256, 0, st>>>(g, u, s, mz, w1, w2, scratch, cs, hw, c, hid);
  rc = check_launch("hat_ca_bwd");
  if (rc) return rc;
  const int nw = 2 * c * hid + c + hid;
  hat_ca_wgrad_kernel<<<cdiv(nw, 256), 256, 0, st>>>(scratch, mz, dw1, db1, dw2, db2, n, c, hid);
  rc = check_launch("hat_ca_wgrad");
  if (rc) return rc;
  hat_combine_bwd_kernel<<<ew_grid(quads), 256, 0, st>>>(reinterpret_cast<const float4*>(g), kb, reinterpret_cast<const float4*>(s),
                                                         scratch, reinterpret_cast<float4*>(da), reinterpret_cast<float4*>(du), cs,
                                                         quads, per, c / 4, 2 * c + hid, c + hid);
  return check_launch(who);
}

extern "C" {

int srhip_hat_combine_bwd(const float* g, const float* kb, const float* u, const float* s, const float* mz, const float* w1,
                          const float* w2, float* da, float* du, float* dw1, float* db1, float* dw2, float* db2, void* workspace,
                          size_t workspace_bytes, float cs, int n, long hw, int c, int hid, void* stream) {
  return combine_bwd<false>(g, kb, u, s, mz, w1, w2, da, du, dw1, db1, dw2, db2, workspace, workspace_bytes, cs, n, hw, c, hid,
                            stream);
}

int srhip_hatw_ca_fwd(const float* u, const float* w1, const float* b1, const float* w2, const float* b2, float* s, float* mz, int n,
                      long hw, int c, int hid, void* stream) {
  SRHIP_REQUIRE(u && w1 && w2 && s && mz && aligned16(u), "hatw_ca_fwd: NULL or misaligned tensor");
  int rc = ca_wide_check("hatw_ca_fwd", n, hw, c, hid);
  if (rc) return rc;
  hat_ca_fwd_kernel<HAT_CA_WIDE_MAXC><<<n, 2 * HAT_CA_WIDE_MAXC, 0, as_stream(stream)>>>(u, w1, b1, w2, b2, s, mz, hw, c, hid);
  return check_launch("hatw_ca_fwd");
}

int srhip_hatw_combine_bwd(const float* g, const float* kb, const float* u, const float* s, const float* mz, const float* w1,
                           const float* w2, float* da, float* du, float* dw1, float* db1, float* dw2, float* db2, void* workspace,
                           size_t workspace_bytes, float cs, int n, long hw, int c, int hid, void* stream) {
  return combine_bwd<true>(g, kb, u, s, mz, w1, w2, da, du, dw1, db1, dw2, db2, workspace, workspace_bytes, cs, n, hw, c, hid,
                           stream);
}

}  // extern "C"
