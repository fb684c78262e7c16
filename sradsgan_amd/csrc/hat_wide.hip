// HAT at its published widths (embed_dim 144 / 180, six heads of 24 / 30 channels, window 16, overlap 0.5): the passes of hat.hip
// whose kernels are tied to C = 96 and windows of 8 / 9, rebuilt with the width as an argument.
//   * LayerNorm over 128 < C <= 192 channels (eps 1e-5): one wave per token, lane l holds channels l, 64 + l and 128 + l; the
//     backward's dgamma / dbeta come from per-block partials folded in a fixed order;
//   * window attention at window 16 for head widths 24 and 30, flash style on the exact-fp32 matrix pipe
//     (v_mfma_f32_32x32x2_f32), the contraction padded to 32 channels in LDS / registers (never in memory):
//       forward   one wave owns 32 queries; keys and values stream through LDS 128 at a time with an online soft-max; the rows'
//                 log-sum-exp is saved;
//       backward  two kernels that rebuild P = exp(S - lse).  The dq kernel walks windows; per chunk of 32 queries its four waves
//                 split the key tiles, leave dS^T of the chunk in LDS ([keys][33]), fold their dq partials in wave order, and
//                 every thread gathers the (query, key) pairs of the bias-table rows it owns from that tile in a fixed order -- no
//                 array with one element per (query, key) pair ever reaches memory.  The dk / dv kernel gives a wave 32 keys and
//                 streams the window's queries through LDS.  OCA's overlapping dk / dv go to per-window slabs that a gather pass
//                 folds per pixel (wy, then wx ascending).
//     q, k and v are read straight from the [tokens, 3C] rows with float2 loads (a head of 30 channels starts 120 bytes into the
//     row); roll, partition, unfold's zero padding and window reverse are address arithmetic; the table is indexed modulo its size;
//     the shift mask adds -100.
// fp32 throughout, whatever the conv arithmetic mode; no atomics: every result is bit-identical from run to run.
#include "common.h"

namespace srhip {
namespace hatw {

constexpr float LN_EPS = 1e-5f;
constexpr int LN_MAXC = 192;
constexpr int WS = 16;             // window
constexpr int NQ = WS * WS;
constexpr int KC = 128;            // keys (queries in the dk / dv kernel: QC) per LDS chunk
constexpr int QC = 64;
constexpr int LDP = 33;            // padded LDS row of 32 channels
constexpr int MAX_HEADS = 6;       // C = heads * D <= 180: the widths the family is built and tested for
constexpr int BWD_BLOCKS = 64;     // dq kernel: most blocks per head (each walks windows g, g + G, ...)

// ---------------------------------------------------------------------------------------------------------------------------- //
// LayerNorm
// ---------------------------------------------------------------------------------------------------------------------------- //

__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                     const float* __restrict__ b, float* __restrict__ y, float* __restrict__ mean,
                                                     float* __restrict__ rstd, long tokens, int c) {
  const long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= tokens) return;
  const int l = threadIdx.x & 63;
  const bool has2 = 128 + l < c;                     // c > 128: channels l and 64 + l always exist
  const float* xr = x + t * c;
  const float x0 = xr[l], x1 = xr[64 + l], x2 = has2 ? xr[128 + l] : 0.f;
  const float mu = wave_sum((x0 + x1) + x2) / (float)c;
  const float d0 = x0 - mu, d1 = x1 - mu, d2 = has2 ? x2 - mu : 0.f;
  const float var = wave_sum((d0 * d0 + d1 * d1) + d2 * d2) / (float)c;
  const float r = 1.f / sqrtf(var + LN_EPS);
  float* yr = y + t * c;
  yr[l] = d0 * r * g[l] + b[l];
  yr[64 + l] = d1 * r * g[64 + l] + b[64 + l];
  if (has2) yr[128 + l] = d2 * r * g[128 + l] + b[128 + l];
  if (l == 0) {
    mean[t] = mu;
    rstd[t] = r;
  }
}

static int ln_parts(long tokens) { const long b = (tokens + 3) / 4; return (int)(b < 512 ? b : 512); }

// dx = r (dy g - mean(dy g) - xhat mean(dy g xhat)) [+ dadd]; part[blk][0..c) = sum dy xhat, part[blk][c..2c) = sum dy
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                     const float* __restrict__ g, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, const float* __restrict__ dadd,
                                                     float* __restrict__ dx, float* __restrict__ part, long tokens, int c) {
  __shared__ float red[4][2 * LN_MAXC];
  const int wv = threadIdx.x >> 6, l = threadIdx.x & 63;
  const bool has2 = 128 + l < c;
  const float g0 = g[l], g1 = g[64 + l], g2 = has2 ? g[128 + l] : 0.f;
  float ag0 = 0.f, ag1 = 0.f, ag2 = 0.f, ab0 = 0.f, ab1 = 0.f, ab2 = 0.f;
  for (long t = (long)blockIdx.x * 4 + wv; t < tokens; t += (long)gridDim.x * 4) {
    const float* xr = x + t * c;
    const float* dr = dy + t * c;
    const float mu = mean[t], r = rstd[t];
    const float h0 = (xr[l] - mu) * r, h1 = (xr[64 + l] - mu) * r, h2 = has2 ? (xr[128 + l] - mu) * r : 0.f;
    const float e0 = dr[l], e1 = dr[64 + l], e2 = has2 ? dr[128 + l] : 0.f;
    const float q0 = e0 * g0, q1 = e1 * g1, q2 = e2 * g2;
    const float c1 = wave_sum((q0 * h0 + q1 * h1) + q2 * h2) / (float)c;
    const float c2 = wave_sum((q0 + q1) + q2) / (float)c;
    float* o = dx + t * c;
    float v0 = r * (q0 - c2 - h0 * c1), v1 = r * (q1 - c2 - h1 * c1), v2 = r * (q2 - c2 - h2 * c1);
    if (dadd) {
      v0 += dadd[t * c + l];
      v1 += dadd[t * c + 64 + l];
      if (has2) v2 += dadd[t * c + 128 + l];
    }
    o[l] = v0;
    o[64 + l] = v1;
    if (has2) o[128 + l] = v2;
    ag0 += e0 * h0;
    ag1 += e1 * h1;
    ag2 += e2 * h2;
    ab0 += e0;
    ab1 += e1;
    ab2 += e2;
  }
  red[wv][l] = ag0;
  red[wv][64 + l] = ag1;
  red[wv][c + l] = ab0;
  red[wv][c + 64 + l] = ab1;
  if (has2) {
    red[wv][128 + l] = ag2;
    red[wv][c + 128 + l] = ab2;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < 2 * c; k += 256)
    part[(size_t)blockIdx.x * 2 * c + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
}

// out[col] = sum over the nparts rows of part[.][col]: one wave per column, lane l walks rows l, l + 64, ... in order, then the
// wave's fixed butterfly (columns below `split` go to out0, the others to out1; a NULL destination is not written)
__global__ __launch_bounds__(64) void sum_rows_kernel(const float* __restrict__ part, float* __restrict__ out0,
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
// Window attention, window 16
// ---------------------------------------------------------------------------------------------------------------------------- //

template <int OCA>
struct Geom {
  static constexpr int OWS = WS + WS / 2;                // 24
  static constexpr int PAD = (OWS - WS) / 2;             // nn.Unfold padding 4
  static constexpr int KW = OCA ? OWS : WS;              // keys per row of the key window
  static constexpr int NK = KW * KW;                     // 576 / 256: multiples of 32
  static constexpr int L = OCA ? WS + OWS - 1 : 2 * WS - 1;
  static constexpr int T = L * L;                        // bias table rows: 1521 / 961
  static constexpr int C0 = OCA ? WS - OWS + 1 : WS - 1; // offset of the relative coordinate
  static constexpr int BMIN = OCA ? C0 - (WS - 1) : 0;   // smallest value of either factor of the raw index
  static constexpr int NR = (T + 255) / 256;             // table rows a thread of the dq kernel owns

  // table row of (query i, key j); the reference's table[rpi.view(-1)] wraps negative OCA indices
  __device__ static int bias_row(int i, int j) {
    const int qy = i / WS, qx = i % WS, ky = j / KW, kx = j % KW;
    const int idx = OCA ? (ky - qy + C0) * L + (kx - qx + C0) : (qy - ky + C0) * L + (qx - kx + C0);
    return idx < 0 ? idx + T : idx;
  }
};

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// row of accumulator register i in lane half hh (column = lane & 31)
__device__ __forceinline__ int acc_row(int i, int hh) { return (i >> 2) * 8 + hh * 4 + (i & 3); }

// region label of a shifted-window coordinate (calculate_mask: slices [0, H - ws), [H - ws, H - shift), [H - shift, H))
__device__ __forceinline__ int mask_label(int r, int n, int shift) { return r < n - WS ? 0 : (r < n - shift ? 1 : 2); }

// pixel (row index in [0, n*h*w)) of key slot j of window (bimg, wy, wx), or -1 for an OCA key in the zero padding
template <int OCA>
__device__ __forceinline__ long key_pixel(int j, int bimg, int wy, int wx, int h, int w, int shift) {
  using G = Geom<OCA>;
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

__device__ __forceinline__ long query_pixel(int i, int bimg, int wy, int wx, int h, int w, int shift) {
  int y = wy * WS + i / WS + shift, x = wx * WS + i % WS + shift;
  if (y >= h) y -= h;
  if (x >= w) x -= w;
  return ((long)bimg * h + y) * w + x;
}

// bias + shift mask of (query i, key j): -100 where the two lie in different regions of a shifted window (SA with shift > 0)
template <int OCA>
__device__ __forceinline__ float bias_mask(const float* tab, int i, int j, int wy, int wx, int h, int w, int shift) {
  float b = tab[Geom<OCA>::bias_row(i, j)];
  if (!OCA && shift > 0) {
    const int li = 3 * mask_label(wy * WS + i / WS, h, shift) + mask_label(wx * WS + i % WS, w, shift);
    const int lj = 3 * mask_label(wy * WS + j / WS, h, shift) + mask_label(wx * WS + j % WS, w, shift);
    if (li != lj) b += -100.f;
  }
  return b;
}

// channels hh * 16 .. hh * 16 + 15 of a head's slice at `p` (d channels, the rest of the 32 reads as 0), times `mul`
__device__ __forceinline__ void load_half(const float* p, int d, int hh, float mul, float (&f)[16]) {
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const int ch = hh * 16 + 2 * m;
    float2 v = make_float2(0.f, 0.f);
    if (p && ch < d) v = *reinterpret_cast<const float2*>(p + ch);
    f[2 * m] = v.x * mul;
    f[2 * m + 1] = v.y * mul;
  }
}

// rows [0, rows) of an LDS tile [rows][LDP]: row j = channels 0..31 of the head's slice at src(j) (NULL: zeros), times `mul`
template <typename F>
__device__ __forceinline__ void stage_rows(float (*dst)[LDP], int rows, int d, float mul, F src) {
  for (int e = threadIdx.x; e < rows * 16; e += blockDim.x) {
    const int j = e >> 4, ch = (e & 15) * 2;
    const float* p = src(j);
    float2 v = make_float2(0.f, 0.f);
    if (p && ch < d) v = *reinterpret_cast<const float2*>(p + ch);
    dst[j][ch] = v.x * mul;
    dst[j][ch + 1] = v.y * mul;
  }
}

// the accumulator tile acc^T[channel][token = lane column] times `mul` to the head's slice at dst (channels < d)
__device__ __forceinline__ void store_tile(const f32x16& acc, float mul, float* dst, int d, int hh) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int ch = g * 8 + hh * 4;
    if (ch < d) *reinterpret_cast<float2*>(dst + ch) = make_float2(acc[4 * g] * mul, acc[4 * g + 1] * mul);
    if (ch + 2 < d) *reinterpret_cast<float2*>(dst + ch + 2) = make_float2(acc[4 * g + 2] * mul, acc[4 * g + 3] * mul);
  }
}

// grid (2 nwin, heads), 4 waves: wave wv owns queries (blockIdx.x & 1) * 128 + wv * 32 .. + 31 of window blockIdx.x / 2
template <int OCA>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const float* __restrict__ qkv, const float* __restrict__ table,
                                                       float* __restrict__ out, float* __restrict__ lse, int h, int w, int shift,
                                                       int c, int heads, int d, float scale) {
  using G = Geom<OCA>;
  __shared__ float ks[KC][LDP];
  __shared__ float vs[KC][LDP];
  __shared__ float tab[G::T];
  const int head = blockIdx.y, nwx = w / WS, nwy = h / WS;
  const int win = blockIdx.x >> 1, bimg = win / (nwy * nwx), wy = (win / nwx) % nwy, wx = win % nwx;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
  const long ld = 3L * c;
  for (int e = threadIdx.x; e < G::T; e += 256) tab[e] = table[(long)e * heads + head];
  const int q = (blockIdx.x & 1) * 128 + wv * 32 + r;
  const long pq = query_pixel(q, bimg, wy, wx, h, w, OCA ? 0 : shift);
  float qf[16];
  load_half(qkv + pq * ld + head * d, d, hh, scale, qf);
  f32x16 o;
#pragma unroll
  for (int i = 0; i < 16; ++i) o[i] = 0.f;
  float m = -INFINITY, l = 0.f;
  for (int kc0 = 0; kc0 < G::NK; kc0 += KC) {
    __syncthreads();                                   // the previous chunk's readers are done (and tab is written)
    const int rows = G::NK - kc0 < KC ? G::NK - kc0 : KC;
    auto ksrc = [&](int j) -> const float* {
      const long p = key_pixel<OCA>(kc0 + j, bimg, wy, wx, h, w, shift);
      return p < 0 ? nullptr : qkv + p * ld + c + head * d;
    };
    auto vsrc = [&](int j) -> const float* {
      const long p = key_pixel<OCA>(kc0 + j, bimg, wy, wx, h, w, shift);
      return p < 0 ? nullptr : qkv + p * ld + 2 * c + head * d;
    };
    stage_rows(ks, rows, d, 1.f, ksrc);
    stage_rows(vs, rows, d, 1.f, vsrc);
    __syncthreads();
    for (int kt = 0; kt * 32 < rows; ++kt) {
      f32x16 s;
#pragma unroll
      for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) s = mfma(ks[kt * 32 + r][hh * 16 + j], qf[j], s);      // S^T[key acc_row(i, hh)][query r]
      float mx = -INFINITY;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        s[i] += bias_mask<OCA>(tab, q, kc0 + kt * 32 + acc_row(i, hh), wy, wx, h, w, shift);
        mx = fmaxf(mx, s[i]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mnew = fmaxf(m, mx);
      const float alpha = expf(m - mnew);                                                  // 0 on the first tile (m = -inf)
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
      for (int i = 0; i < 16; ++i) o[i] *= alpha;
#pragma unroll
      for (int i = 0; i < 16; ++i) o = mfma(vs[kt * 32 + acc_row(i, hh)][r], s[i], o);     // O^T[channel][query r]
    }
  }
  store_tile(o, 1.f / l, out + pq * c + head * d, d, hh);
  if (hh == 0) lse[pq * heads + head] = m + logf(l);
}

// dq, delta and the table-gradient partials.  grid (G, heads), 4 waves: block g walks windows g, g + G, ...; per chunk of 32 queries
// (two window rows) wave wv takes key tile wv of every 128-key chunk.  part[head][g][T]: the block's sums by table row.
template <int OCA>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ table,
                                                          const float* __restrict__ out, const float* __restrict__ dout,
                                                          const float* __restrict__ lse, float* __restrict__ delta,
                                                          float* __restrict__ dqkv, float* __restrict__ part, int nwin, int h, int w,
                                                          int shift, int c, int heads, int d, float scale) {
  using G = Geom<OCA>;
  __shared__ float ks[KC][LDP];                        // between the key loop and the next chunk: the waves' dq partials
  __shared__ float vs[KC][LDP];
  __shared__ float dst[G::NK][LDP];                    // dS^T of the query chunk (rows padded: the table gather walks keys)
  __shared__ float tab[G::T];
  float (*red)[32][LDP] = reinterpret_cast<float (*)[32][LDP]>(&ks[0][0]);
  const int head = blockIdx.y, nwx = w / WS, nwy = h / WS;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, r = lane & 31, hh = lane >> 5;
  const long ld = 3L * c;
  for (int e = t; e < G::T; e += 256) tab[e] = table[(long)e * heads + head];
  // the one relative offset (oy, ox) that maps to each owned row: raw = row or row - T, raw = a L + b with a, b in [BMIN, BMIN + L)
  int oy[G::NR], ox[G::NR];
  float tacc[G::NR];
#pragma unroll
  for (int m = 0; m < G::NR; ++m) {
    const int row = t + 256 * m;
    tacc[m] = 0.f;
    oy[m] = 1000;                                      // no pair matches
    ox[m] = 0;
    if (row < G::T) {
#pragma unroll
      for (int cand = 0; cand < 2; ++cand) {
        const int raw = cand ? row - G::T : row;
        const int a = (raw - G::BMIN) >= 0 ? (raw - G::BMIN) / G::L : -((G::BMIN - raw + G::L - 1) / G::L);
        const int b = raw - a * G::L;
        if (a >= G::BMIN && a < G::BMIN + G::L && b >= G::BMIN && b < G::BMIN + G::L) {
          oy[m] = a - G::C0;
          ox[m] = b - G::C0;
        }
      }
    }
  }
  for (int win = blockIdx.x; win < nwin; win += gridDim.x) {
    const int bimg = win / (nwy * nwx), wy = (win / nwx) % nwy, wx = win % nwx;
    for (int qc = 0; qc < NQ / 32; ++qc) {
      const int q = qc * 32 + r;
      const long pq = query_pixel(q, bimg, wy, wx, h, w, OCA ? 0 : shift);
      float qf[16], dof[16];
      load_half(qkv + pq * ld + head * d, d, hh, scale, qf);
      load_half(dout + pq * c + head * d, d, hh, 1.f, dof);
      float dl = 0.f;
      {
        float of[16];
        load_half(out + pq * c + head * d, d, hh, 1.f, of);
#pragma unroll
        for (int j = 0; j < 16; ++j) dl += dof[j] * of[j];
        dl += __shfl_xor(dl, 32, 64);
      }
      const float ls = lse[pq * heads + head];
      if (wv == 0 && hh == 0) delta[pq * heads + head] = dl;
      f32x16 dq;
#pragma unroll
      for (int i = 0; i < 16; ++i) dq[i] = 0.f;
      for (int kc0 = 0; kc0 < G::NK; kc0 += KC) {
        __syncthreads();                               // ks / vs / dst / red of the previous round are read
        const int rows = G::NK - kc0 < KC ? G::NK - kc0 : KC;
        auto ksrc = [&](int j) -> const float* {
          const long p = key_pixel<OCA>(kc0 + j, bimg, wy, wx, h, w, shift);
          return p < 0 ? nullptr : qkv + p * ld + c + head * d;
        };
        auto vsrc = [&](int j) -> const float* {
          const long p = key_pixel<OCA>(kc0 + j, bimg, wy, wx, h, w, shift);
          return p < 0 ? nullptr : qkv + p * ld + 2 * c + head * d;
        };
        stage_rows(ks, rows, d, 1.f, ksrc);
        stage_rows(vs, rows, d, 1.f, vsrc);
        __syncthreads();
        if (wv * 32 < rows) {
          const int k0 = wv * 32;
          f32x16 s, dp;
#pragma unroll
          for (int i = 0; i < 16; ++i) s[i] = 0.f, dp[i] = 0.f;
#pragma unroll
          for (int j = 0; j < 16; ++j) s = mfma(ks[k0 + r][hh * 16 + j], qf[j], s);       // S^T[key][query]
#pragma unroll
          for (int j = 0; j < 16; ++j) dp = mfma(vs[k0 + r][hh * 16 + j], dof[j], dp);    // dP^T[key][query]
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int key = kc0 + k0 + acc_row(i, hh);
            const float pr = expf(s[i] + bias_mask<OCA>(tab, q, key, wy, wx, h, w, shift) - ls);
            s[i] = pr * (dp[i] - dl);                                                      // dS^T
            dst[key][r] = s[i];
          }
#pragma unroll
          for (int i = 0; i < 16; ++i) dq = mfma(ks[k0 + acc_row(i, hh)][r], s[i], dq);   // dQ^T[channel][query] += K^T dS^T
        }
      }
      __syncthreads();                                 // dst is complete, ks is free
#pragma unroll
      for (int i = 0; i < 16; ++i) red[wv][acc_row(i, hh)][r] = dq[i];
      __syncthreads();
      for (int e = t; e < 32 * 32; e += 256) {
        const int ch = e & 31, qq = e >> 5;
        if (ch < d) {
          const long p = query_pixel(qc * 32 + qq, bimg, wy, wx, h, w, OCA ? 0 : shift);
          dqkv[p * ld + head * d + ch] = ((red[0][ch][qq] + red[1][ch][qq]) + (red[2][ch][qq] + red[3][ch][qq])) * scale;
        }
      }
      // the owned table rows: pairs (query of this chunk, key = query + offset), queries ascending
#pragma unroll
      for (int m = 0; m < G::NR; ++m) {
        float a = tacc[m];
        for (int qyl = 0; qyl < 2; ++qyl) {
          const int qy = 2 * qc + qyl;
          const int ky = OCA ? qy + oy[m] : qy - oy[m];
          if (ky < 0 || ky >= G::KW) continue;
          for (int qx = 0; qx < WS; ++qx) {
            const int kx = OCA ? qx + ox[m] : qx - ox[m];
            if (kx < 0 || kx >= G::KW) continue;
            a += dst[ky * G::KW + kx][qyl * WS + qx];
          }
        }
        tacc[m] = a;
      }
    }
  }
  float* pb = part + ((long)head * gridDim.x + blockIdx.x) * G::T;
#pragma unroll
  for (int m = 0; m < G::NR; ++m)
    if (t + 256 * m < G::T) pb[t + 256 * m] = tacc[m];
}

// dtable[row][head] = sum over the dq kernel's blocks, in order, of part[head][g][row]
__global__ __launch_bounds__(256) void table_reduce_kernel(const float* __restrict__ part, float* __restrict__ dtable, int nblk,
                                                           int rows, int heads) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * heads) return;
  const int row = i / heads, head = i % heads;
  const float* col = part + (long)head * nblk * rows + row;
  float s = 0.f;
  for (int g = 0; g < nblk; ++g) s += col[(long)g * rows];
  dtable[i] = s;
}

// dk, dv.  grid (nwin * ceil(NK / 128), heads), 4 waves: wave wv owns keys (blockIdx.x % KB) * 128 + wv * 32 .. + 31 and walks the
// window's queries, 64 at a time through LDS.  SA writes dqkv's k and v parts; OCA writes slab[win][key][2C].
template <int OCA>
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ table,
                                                           const float* __restrict__ dout, const float* __restrict__ lse,
                                                           const float* __restrict__ delta, float* __restrict__ dqkv,
                                                           float* __restrict__ slab, int h, int w, int shift, int c, int heads, int d,
                                                           float scale) {
  using G = Geom<OCA>;
  constexpr int KB = (G::NK + KC - 1) / KC;
  __shared__ float qs[QC][LDP];
  __shared__ float dos[QC][LDP];
  __shared__ float lss[QC], dls[QC];
  __shared__ float tab[G::T];
  const int head = blockIdx.y, nwx = w / WS, nwy = h / WS;
  const int win = blockIdx.x / KB, bimg = win / (nwy * nwx), wy = (win / nwx) % nwy, wx = win % nwx;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, r = lane & 31, hh = lane >> 5;
  const long ld = 3L * c;
  for (int e = t; e < G::T; e += 256) tab[e] = table[(long)e * heads + head];
  const int k0 = (blockIdx.x % KB) * KC + wv * 32;
  const bool live = k0 < G::NK;                        // OCA's last block holds 64 keys
  const int key = k0 + r;
  const long pk = live ? key_pixel<OCA>(key, bimg, wy, wx, h, w, shift) : -1;
  float kf[16], vf[16];
  load_half(pk < 0 ? nullptr : qkv + pk * ld + c + head * d, d, hh, 1.f, kf);
  load_half(pk < 0 ? nullptr : qkv + pk * ld + 2 * c + head * d, d, hh, 1.f, vf);
  f32x16 dk, dv;
#pragma unroll
  for (int i = 0; i < 16; ++i) dk[i] = 0.f, dv[i] = 0.f;
  const int qshift = OCA ? 0 : shift;
  for (int q0 = 0; q0 < NQ; q0 += QC) {
    __syncthreads();                                   // the previous chunk's readers are done
    auto qsrc = [&](int j) -> const float* { return qkv + query_pixel(q0 + j, bimg, wy, wx, h, w, qshift) * ld + head * d; };
    auto dsrc = [&](int j) -> const float* { return dout + query_pixel(q0 + j, bimg, wy, wx, h, w, qshift) * c + head * d; };
    stage_rows(qs, QC, d, scale, qsrc);
    stage_rows(dos, QC, d, 1.f, dsrc);
    if (t < QC) {
      const long p = query_pixel(q0 + t, bimg, wy, wx, h, w, qshift);
      lss[t] = lse[p * heads + head];
      dls[t] = delta[p * heads + head];
    }
    __syncthreads();
    if (live) {
      for (int sub = 0; sub < QC / 32; ++sub) {
        const int b0 = sub * 32;
        f32x16 s, dp;
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = 0.f, dp[i] = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) s = mfma(qs[b0 + r][hh * 16 + j], kf[j], s);         // S[query][key]
#pragma unroll
        for (int j = 0; j < 16; ++j) dp = mfma(dos[b0 + r][hh * 16 + j], vf[j], dp);      // dP[query][key]
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int ql = b0 + acc_row(i, hh);
          const float pr = expf(s[i] + bias_mask<OCA>(tab, q0 + ql, key, wy, wx, h, w, shift) - lss[ql]);
          s[i] = pr;
          dp[i] = pr * (dp[i] - dls[ql]);                                                  // dS
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int ql = b0 + acc_row(i, hh);
          dv = mfma(dos[ql][r], s[i], dv);                                                 // dV^T[channel][key] += dO^T P
          dk = mfma(qs[ql][r], dp[i], dk);                                                 // dK^T[channel][key] += Q^T dS
        }
      }
    }
  }
  if (!live) return;
  float* o;
  if (OCA) {
    o = slab + ((long)win * G::NK + key) * 2 * c + head * d;       // a key in the zero padding: its slab row is never read
  } else {
    o = dqkv + pk * ld + c + head * d;
  }
  store_tile(dk, 1.f, o, d, hh);
  store_tile(dv, 1.f, o + c, d, hh);
}

// OCA: dqkv[p][C + ch] = sum over the windows whose 24 x 24 region holds pixel p (wy, then wx ascending) of the slab; ch < 2C
__global__ __launch_bounds__(384) void oca_fold_kernel(const float* __restrict__ slab, float* __restrict__ dqkv, int h, int w, int c) {
  using G = Geom<1>;
  const long p = blockIdx.x;
  const int x = (int)(p % w), y = (int)((p / w) % h), bimg = (int)(p / ((long)w * h));
  const int nwx = w / WS, nwy = h / WS;
  for (int ch = threadIdx.x; ch < 2 * c; ch += blockDim.x) {
    float s = 0.f;
    for (int wy = 0; wy < nwy; ++wy) {
      const int ky = y - wy * WS + G::PAD;
      if (ky < 0 || ky >= G::OWS) continue;
      for (int wx = 0; wx < nwx; ++wx) {
        const int kx = x - wx * WS + G::PAD;
        if (kx < 0 || kx >= G::OWS) continue;
        const long win = ((long)bimg * nwy + wy) * nwx + wx;
        s += slab[(win * G::NK + ky * G::OWS + kx) * 2 * c + ch];
      }
    }
    dqkv[p * 3 * c + c + ch] = s;
  }
}

static size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
static int bwd_blocks(int nwin) { return nwin < BWD_BLOCKS ? nwin : BWD_BLOCKS; }

// workspace: [part: heads x blocks x T] [delta: tokens x heads] [OCA: slab nwin x 576 x 2C]
static size_t ws_bytes(int kind, long tokens, int nwin, int c, int heads) {
  const size_t rows = kind ? Geom<1>::T : Geom<0>::T;
  size_t b = up256((size_t)heads * bwd_blocks(nwin) * rows * 4) + up256((size_t)tokens * heads * 4);
  if (kind) b += (size_t)nwin * Geom<1>::NK * 2 * c * 4;
  return b;
}

template <int OCA>
static int bwd_launch(const float* qkv, const float* table, const float* out, const float* dout, const float* lse, float* dqkv,
                      float* dtable, void* ws, int n, int h, int w, int shift, int c, int heads, hipStream_t st) {
  using G = Geom<OCA>;
  const int nwin = n * (h / WS) * (w / WS), nblk = bwd_blocks(nwin), d = c / heads;
  const long tokens = (long)n * h * w;
  const float scale = 1.f / sqrtf((float)d);
  float* part = static_cast<float*>(ws);
  float* delta = reinterpret_cast<float*>(static_cast<char*>(ws) + up256((size_t)heads * nblk * G::T * 4));
  float* slab = reinterpret_cast<float*>(reinterpret_cast<char*>(delta) + up256((size_t)tokens * heads * 4));
  attn_bwd_dq_kernel<OCA><<<dim3(nblk, heads), 256, 0, st>>>(qkv, table, out, dout, lse, delta, dqkv, part, nwin, h, w, shift, c,
                                                             heads, d, scale);
  int rc = check_launch("hatw_attn_bwd_dq");
  if (rc) return rc;
  table_reduce_kernel<<<cdiv((long)G::T * heads, 256), 256, 0, st>>>(part, dtable, nblk, G::T, heads);
  rc = check_launch("hatw_attn_table_reduce");
  if (rc) return rc;
  constexpr int KB = (G::NK + KC - 1) / KC;
  attn_bwd_dkv_kernel<OCA><<<dim3(nwin * KB, heads), 256, 0, st>>>(qkv, table, dout, lse, delta, dqkv, OCA ? slab : nullptr, h, w,
                                                                   shift, c, heads, d, scale);
  rc = check_launch("hatw_attn_bwd_dkv");
  if (rc || !OCA) return rc;
  oca_fold_kernel<<<(unsigned)tokens, 384, 0, st>>>(slab, dqkv, h, w, c);
  return check_launch("hatw_oca_fold");
}

}  // namespace hatw
}  // namespace srhip

using namespace srhip;

static bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

static bool ln_width_ok(int c) { return c > 128 && c <= hatw::LN_MAXC && c % 4 == 0; }

extern "C" {

int srhip_hatw_ln_parts(long tokens) { return tokens > 0 ? hatw::ln_parts(tokens) : 0; }

int srhip_hatw_ln_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, long tokens, int c,
                      void* stream) {
  SRHIP_REQUIRE(x && gamma && beta && y && mean && rstd && tokens > 0, "hatw_ln_fwd: bad arguments");
  SRHIP_REQUIRE(ln_width_ok(c), "hatw_ln_fwd: 128 < C <= 192, C %% 4 == 0, got %d", c);
  SRHIP_REQUIRE((tokens + 3) / 4 < (1L << 31), "hatw_ln_fwd: too many tokens");
  hatw::ln_fwd_kernel<<<(unsigned)((tokens + 3) / 4), 256, 0, as_stream(stream)>>>(x, gamma, beta, y, mean, rstd, tokens, c);
  return check_launch("hatw_ln_fwd");
}

int srhip_hatw_ln_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, const float* dadd,
                      float* dx, float* part, float* dgamma, float* dbeta, long tokens, int c, void* stream) {
  SRHIP_REQUIRE(dy && x && gamma && mean && rstd && dx && part && tokens > 0, "hatw_ln_bwd: bad arguments");
  SRHIP_REQUIRE(ln_width_ok(c), "hatw_ln_bwd: 128 < C <= 192, C %% 4 == 0, got %d", c);
  const int np = hatw::ln_parts(tokens);
  hipStream_t st = as_stream(stream);
  hatw::ln_bwd_kernel<<<np, 256, 0, st>>>(dy, x, gamma, mean, rstd, dadd, dx, part, tokens, c);
  int rc = check_launch("hatw_ln_bwd");
  if (rc) return rc;
  hatw::sum_rows_kernel<<<2 * c, 64, 0, st>>>(part, dgamma, dbeta, np, 2 * c, c);
  return check_launch("hatw_ln_bwd_reduce");
}

static int hatw_attn_check(const char* who, int kind, int n, int h, int w, int c, int heads, int ws, int shift) {
  SRHIP_REQUIRE(kind == 0 || kind == 1, "%s: kind 0 (SA) or 1 (OCA)", who);
  SRHIP_REQUIRE(ws == hatw::WS, "%s: window 16, got %d", who, ws);
  SRHIP_REQUIRE(heads > 0 && heads <= hatw::MAX_HEADS && c > 0 && c % heads == 0 && (c / heads == 24 || c / heads == 30),
                "%s: 1 to %d heads of 24 or 30 channels, got C %d / %d heads", who, hatw::MAX_HEADS, c, heads);
  SRHIP_REQUIRE(n > 0 && h > 0 && w > 0 && h % ws == 0 && w % ws == 0, "%s: %d images of %d x %d are not multiples of the window %d",
                who, n, h, w, ws);
  SRHIP_REQUIRE(shift == 0 || (kind == 0 && shift == ws / 2), "%s: shift 0 or ws / 2 (SA only), got %d", who, shift);
  SRHIP_REQUIRE((long)n * h * w < (1L << 31) && (long)n * (h / ws) * (w / ws) * 5 < (1L << 31), "%s: too many windows", who);
  return SRHIP_OK;
}

int srhip_hatw_attn_fwd(const float* qkv, const float* table, float* out, float* lse, int kind, int n, int h, int w, int c, int heads,
                        int ws, int shift, void* stream) {
  SRHIP_REQUIRE(qkv && table && out && lse && aligned16(qkv) && aligned16(out), "hatw_attn_fwd: NULL or misaligned tensor");
  int rc = hatw_attn_check("hatw_attn_fwd", kind, n, h, w, c, heads, ws, shift);
  if (rc) return rc;
  const int nwin = n * (h / ws) * (w / ws), d = c / heads;
  const float scale = 1.f / sqrtf((float)d);
  hipStream_t st = as_stream(stream);
  if (kind == 0)
    hatw::attn_fwd_kernel<0><<<dim3(2 * nwin, heads), 256, 0, st>>>(qkv, table, out, lse, h, w, shift, c, heads, d, scale);
  else
    hatw::attn_fwd_kernel<1><<<dim3(2 * nwin, heads), 256, 0, st>>>(qkv, table, out, lse, h, w, 0, c, heads, d, scale);
  return check_launch("hatw_attn_fwd");
}

size_t srhip_hatw_attn_bwd_workspace(int kind, int n, int h, int w, int c, int heads, int ws) {
  if ((kind != 0 && kind != 1) || ws != hatw::WS || n <= 0 || h <= 0 || w <= 0 || h % ws || w % ws || heads <= 0 ||
      heads > hatw::MAX_HEADS || c <= 0 || c % heads || (c / heads != 24 && c / heads != 30))
    return 0;
  return hatw::ws_bytes(kind, (long)n * h * w, n * (h / ws) * (w / ws), c, heads);
}

int srhip_hatw_attn_bwd(const float* qkv, const float* table, const float* out, const float* dout, const float* lse, float* dqkv,
                        float* dtable, void* workspace, size_t workspace_bytes, int kind, int n, int h, int w, int c, int heads, int ws,
                        int shift, void* stream) {
  SRHIP_REQUIRE(qkv && table && out && dout && lse && dqkv && dtable && aligned16(qkv) && aligned16(out) && aligned16(dout) &&
                    aligned16(dqkv) && aligned16(workspace),
                "hatw_attn_bwd: NULL or misaligned tensor");
  int rc = hatw_attn_check("hatw_attn_bwd", kind, n, h, w, c, heads, ws, shift);
  if (rc) return rc;
  const size_t need = srhip_hatw_attn_bwd_workspace(kind, n, h, w, c, heads, ws);
  if (!workspace || workspace_bytes < need) {
    set_error("hatw_attn_bwd: workspace %zu bytes < required %zu", workspace_bytes, need);
    return SRHIP_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  if (kind == 0) return hatw::bwd_launch<0>(qkv, table, out, dout, lse, dqkv, dtable, workspace, n, h, w, shift, c, heads, st);
  return hatw::bwd_launch<1>(qkv, table, out, dout, lse, dqkv, dtable, workspace, n, h, w, 0, c, heads, st);
}

}  // extern "C"
