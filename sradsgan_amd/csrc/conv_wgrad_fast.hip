// Fast weight-gradient kernels for gfx950 (Cin % 16 == 0, Cout % 4 == 0): three generations of split-K kernels (register-staged,
// LDS-DMA, row-tap), their reduce kernels, the attention tail's scaled 1x1 kernel and the dispatcher.  The kernels also emit the
// bias gradient (column sums of dy) from the tiles they already stage.  Forward / data gradient: conv_fast_fprop.hip.
#include "conv_dev.h"

namespace srhip {

// ================================================================================================ //
// wgrad: dW[co][(tap,ci)] = sum_p dy[p][co] * xwin[p][(tap,ci)], split over pixel ranges.
// Both operands are pixel-major, so the LDS images are k-major ([pixel][channel]) and fragments are
// conflict-free ds_read_b32 of consecutive dwords.  Blocks with tile_n == 0 also emit the column sums
// of their dy tiles (bias gradient partials).
// ================================================================================================ //
struct WgradGeom {
  int N, H, W, C, ldx;       // x
  int Ho, Wo, K, ldy;        // dy
  int KH, KW, stride, pad;
  int P;                     // N*Ho*Wo pixels
  int Ktot;                  // KH*KW*C
  int nsplit, chunks_per_split;
  unsigned x_bytes, dy_bytes;
};

template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256) void fast_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                          float* __restrict__ partial,
                                                          float* __restrict__ bias_partial,
                                                          const float* __restrict__ xrow,
                                                          const float* __restrict__ xchan, WgradGeom g) {
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int LDA = BM + 4, LDB = BN + 4;
  constexpr int AV = (FBK * BM / 4) / 256, BV = (FBK * BN / 4) / 256;   // float4 per thread per chunk
  static_assert(AV >= 1 && BV >= 1, "tile too small");
  constexpr int STAGE = FBK * (LDA + LDB);
  __shared__ __attribute__((aligned(16))) float lds[2 * STAGE];

  const int tid = threadIdx.x;
  const int ntn = (g.Ktot + BN - 1) / BN;
  const int ntm = (g.K + BM - 1) / BM;
  // XCD-aware order: every tile (tile_m, tile_n) of one pixel split runs on the same XCD (blocks b, b+8,
  // b+16, ... share an L2), so a dy / x chunk is fetched from HBM once per split instead of once per tile
  int tile_n, tile_m, split;
  {
    const int tps = ntm * ntn;
    int bid = blockIdx.x;
    if (g.nsplit % 8 == 0) {
      const int j = bid >> 3;
      split = (j / tps) * 8 + (bid & 7);
      bid = j % tps;
    } else {
      split = bid / tps;
      bid -= split * tps;
    }
    tile_n = bid % ntn;
    tile_m = bid / ntn;
  }
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, g.x_bytes, 0x00020000);
  __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dy), 0, g.dy_bytes, 0x00020000);

  const int c_begin = split * g.chunks_per_split;
  const int nchunks_total = (g.P + FBK - 1) / FBK;
  const int c_end = min(c_begin + g.chunks_per_split, nchunks_total);

  // A (dy) thread mapping: idx = tid + 256*j -> pixel row arow = idx / (BM/4), column quad ac
  constexpr int AQ = BM / 4, BQ = BN / 4;
  const int a_row0 = tid / AQ, a_c = tid - a_row0 * AQ;          // rows a_row0 + j*(256/AQ)
  const int b_row0 = tid / BQ, b_c = tid - b_row0 * BQ;          // rows b_row0 + j*(256/BQ)
  const bool a_colok = (m0 + a_c * 4) < g.K;                     // K % 4 == 0 on this path
  // this thread's B columns (a quad of input channels of ONE filter tap; C % 4 == 0)
  const int kcol = n0 + b_c * 4;
  const bool b_colok = kcol < g.Ktot;
  const int tap = kcol / g.C, ci0 = kcol - tap * g.C;
  const int kh = tap / g.KW, kw = tap - kh * g.KW;

  // B (x window) per-row pixel coordinates, advanced incrementally by FBK pixels per chunk
  int bn[BV], bho[BV], bwo[BV];
#pragma unroll
  for (int j = 0; j < BV; ++j) {
    const int p = c_begin * FBK + b_row0 + j * (256 / BQ);
    const int HoWo = g.Ho * g.Wo;
    bn[j] = p / HoWo;
    const int rem = p - bn[j] * HoWo;
    bho[j] = rem / g.Wo;
    bwo[j] = rem - bho[j] * g.Wo;
  }

  float4 ra[AV], rb[BV], rxs[BV];
  float4 bsum = make_float4(0.f, 0.f, 0.f, 0.f);
  const bool xscale = xrow != nullptr || xchan != nullptr;
  auto load_tiles = [&](int kc) {
#pragma unroll
    for (int j = 0; j < AV; ++j) {
      const int p = kc * FBK + a_row0 + j * (256 / AQ);
      const unsigned off = (p < g.P && a_colok) ? ((unsigned)p * g.ldy + m0 + a_c * 4) * 4u : F_OOB;
      ra[j] = bufload4(ry, off);
    }
#pragma unroll
    for (int j = 0; j < BV; ++j) {
      const int hi = bho[j] * g.stride - g.pad + kh, wi = bwo[j] * g.stride - g.pad + kw;
      const bool ok = b_colok && bn[j] < g.N && hi >= 0 && hi < g.H && wi >= 0 && wi < g.W;
      const unsigned off = ok ? ((unsigned)((bn[j] * g.H + hi) * g.W + wi) * g.ldx + ci0) * 4u : F_OOB;
      rb[j] = bufload4(rx, off);
      if (xscale) {
        float4 sc = make_float4(1.f, 1.f, 1.f, 1.f);
        if (ok) {
          if (xchan) sc = *reinterpret_cast<const float4*>(xchan + (size_t)bn[j] * g.C + ci0);
          if (xrow) {
            const float r = xrow[(size_t)(bn[j] * g.H + hi) * g.W + wi];
            sc.x *= r; sc.y *= r; sc.z *= r; sc.w *= r;
          }
        }
        rxs[j] = sc;
      }
      bwo[j] += FBK;
      while (bwo[j] >= g.Wo) {
        bwo[j] -= g.Wo;
        if (++bho[j] == g.Ho) {
          bho[j] = 0;
          ++bn[j];
        }
      }
    }
  };
  auto store_tiles = [&](int stage) {
    float* a = lds + stage * STAGE;
#pragma unroll
    for (int j = 0; j < AV; ++j) {
      *reinterpret_cast<float4*>(a + (a_row0 + j * (256 / AQ)) * LDA + a_c * 4) = ra[j];
      bsum.x += ra[j].x;
      bsum.y += ra[j].y;
      bsum.z += ra[j].z;
      bsum.w += ra[j].w;
    }
    float* b = lds + stage * STAGE + FBK * LDA;
    if (xscale) {
#pragma unroll
      for (int j = 0; j < BV; ++j) {
        rb[j].x *= rxs[j].x;
        rb[j].y *= rxs[j].y;
        rb[j].z *= rxs[j].z;
        rb[j].w *= rxs[j].w;
      }
    }
#pragma unroll
    for (int j = 0; j < BV; ++j) *reinterpret_cast<float4*>(b + (b_row0 + j * (256 / BQ)) * LDB + b_c * 4) = rb[j];
  };

  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave - wm * WN;
  const int khalf = lane >> 5, l31 = lane & 31;
  f32x16 acc[TM][TN];
#pragma unroll
  for (int t = 0; t < TM; ++t)
#pragma unroll
    for (int u = 0; u < TN; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][u][r] = 0.f;

  if (c_begin < c_end) {
    load_tiles(c_begin);
    store_tiles(0);
    __syncthreads();
    for (int kc = c_begin; kc < c_end; ++kc) {
      const int stage = (kc - c_begin) & 1;
      if (kc + 1 < c_end) load_tiles(kc + 1);
      const float* a = lds + stage * STAGE + khalf * LDA + wm * WTM + l31;
      const float* b = lds + stage * STAGE + FBK * LDA + khalf * LDB + wn * WTN + l31;
      float av[2][TM], bv[2][TN];
#pragma unroll
      for (int t = 0; t < TM; ++t) av[0][t] = a[t * 32];
#pragma unroll
      for (int u = 0; u < TN; ++u) bv[0][u] = b[u * 32];
#pragma unroll
      for (int kk = 0; kk < FBK / 2; ++kk) {
        const int cur = kk & 1, nxt = cur ^ 1;
        if (kk + 1 < FBK / 2) {
#pragma unroll
          for (int t = 0; t < TM; ++t) av[nxt][t] = a[(kk + 1) * 2 * LDA + t * 32];
#pragma unroll
          for (int u = 0; u < TN; ++u) bv[nxt][u] = b[(kk + 1) * 2 * LDB + u * 32];
        }
#pragma unroll
        for (int t = 0; t < TM; ++t)
#pragma unroll
          for (int u = 0; u < TN; ++u) acc[t][u] = mfma32f(av[cur][t], bv[cur][u], acc[t][u]);
      }
      if (kc + 1 < c_end) store_tiles(stage ^ 1);
      __syncthreads();
    }
  }

  float* out = partial + (size_t)split * g.K * g.Ktot;
#pragma unroll
  for (int u = 0; u < TN; ++u) {
    const int n = n0 + wn * WTN + u * 32 + l31;
#pragma unroll
    for (int t = 0; t < TM; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * WTM + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
        if (m < g.K && n < g.Ktot) out[(size_t)m * g.Ktot + n] = acc[t][u][r];
      }
  }

  // bias-gradient partial: column sums of every dy tile this block staged (only the tile_n == 0 blocks)
  if (bias_partial != nullptr && tile_n == 0) {
    __syncthreads();
    float* red = lds;                                  // [256/AQ][BM]
    *reinterpret_cast<float4*>(red + a_row0 * BM + a_c * 4) = bsum;
    __syncthreads();
    if (tid < BM && m0 + tid < g.K) {
      float s = 0.f;
#pragma unroll
      for (int rr = 0; rr < 256 / AQ; ++rr) s += red[rr * BM + tid];
      bias_partial[(size_t)split * g.K + m0 + tid] = s;
    }
  }
}

// ---- wgrad, LDS-DMA variant: same ring / counted-vmcnt structure as fast_conv_dma_kernel.  Both
// operands are pixel-major, so a stage is simply [16 pixels][BM] + [16 pixels][BN] floats, written
// lane-linear by the DMA and read back as conflict-free ds_read_b32 (consecutive dwords) -- no swizzle.
// MATH 1 (SRHIP_MATH_BF16X3): a lane gathers its 8 consecutive pixels of one channel with 8 ds_read_b32 (still
// consecutive dwords across lanes), splits them into bf16 hi/lo and issues three 32x32x16 MFMAs per tile pair.
// 16 zero bytes: the source of fast_wgrad_dma_kernel's LDS-DMA for padding and out-of-range pixels
__device__ __attribute__((aligned(16))) float g_zero16[4] = {0.f, 0.f, 0.f, 0.f};
template <int BM, int BN, int WM, int WN, int WBK, int MATH>
__global__ __launch_bounds__(256) void fast_wgrad_dma_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                              float* __restrict__ partial,
                                                              float* __restrict__ bias_partial, WgradGeom g) {
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int AI = BM * WBK / 1024, BI = BN * WBK / 1024;   // DMA instructions per wave per chunk
  constexpr int ALR = BM / 4, BLR = BN / 4;              // lanes per pixel row
  constexpr int ARPI = 64 / ALR, BRPI = 64 / BLR;        // pixel rows per DMA instruction
  constexpr int STAGE_B = (BM + BN) * WBK * 4;
  __shared__ __attribute__((aligned(1024))) char lds[3 * STAGE_B];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: keeps per-wave control flow on the scalar unit
  const int ntn = (g.Ktot + BN - 1) / BN;
  const int ntm = (g.K + BM - 1) / BM;
  // XCD-aware order: every tile (tile_m, tile_n) of one pixel split runs on the same XCD (blocks b, b+8,
  // b+16, ... share an L2), so a dy / x chunk is fetched from HBM once per split instead of once per tile
  int tile_n, tile_m, split;
  {
    const int tps = ntm * ntn;
    int bid = blockIdx.x;
    if (g.nsplit % 8 == 0) {
      const int j = bid >> 3;
      split = (j / tps) * 8 + (bid & 7);
      bid = j % tps;
    } else {
      split = bid / tps;
      bid -= split * tps;
    }
    tile_n = bid % ntn;
    tile_m = bid / ntn;
  }
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) char*)lds;

  const int c_begin = split * g.chunks_per_split;
  const int nchunks_total = (g.P + WBK - 1) / WBK;
  const int c_end = min(c_begin + g.chunks_per_split, nchunks_total);
  const int nk = c_end - c_begin;

  // A (dy): this lane feeds pixel row arow[i], channels m0 + acol*4 ..
  const int acol = lane % ALR;
  const bool a_colok = (m0 + acol * 4) < g.K;
  int arow[AI];
#pragma unroll
  for (int i = 0; i < AI; ++i) arow[i] = (wave * AI + i) * ARPI + lane / ALR;
  // B (x window): pixel row brow[j], columns kcol..kcol+3 of ONE tap
  const int bcolq = lane % BLR;
  const int kcol = n0 + bcolq * 4;
  const bool b_colok = kcol < g.Ktot;
  const int tap = kcol / g.C, ci0 = kcol - tap * g.C;
  const int kh = tap / g.KW, kw = tap - kh * g.KW;
  int bn[BI], bho[BI], bwo[BI];
  const int HoWo = g.Ho * g.Wo;
#pragma unroll
  for (int j = 0; j < BI; ++j) {
    const int p = c_begin * WBK + (wave * BI + j) * BRPI + lane / BLR;
    bn[j] = p / HoWo;
    const int rem = p - bn[j] * HoWo;
    bho[j] = rem / g.Wo;
    bwo[j] = rem - bho[j] * g.Wo;
  }
  const unsigned a_dst = __builtin_amdgcn_readfirstlane(lds_base + wave * AI * 1024);
  const unsigned b_dst = __builtin_amdgcn_readfirstlane(lds_base + BM * WBK * 4 + wave * BI * 1024);

  int kc_issue = c_begin;
  auto issue = [&](int stage) {
    const unsigned so = stage * STAGE_B;
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      const int p = kc_issue * WBK + arow[i];
      const float* ptr = (p < g.P && a_colok) ? dy + ((long)p * g.ldy + m0 + acol * 4) : g_zero16;
      lds_dma16(ptr, a_dst + so + i * 1024);
    }
#pragma unroll
    for (int j = 0; j < BI; ++j) {
      const int hi = bho[j] * g.stride - g.pad + kh, wi = bwo[j] * g.stride - g.pad + kw;
      const bool ok = b_colok && bn[j] < g.N && hi >= 0 && hi < g.H && wi >= 0 && wi < g.W;
      const float* ptr = ok ? x + ((long)((bn[j] * g.H + hi) * g.W + wi) * g.ldx + ci0) : g_zero16;
      lds_dma16(ptr, b_dst + so + j * 1024);
      bwo[j] += WBK;
      while (bwo[j] >= g.Wo) {
        bwo[j] -= g.Wo;
        if (++bho[j] == g.Ho) {
          bho[j] = 0;
          ++bn[j];
        }
      }
    }
    ++kc_issue;
  };

  const int wm = wave / WN, wn = wave - wm * WN;
  const int khalf = lane >> 5, l31 = lane & 31;
  f32x16 acc[TM][TN];
#pragma unroll
  for (int t = 0; t < TM; ++t)
#pragma unroll
    for (int u = 0; u < TN; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][u][r] = 0.f;
  float bsum = 0.f;
  const bool want_bias = bias_partial != nullptr && tile_n == 0 && tid < BM;

  if (nk > 0) {
    issue(0);
    if (nk > 1) issue(1);
    int stage = 0, nstage = 2;
    for (int kc = 0; kc < nk; ++kc) {
      if (kc + 1 < nk)
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(AI + BI) : "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (kc + 2 < nk) issue(nstage);
      const float* a = reinterpret_cast<const float*>(lds + stage * STAGE_B) + khalf * BM + wm * WTM + l31;
      const float* b = reinterpret_cast<const float*>(lds + stage * STAGE_B) + WBK * BM + khalf * BN + wn * WTN + l31;
      if (MATH == 0) {
#pragma unroll
        for (int kk = 0; kk < WBK / 2; ++kk) {
          float av[TM], bv[TN];
#pragma unroll
          for (int t = 0; t < TM; ++t) av[t] = a[kk * 2 * BM + t * 32];
#pragma unroll
          for (int u = 0; u < TN; ++u) bv[u] = b[kk * 2 * BN + u * 32];
#pragma unroll
          for (int t = 0; t < TM; ++t)
#pragma unroll
            for (int u = 0; u < TN; ++u) acc[t][u] = mfma32f(av[t], bv[u], acc[t][u]);
        }
      } else {
        // pixel rows khalf*8 .. khalf*8+7 of each 16-pixel step (a/b above start at row khalf: rebase to khalf*8)
        const float* a8 = a + 7 * khalf * BM;
        const float* b8 = b + 7 * khalf * BN;
        constexpr bool SPLIT = MATH == 1;               // MATH 2: one bf16 product (SRHIP_MATH_HALF)
#pragma unroll
        for (int ks = 0; ks < WBK / 16; ++ks) {
          bf16x8_t ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
          for (int t = 0; t < TM; ++t) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = a8[(ks * 16 + j) * BM + t * 32];
            if (SPLIT) split_bf16x8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), ah[t], al[t]);
            else ah[t] = al[t] = round16x8<1>(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]));
          }
#pragma unroll
          for (int u = 0; u < TN; ++u) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = b8[(ks * 16 + j) * BN + u * 32];
            if (SPLIT) split_bf16x8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), bh[u], bl[u]);
            else bh[u] = bl[u] = round16x8<1>(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]));
          }
          if (SPLIT) {
#pragma unroll
            for (int t = 0; t < TM; ++t)
#pragma unroll
              for (int u = 0; u < TN; ++u) acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[t], bh[u], acc[t][u], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < TM; ++t)
#pragma unroll
              for (int u = 0; u < TN; ++u) acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[t], bl[u], acc[t][u], 0, 0, 0);
          }
#pragma unroll
          for (int t = 0; t < TM; ++t)
#pragma unroll
            for (int u = 0; u < TN; ++u) acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[t], bh[u], acc[t][u], 0, 0, 0);
        }
      }
      if (want_bias) {
        const float* col = reinterpret_cast<const float*>(lds + stage * STAGE_B) + tid;
#pragma unroll
        for (int r = 0; r < WBK; ++r) bsum += col[r * BM];
      }
      stage = stage == 2 ? 0 : stage + 1;
      nstage = nstage == 2 ? 0 : nstage + 1;
    }
  }

  // partial tile -> LDS (wave-private region of the idle ring) -> row-contiguous 16-byte stores
  float* out = partial + (size_t)split * g.K * g.Ktot;
  __syncthreads();
  float* wl = reinterpret_cast<float*>(lds) + wave * (32 * WTN);
  constexpr int QPRW = WTN / 4;
  constexpr int NRD = 32 * QPRW / 64;
#pragma unroll
  for (int t = 0; t < TM; ++t) {
#pragma unroll
    for (int u = 0; u < TN; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) wl[((r & 3) + 8 * (r >> 2) + 4 * khalf) * WTN + u * 32 + l31] = acc[t][u][r];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < NRD; ++i) {
      const int idx = i * 64 + lane;
      const int row = idx / QPRW, cq = idx - row * QPRW;
      const float4 v = *reinterpret_cast<const float4*>(wl + row * WTN + cq * 4);
      const int m = m0 + wm * WTM + t * 32 + row;
      const int n = n0 + wn * WTN + cq * 4;
      if (m < g.K && n < g.Ktot) *reinterpret_cast<float4*>(out + (size_t)m * g.Ktot + n) = v;   // Ktot % 4 == 0
    }
    if (t + 1 < TM) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  if (want_bias && m0 + tid < g.K) bias_partial[(size_t)split * g.K + m0 + tid] = bsum;
}

// ================================================================================================ //
// wgrad of stride-1 pad-1 3x3 convolutions in split-bf16, "row-tap" form.
// fast_wgrad_dma_kernel<.., MATH 1> is VALU-issue bound (14-22 VALU per MFMA: every wave splits every fragment,
// and for Cin = 64 the nine tap tiles each re-fetch and re-split the same dy pixels).  Here
//   * a K chunk is 16 output pixels of ONE image row, so (image, row, first column) are scalars;
//   * a block owns [BM output channels] x [one filter row kh, a slice of 64 input channels, ALL THREE kw]:
//     the three kw taps read the same input row shifted by one pixel, so the x operand is staged once as an
//     18-pixel segment and a lane builds its three B fragments from 10 gathered values (one split, two funnel
//     shifts) instead of 24; the dy operand is fetched and split once for the three taps.
//   18 MFMAs per wave and chunk for ~75 VALU (fast_wgrad_dma_kernel: 6 MFMAs for ~90).
// LDS: 3-slot ring of [16 px][BM] dy + [20 px][64] x (fp32, lane-linear LDS-DMA images); same split-K partial
// layout, reduce kernel and XCD mapping as the other wgrad kernels.
// ================================================================================================ //
// GROUPED launches (round 3): up to 4 weight gradients of the SAME shape in one launch.  The chip wants one full wave of blocks
// (768) whatever the number of convolutions behind it, so G problems run with nsplit / G splits each: the split-K partial
// tiles (the 2 x 76 MB per convolution that made the single launch move 2.5 x its algorithmic bytes), the end-of-kernel
// write burst and the reduce shrink by G, and every block's K loop gets G times longer.  Blocks [p * bpp, (p + 1) * bpp)
// serve problem p (bpp % 8 == 0 keeps a block's XCD = its split lane).
struct WgradBatch {
  const float* x[4];
  const float* dy[4];
  float* partial[4];
  float* bias_partial[4];
  int nprob, bpp;
};

template <int BM, int CIS, bool SPLIT = true>     // SPLIT false: one bf16 product per multiply (SRHIP_MATH_HALF)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void wgrad_rowtap_kernel(
    const float* __restrict__ x_, const float* __restrict__ dy_, float* __restrict__ partial_,
    float* __restrict__ bias_partial_, WgradGeom g, int nseg, int chunks_per_split, int tail_rem, WgradBatch bt) {
  const float* x = x_;
  const float* dy = dy_;
  float* partial = partial_;
  float* bias_partial = bias_partial_;
  int bid0 = blockIdx.x;
  if (bt.nprob > 1) {
    const int prob = __builtin_amdgcn_readfirstlane((int)blockIdx.x / bt.bpp);
    bid0 = (int)blockIdx.x - prob * bt.bpp;
    x = bt.x[prob];
    dy = bt.dy[prob];
    partial = bt.partial[prob];
    bias_partial = bt.bias_partial[prob];
  }
  // tail_rem > 0 ("paired tails", rows of 16 q + tail_rem pixels with tail_rem <= 8): the chunks are enumerated per PAIR of
  // image rows -- q full 16-pixel segments of row A, q of row B, then ONE chunk that holds both rows' tails: MFMA K index
  // k < 8 is pixel 16 q + k of row A, k >= 8 pixel 16 q + (k - 8) of row B (slots past the tail carry dy = 0).  Each half
  // is staged with its own halo (staged rows 0..9 / 10..19), so a lane's gather only swaps the base row of its K half
  // (8 khalf -> 10 khalf).  54-pixel rows: 7 chunks per two rows instead of 8 (an eighth of the MFMAs, DMAs and splits
  // of the 4 x 16 layout fell on padding).
  // tile = BM output channels x (one kh, CIS input channels, three kw); 128 x 64 for wide layers, 64 x 128 for Cout = 64
  constexpr int WM = BM / 64, WN = 4 / WM;          // a wave owns 64 co x (3 kw x 32 ci)
  constexpr int NCI = CIS / WN;
  static_assert((BM == 128 && CIS == 64) || (BM == 64 && CIS == 128), "tile shapes");
  static_assert(NCI == 32, "32 input channels per wave");
  constexpr int TM = 2, TN = 3;                     // TN = kw
  constexpr int A_B = BM * 64;                      // [16 px][BM] fp32
  constexpr int B_B = 20 * CIS * 4;                 // [20 px][CIS] fp32 (18 used)
  constexpr int STAGE_B = A_B + B_B;
  constexpr int NA = A_B / 1024 / 4;                // A pieces per wave
  constexpr int NBT = B_B / 1024;                   // B pieces per chunk, dealt to the waves in order
  constexpr int RPA = 1024 / (BM * 4), RPB = 1024 / (CIS * 4);   // pixel rows per piece
  constexpr int EPI_B = 4 * 32 * 32 * 4;
  constexpr int NSLOT = 3;
  constexpr int LDS_B = NSLOT * STAGE_B > EPI_B ? NSLOT * STAGE_B : EPI_B;
  __shared__ __attribute__((aligned(1024))) char lds[LDS_B];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ncs = g.C / CIS;                        // channel slices of the input
  const int ntn = 3 * ncs;                          // N tiles: (kh, ci slice)
  const int ntm = (g.K + BM - 1) / BM;
  int tile_n, tile_m, split;                        // XCD-aware order, as in fast_wgrad_kernel
  {
    const int tps = ntm * ntn;
    int bid = bid0;
    if (g.nsplit % 8 == 0) {
      const int j = bid >> 3;
      split = (j / tps) * 8 + (bid & 7);
      bid = j % tps;
    } else {
      split = bid / tps;
      bid -= split * tps;
    }
    tile_n = bid % ntn;
    tile_m = bid / ntn;
  }
  const int kh = tile_n / ncs, cs = tile_n - kh * ncs;
  const int m0 = tile_m * BM, ci_base = cs * CIS;
  const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) char*)lds;

  const int q = g.Wo >> 4;                          // full segments per row (paired-tails mode)
  const int cpp = 2 * q + 1;                        // chunks per row pair
  const int rows_total = g.N * g.Ho;
  const int nchunks_total = tail_rem > 0 ? ((rows_total + 1) >> 1) * cpp : g.N * g.Ho * nseg;
  const int c_begin = split * chunks_per_split;
  const int c_end = min(c_begin + chunks_per_split, nchunks_total);
  const int nk = c_end - c_begin;

  // DMA lanes.  A (dy): RPA pixel rows per 1 KiB piece, NA pieces per wave.  B (x): RPB staged pixel rows per piece,
  // NBT pieces dealt to the waves in order (wave-uniform counts nb)
  const int a_col = lane % (BM / 4), a_rsub = lane / (BM / 4);
  const bool a_colok = (m0 + a_col * 4) < g.K;
  const int b_col = lane % (CIS / 4), b_rsub = lane / (CIS / 4);
  const int nb = NBT / 4 + (wave < NBT % 4 ? 1 : 0);
  const int b_first = wave * (NBT / 4) + (wave < NBT % 4 ? wave : NBT % 4);
  const unsigned a_dst = __builtin_amdgcn_readfirstlane(lds_base + wave * NA * 1024);
  const unsigned b_dst = __builtin_amdgcn_readfirstlane(lds_base + A_B + b_first * 1024);

  __amdgpu_buffer_rsrc_t rs_y = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dy), 0, g.dy_bytes, 0x00020000);
  int i_n, i_ho, i_seg;                             // chunk the next issue_s() fetches (scalars); paired tails: (i_n, i_ho) = row A of the pair, i_seg = index inside the pair
  if (tail_rem > 0) {
    i_seg = c_begin % cpp;
    const int r0 = (c_begin / cpp) * 2;
    i_ho = r0 % g.Ho;
    i_n = r0 / g.Ho;
  } else {
    i_seg = c_begin % nseg;
    const int t = c_begin / nseg;
    i_ho = t % g.Ho;
    i_n = t / g.Ho;
  }
  // The DMAs take the chunk's position as the instruction's SCALAR offset (round 4; rounds 1-3 rebuilt every lane's byte offset
  // per chunk: ~90 VALU instructions and 16 branches per chunk and wave in front of the 18 MFMAs).  A lane keeps constant
  // offsets relative to the chunk's first pixel, the chunk's first pixel goes into the buffer instruction's soffset (tensors
  // < 2 GiB, so offset + soffset cannot wrap and a dead lane's 0x80000000 stays out of range whichever way the range check
  // counts soffset), and validity is one compare against a scalar limit.  The x descriptor starts one image row + one pixel
  // BEFORE the tensor so that the halo pixel (-1) of row -1 has offset 0; lanes that would read there are dead lanes.
  const unsigned x_shift = (unsigned)(g.W + 1) * (unsigned)g.ldx * 4u;
  __amdgpu_buffer_rsrc_t rs_xs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x) - (size_t)(g.W + 1) * g.ldx, 0, g.x_bytes + x_shift, 0x00020000);
  unsigned a_full[NA], a_tailv[NA], a_tailA[NA];     // dy: full chunk / tail chunk (both rows live) / tail chunk (row B dead)
  int a_j[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int j = (wave * NA + i) * RPA + a_rsub;
    a_j[i] = j;
    a_full[i] = a_colok ? (unsigned)(j * g.ldy + m0 + a_col * 4) * 4u : F_OOB;
    const int half = j >> 3, jj = j & 7;
    a_tailv[i] = (a_colok && jj < tail_rem) ? (unsigned)((half * g.Wo + jj) * g.ldy + m0 + a_col * 4) * 4u : F_OOB;
    a_tailA[i] = half ? F_OOB : a_tailv[i];
  }
  constexpr int NBI = NBT / 4 + 1;
  unsigned b_full[NBI], b_tailv[NBI];
  int b_r[NBI], b_half[NBI];
#pragma unroll
  for (int i = 0; i < NBI; ++i) {
    const int r = (b_first + i) * RPB + b_rsub;
    b_r[i] = r;
    b_full[i] = r < 18 ? (unsigned)(r * g.ldx + ci_base + b_col * 4) * 4u : F_OOB;
    const int half = r >= 10 ? 1 : 0, ss = r - 10 * half;
    b_half[i] = half;
    const int wo0t = (g.Wo >> 4) * 16;
    const bool okss = r < 20 && ss <= tail_rem && wo0t - 1 + ss >= 0;            // input column wo0 - 1 + ss inside the row
    b_tailv[i] = okss ? (unsigned)((half * g.W + ss) * g.ldx + ci_base + b_col * 4) * 4u : F_OOB;
  }
  int i_row = i_n * g.Ho + i_ho;                    // flat output row (image * Ho + row) of the chunk the next issue fetches (row A of a pair)
  const int rows_all = g.N * g.Ho;
  auto dma_s = [&](unsigned voff, unsigned soff, __amdgpu_buffer_rsrc_t r, unsigned dst) {
    asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %2 offen lds" ::"v"(voff), "s"(r), "s"(soff), "s"(dst) : "memory");
  };
  auto issue_s = [&](int slot) {
    const unsigned adst = a_dst + slot * STAGE_B, bdst = b_dst + slot * STAGE_B;
    if (tail_rem > 0 && i_seg == 2 * q) {           // both rows' tails
      const int wo0 = q * 16;
      const bool liveB = i_row + 1 < rows_all;
      const int hoB = i_ho + 1 < g.Ho ? i_ho + 1 : 0;
      const int hiA = i_ho - 1 + kh, hiB = hoB - 1 + kh;
      const bool okA = hiA >= 0 && hiA < g.H, okB = liveB && hiB >= 0 && hiB < g.H;
      const unsigned sa = (unsigned)(i_row * g.Wo + wo0) * (unsigned)g.ldy * 4u;
      const unsigned sb = (unsigned)((i_row + kh) * g.W + wo0) * (unsigned)g.ldx * 4u;
#pragma unroll
      for (int i = 0; i < NA; ++i) dma_s(liveB ? a_tailv[i] : a_tailA[i], sa, rs_y, adst + i * 1024);
#pragma unroll
      for (int i = 0; i < NBI; ++i)
        if (i < nb) dma_s((b_half[i] ? okB : okA) ? b_tailv[i] : F_OOB, sb, rs_xs, bdst + i * 1024);
      i_seg = 0;
      i_row += 2;
      i_ho += 2;
      if (i_ho >= g.Ho) i_ho -= g.Ho;
      return;
    }
    const int rowB = (tail_rem > 0 && i_seg >= q) ? 1 : 0;
    const int c_row = i_row + rowB;
    int c_ho = i_ho + rowB;
    if (c_ho >= g.Ho) c_ho -= g.Ho;
    const bool rowlive = c_row < rows_all;
    const int wo0 = (rowB ? i_seg - q : i_seg) * 16;
    const int hi = c_ho - 1 + kh;
    const bool rowok = rowlive && hi >= 0 && hi < g.H;
    const unsigned sa = rowlive ? (unsigned)(c_row * g.Wo + wo0) * (unsigned)g.ldy * 4u : 0u;
    const unsigned sb = rowok ? (unsigned)((c_row + kh) * g.W + wo0) * (unsigned)g.ldx * 4u : 0u;
    const int lim_a = rowlive ? g.Wo - wo0 : 0;                       // pixel slots j < lim_a are inside the row
    const int lo_b = rowok ? 1 - wo0 : 64;                            // staged rows lo_b <= r < hi_b are inside the input row
    const int hi_b = g.W + 1 - wo0;
#pragma unroll
    for (int i = 0; i < NA; ++i) dma_s(a_j[i] < lim_a ? a_full[i] : F_OOB, sa, rs_y, adst + i * 1024);
#pragma unroll
    for (int i = 0; i < NBI; ++i)
      if (i < nb) dma_s((b_r[i] >= lo_b && b_r[i] < hi_b) ? b_full[i] : F_OOB, sb, rs_xs, bdst + i * 1024);
    if (tail_rem > 0) {
      ++i_seg;
    } else if (++i_seg == nseg) {
      i_seg = 0;
      ++i_row;
      if (++i_ho == g.Ho) i_ho = 0;
    }
  };
  auto wait_chunk = [&](bool more) {                // this wave's pieces of the oldest chunk in flight have landed
    if (!more) {
      wait_vmcnt<0>();
    } else if (nb == NBT / 4 + 1) {
      wait_vmcnt<NA + NBT / 4 + 1>();
    } else {
      wait_vmcnt<NA + NBT / 4>();
    }
  };

  const int wm = wave / WN, wn = wave - wm * WN;
  const int khalf = lane >> 5, l31 = lane & 31;
  // fragment gather offsets inside a stage (bytes): A value j of tile t = raw A[(8 khalf + j)][wm*64 + t*32 + l31];
  // B value j (0..9) = staged row 8 khalf + j, channel wn*32 + l31
  const int a_off = (8 * khalf) * BM * 4 + (wm * 64 + l31) * 4;
  const int b_off_full = A_B + (8 * khalf) * CIS * 4 + (wn * NCI + l31) * 4;
  const int b_off_tail = A_B + (10 * khalf) * CIS * 4 + (wn * NCI + l31) * 4;
  int c_sub = tail_rem > 0 ? c_begin % cpp : 0;     // compute side: position of the current chunk inside its row pair
  f32x16 acc[TM][TN];
#pragma unroll
  for (int t = 0; t < TM; ++t)
#pragma unroll
    for (int u = 0; u < TN; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][u][r] = 0.f;
  float bsum = 0.f;
  const bool want_bias = bias_partial != nullptr && tile_n == 0 && tid < BM;

  struct Frags {
    bf16x8_t ah[TM], al[TM], bh[TN], bl[TN];
  };
  // raw fp32 stage -> this wave's split fragments of one chunk (+ the bias column sum, taken from the raw dy rows)
  auto convert = [&](int slot, Frags& f) {
    const char* sb = lds + slot * STAGE_B;
    const int b_off = (tail_rem > 0 && c_sub == 2 * q) ? b_off_tail : b_off_full;
    if (tail_rem > 0) c_sub = c_sub == 2 * q ? 0 : c_sub + 1;
    // A fragments: gather 8 pixels, split
#pragma unroll
    for (int t = 0; t < TM; ++t) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const float*>(sb + a_off + j * BM * 4 + t * 128);
      split_bf16x8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), f.ah[t], f.al[t]);
    }
    // B: 10 staged pixels -> packed hi/lo pairs P0..P4 -> the three kw fragments (kw 1 by a 16-bit funnel shift)
    unsigned ph[5], pl[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const float e0 = *reinterpret_cast<const float*>(sb + b_off + (2 * i) * CIS * 4);
      const float e1 = *reinterpret_cast<const float*>(sb + b_off + (2 * i + 1) * CIS * 4);
      typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
      const bf16x2_t h = {(__bf16)e0, (__bf16)e1};
      ph[i] = __builtin_bit_cast(unsigned, h);
      const bf16x2_t l = {(__bf16)(e0 - __uint_as_float(ph[i] << 16)), (__bf16)(e1 - __uint_as_float(ph[i] & 0xffff0000u))};
      pl[i] = __builtin_bit_cast(unsigned, l);
    }
    {
      const u32x4 h0 = {ph[0], ph[1], ph[2], ph[3]}, l0 = {pl[0], pl[1], pl[2], pl[3]};
      const u32x4 h2 = {ph[1], ph[2], ph[3], ph[4]}, l2 = {pl[1], pl[2], pl[3], pl[4]};
      const u32x4 h1 = {__builtin_amdgcn_alignbit(ph[1], ph[0], 16), __builtin_amdgcn_alignbit(ph[2], ph[1], 16),
                        __builtin_amdgcn_alignbit(ph[3], ph[2], 16), __builtin_amdgcn_alignbit(ph[4], ph[3], 16)};
      const u32x4 l1 = {__builtin_amdgcn_alignbit(pl[1], pl[0], 16), __builtin_amdgcn_alignbit(pl[2], pl[1], 16),
                        __builtin_amdgcn_alignbit(pl[3], pl[2], 16), __builtin_amdgcn_alignbit(pl[4], pl[3], 16)};
      f.bh[0] = __builtin_bit_cast(bf16x8_t, h0); f.bl[0] = __builtin_bit_cast(bf16x8_t, l0);
      f.bh[1] = __builtin_bit_cast(bf16x8_t, h1); f.bl[1] = __builtin_bit_cast(bf16x8_t, l1);
      f.bh[2] = __builtin_bit_cast(bf16x8_t, h2); f.bl[2] = __builtin_bit_cast(bf16x8_t, l2);
    }
    if (want_bias) {
      const float* col = reinterpret_cast<const float*>(sb) + tid;
#pragma unroll
      for (int r = 0; r < 16; ++r) bsum += col[r * BM];
    }
  };
  auto mfma_all = [&](const Frags& f) {
#pragma unroll
    for (int i = 0; i < (SPLIT ? 3 : 1) * TM * TN; ++i) {
      const int grp = SPLIT ? i / (TM * TN) : 2, t = (i % (TM * TN)) / TN, u = i % TN;
      acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(grp == 0 ? f.al[t] : f.ah[t], grp == 1 ? f.bl[u] : f.bh[u], acc[t][u], 0, 0, 0);
    }
  };
  if (nk > 0) {
    issue_s(0);
    if (nk > 1) issue_s(1);
    int stage = 0, nstage = 2;
    for (int kc = 0; kc < nk; ++kc) {
      wait_chunk(kc + 1 < nk);
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (kc + 2 < nk) issue_s(nstage);
      Frags f;
      convert(stage, f);
      mfma_all(f);
      stage = stage == 2 ? 0 : stage + 1;
      nstage = nstage == 2 ? 0 : nstage + 1;
    }
  }

  // partial tile -> LDS (wave-private 32x32 region) -> row-contiguous 16-byte stores; sub-tile u is tap (kh, kw = u)
  float* out = partial + (size_t)split * g.K * g.Ktot;
  __syncthreads();
  float* wl = reinterpret_cast<float*>(lds) + wave * (32 * 32);
#pragma unroll
  for (int t = 0; t < TM; ++t) {
#pragma unroll
    for (int u = 0; u < TN; ++u) {
#pragma unroll
      for (int r = 0; r < 16; ++r) wl[((r & 3) + 8 * (r >> 2) + 4 * khalf) * 32 + l31] = acc[t][u][r];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int idx = i * 64 + lane;
        const int row = idx >> 3, cq = idx & 7;
        const float4 v = *reinterpret_cast<const float4*>(wl + row * 32 + cq * 4);
        const int m = m0 + wm * 64 + t * 32 + row;
        const int n = (kh * 3 + u) * g.C + ci_base + wn * NCI + cq * 4;
        if (m < g.K) *reinterpret_cast<float4*>(out + (size_t)m * g.Ktot + n) = v;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
  }
  if (want_bias && m0 + tid < g.K) bias_partial[(size_t)split * g.K + m0 + tid] = bsum;
}

// partial[s][co][(tap,ci)] --sum over s--> dw[co][ci][kh][kw];  bias_partial[s][co] --> db[co]
// 64 outputs per block x SUB split lanes; each lane keeps 4 loads in flight, LDS combines the lanes in a fixed order.
// SUB = 16 for the one- and two-tile GEMMs (1x1 and 64 -> 64 convs: up to 768 splits of a 16 KB tile, only 65 blocks):
// with 4 lanes a thread walked 192 dependent-latency loads (30 us per call, 100 calls per step).
template <int SUB>
__global__ __launch_bounds__(64 * SUB) void fast_wgrad_reduce_kernel(const float* __restrict__ partial,
                                                                     const float* __restrict__ bias_partial,
                                                                     float* __restrict__ dw, float* __restrict__ db,
                                                                     int nsplit, int cout, int cin, int khkw, int ktot,
                                                                     int accumulate) {
  __shared__ float red[64 * SUB];
  const int e = blockIdx.x * 64 + (threadIdx.x & 63), sub = threadIdx.x >> 6;
  const int total = cout * ktot;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (e < total) {
    int i = sub;
    for (; i + 3 * SUB < nsplit; i += 4 * SUB) {
      s0 += partial[(size_t)(i + 0 * SUB) * total + e];
      s1 += partial[(size_t)(i + 1 * SUB) * total + e];
      s2 += partial[(size_t)(i + 2 * SUB) * total + e];
      s3 += partial[(size_t)(i + 3 * SUB) * total + e];
    }
    for (; i < nsplit; i += SUB) s0 += partial[(size_t)i * total + e];
  } else if (db != nullptr && e < total + cout) {
    const int co = e - total;
    for (int i = sub; i < nsplit; i += SUB) s0 += bias_partial[(size_t)i * cout + co];
  }
  red[threadIdx.x] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (sub == 0) {
    const int t = threadIdx.x;
    float v = 0.f;
#pragma unroll
    for (int j = 0; j < SUB; j += 4) v += (red[t + 64 * j] + red[t + 64 * (j + 1)]) + (red[t + 64 * (j + 2)] + red[t + 64 * (j + 3)]);
    if (e < total) {
      const int co = e / ktot, kcol = e - co * ktot;
      const int tap = kcol / cin, ci = kcol - tap * cin;
      float* o = dw + ((size_t)co * cin + ci) * khkw + tap;
      *o = accumulate ? *o + v : v;
    } else if (db != nullptr && e < total + cout) {
      db[e - total] = accumulate ? db[e - total] + v : v;
    }
  }
}

// The same reduction, four consecutive outputs per thread (16-byte loads of the partial rows) and up to four problems of one
// shape per launch (blockIdx.y): round 4.  The summation order of every output element is EXACTLY the scalar kernel's (split lane
// sub sums i = sub, sub + SUB, ... round-robin into four accumulators, (s0 + s1) + (s2 + s3), then the SUB lanes in groups of
// four), so results are bit-identical to it; what changes is the access width (dword loads ran the 38 MB of a RAB conv's
// partials at 3.2 TB/s) and one launch per grouped weight gradient instead of one per convolution.
struct ReduceBatch {
  const float* partial[4];
  const float* bias_partial[4];
  float* dw[4];
  float* db[4];
};
__device__ __forceinline__ float4 add4(const float4& a, const float4& b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
template <int SUB>
__global__ __launch_bounds__(64 * SUB) void fast_wgrad_reduce4_kernel(ReduceBatch rb, int nsplit, int cout, int cin, int khkw,
                                                                      int ktot, int accumulate, int nbias) {   // nbias: rows of bias_partial (= nsplit but for conv_wgrad_flat.hip's flat8 kernel)
  __shared__ float4 red[64 * SUB];
  const int prob = blockIdx.y;
  const float* __restrict__ partial = rb.partial[prob];
  const float* __restrict__ bias_partial = rb.bias_partial[prob];
  float* __restrict__ dw = rb.dw[prob];
  float* __restrict__ db = rb.db[prob];
  const int e = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4, sub = threadIdx.x >> 6;
  const int total = cout * ktot;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 s0 = z, s1 = z, s2 = z, s3 = z;
  if (e < total) {
    int i = sub;
    for (; i + 3 * SUB < nsplit; i += 4 * SUB) {
      s0 = add4(s0, *reinterpret_cast<const float4*>(partial + (size_t)(i + 0 * SUB) * total + e));
      s1 = add4(s1, *reinterpret_cast<const float4*>(partial + (size_t)(i + 1 * SUB) * total + e));
      s2 = add4(s2, *reinterpret_cast<const float4*>(partial + (size_t)(i + 2 * SUB) * total + e));
      s3 = add4(s3, *reinterpret_cast<const float4*>(partial + (size_t)(i + 3 * SUB) * total + e));
    }
    for (; i < nsplit; i += SUB) s0 = add4(s0, *reinterpret_cast<const float4*>(partial + (size_t)i * total + e));
  } else if (db != nullptr && e < total + cout) {
    const int co = e - total;
    for (int i = sub; i < nbias; i += SUB) s0 = add4(s0, *reinterpret_cast<const float4*>(bias_partial + (size_t)i * cout + co));
  }
  red[threadIdx.x] = add4(add4(s0, s1), add4(s2, s3));
  __syncthreads();
  if (sub == 0) {
    const int t = threadIdx.x;
    float4 v = z;
#pragma unroll
    for (int j = 0; j < SUB; j += 4) v = add4(v, add4(add4(red[t + 64 * j], red[t + 64 * (j + 1)]), add4(red[t + 64 * (j + 2)], red[t + 64 * (j + 3)])));
    const float vv[4] = {v.x, v.y, v.z, v.w};
    if (e < total) {
      const int co = e / ktot, kcol = e - co * ktot;              // ktot % 4 == 0: the four outputs share co and the tap
      const int tap = kcol / cin, ci = kcol - tap * cin;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float* o = dw + ((size_t)co * cin + ci + j) * khkw + tap;
        *o = accumulate ? *o + vv[j] : vv[j];
      }
    } else if (db != nullptr && e < total + cout) {
#pragma unroll
      for (int j = 0; j < 4; ++j) db[e - total + j] = accumulate ? db[e - total + j] + vv[j] : vv[j];
    }
  }
}
// one launch for nprob problems of one shape; false: the caller takes the scalar kernel (shapes / pointers the 16-byte form cannot serve)
static bool launch_reduce4(int nprob, const float* const* partial, const float* const* bias_partial, float* const* dw, float* const* db,
                           int nsplit, int cout, int cin, int khkw, int ktot, int accumulate, hipStream_t st, int nbias = -1) {
  if (nbias < 0) nbias = nsplit;
  if (g_wgrad_cfg == WGRAD_CFG_SCALAR_REDUCE || nprob < 1 || nprob > 4 || ktot % 4 != 0 || cout % 4 != 0 || cin % 4 != 0) return false;
  ReduceBatch rb;
  bool anydb = false;
  for (int k = 0; k < 4; ++k) {
    const int j = k < nprob ? k : 0;
    rb.partial[k] = partial[j];
    rb.bias_partial[k] = bias_partial ? bias_partial[j] : nullptr;
    rb.dw[k] = dw[j];
    rb.db[k] = db ? db[j] : nullptr;
    if (((uintptr_t)rb.partial[k] | (uintptr_t)rb.bias_partial[k]) & 15) return false;
    anydb = anydb || rb.db[k] != nullptr;
  }
  const long total = (long)cout * ktot + (anydb ? cout : 0);
  route_note(RF_REDUCE, nsplit >= 64 ? 16 : 4, nprob, 0, 0, 0, cdiv(total, 256) * nprob, nsplit);
  if (nsplit >= 64)
    hipLaunchKernelGGL(fast_wgrad_reduce4_kernel<16>, dim3(cdiv(total, 256), nprob), dim3(1024), 0, st, rb, nsplit, cout, cin, khkw, ktot, accumulate, nbias);
  else
    hipLaunchKernelGGL(fast_wgrad_reduce4_kernel<4>, dim3(cdiv(total, 256), nprob), dim3(256), 0, st, rb, nsplit, cout, cin, khkw, ktot, accumulate, nbias);
  return true;
}

bool launch_reduce4_shared(int nprob, const float* const* partial, const float* const* bias_partial, float* const* dw, float* const* db,
                           int nsplit, int cout, int cin, int khkw, int ktot, int accumulate, hipStream_t st, int nbias) {
  return launch_reduce4(nprob, partial, bias_partial, dw, db, nsplit, cout, cin, khkw, ktot, accumulate, st, nbias);   // conv_wgrad_flat.hip
}

// ================================================================================================ //
// Weight + bias gradient of the attention tail's 1x1 conv (64 -> 64) with its operand scales (round 4):
//     dWc[co][ci] = sum_p g[p][co] * (m[p] * s[b(p)][ci] * u[p][ci]),   dbc[co] = sum_p g[p][co]
// The generic register-staged kernel took 24.5 + 7.9 us at B = 32 for 48 MB of operands (48 launches per step).  Here the fp32
// MFMA 32x32x2 does the contraction over PIXELS directly: with K = 2 per instruction a lane holds ONE k value, so both operands
// are read as they lie in memory -- lanes 0-31 take pixel p, lanes 32-63 pixel p + 1, 32 consecutive channels each, no transpose
// and no LDS.  A block owns a pixel range of ONE image (s is factored out and applied once per block), a wave walks pixel pairs
// with four accumulator tiles (co halves x ci halves); the four waves' tiles are summed through LDS in a fixed order and leave as
// one split-K partial for fast_wgrad_reduce4_kernel.  Exact fp32 products like the kernel it replaces.
// ================================================================================================ //
__global__ __launch_bounds__(256) void wgrad_1x1_scaled_kernel(const float* __restrict__ u, const float* __restrict__ gy,
                                                               const float* __restrict__ m, const float* __restrict__ sc,
                                                               float* __restrict__ partial, float* __restrict__ bias_partial, int hw,
                                                               int per, int sp) {
  __shared__ float red[4][64 * 64];
  __shared__ float bred[4][2][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, kh = lane >> 5;
  const int b = blockIdx.x / sp, j = blockIdx.x - b * sp;
  const int p_begin = j * per, p_end = min(p_begin + per, hw);
  const size_t base = (size_t)b * hw;
  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][c][r] = 0.f;
  float bs0 = 0.f, bs1 = 0.f;
  constexpr int UN = 8;                               // pixel pairs per batch; the next batch's loads are issued before this one's MFMAs
  float g0[2][UN], g1[2][UN], x0[2][UN], x1[2][UN], mv[2][UN];
  auto fetch = [&](int set, int pp) {
#pragma unroll
    for (int i = 0; i < UN; ++i) {
      const int p = pp + 8 * i + kh;
      const bool ok = p < p_end;
      const size_t o = (base + (ok ? p : p_begin)) * 64 + l31;
      g0[set][i] = ok ? gy[o] : 0.f;
      g1[set][i] = ok ? gy[o + 32] : 0.f;
      x0[set][i] = ok ? u[o] : 0.f;
      x1[set][i] = ok ? u[o + 32] : 0.f;
      mv[set][i] = ok ? m[base + p] : 0.f;
    }
  };
  auto compute = [&](int set) {
#pragma unroll
    for (int i = 0; i < UN; ++i) {
      bs0 += g0[set][i];
      bs1 += g1[set][i];
      const float a0 = g0[set][i] * mv[set][i], a1 = g1[set][i] * mv[set][i];
      acc[0][0] = mfma32f(a0, x0[set][i], acc[0][0]);
      acc[0][1] = mfma32f(a0, x1[set][i], acc[0][1]);
      acc[1][0] = mfma32f(a1, x0[set][i], acc[1][0]);
      acc[1][1] = mfma32f(a1, x1[set][i], acc[1][1]);
    }
  };
  int pp = p_begin + 2 * wave;
  if (pp < p_end) {
    fetch(0, pp);
    for (;;) {                                        // two batches per trip: the register sets are indexed at compile time
      const int pn = pp + 8 * UN;
      if (pn < p_end) fetch(1, pn);
      compute(0);
      if (pn >= p_end) break;
      const int pn2 = pn + 8 * UN;
      if (pn2 < p_end) fetch(0, pn2);
      compute(1);
      if (pn2 >= p_end) break;
      pp = pn2;
    }
  }
  // this wave's 64 x 64 tile -> LDS [co][ci]; C/D map of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) red[wave][(a * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh) * 64 + c * 32 + l31] = acc[a][c][r];
  bred[wave][kh][l31] = bs0;
  bred[wave][kh][32 + l31] = bs1;
  __syncthreads();
  float* out = partial + (size_t)blockIdx.x * 64 * 64;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int e = i * 256 + tid;                      // co = e / 64, ci = e % 64
    const float v = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
    out[e] = v * sc[b * 64 + (e & 63)];
  }
  if (bias_partial != nullptr && tid < 64)
    bias_partial[(size_t)blockIdx.x * 64 + tid] = ((bred[0][0][tid] + bred[0][1][tid]) + (bred[1][0][tid] + bred[1][1][tid])) +
                                                 ((bred[2][0][tid] + bred[2][1][tid]) + (bred[3][0][tid] + bred[3][1][tid]));
}

// ================================================================================================ //
// host side: choose_wgrad_route says which kernel a call takes, launch_wgrad_main launches it
// ================================================================================================ //
struct FastWgradPlan {
  int bm, bn, bk, nsplit, chunks_per_split;
};
int g_wgrad_cfg = 0;   // srhip_debug_set(1, cfg): a WgradCfg value (conv_dev.h), 0 = the heuristic
// row-tap kernel (wgrad_rowtap_kernel): split-bf16, 3x3 stride 1 pad 1, Cin % 64 == 0, Cout % 4 == 0
static int rowtap_ok(int cin, int cout, int kh, int kw, int stride, int pad) {   // 0: no, 1: 128 x (kh, 64 ci), 2: 64 x (kh, 128 ci)
  if (!(g_conv_math >= 1 && g_wgrad_cfg != WGRAD_CFG_NO_ROWTAP && (g_wgrad_cfg < WGRAD_CFG_REG || g_wgrad_cfg >= WGRAD_CFG_ROWTAP_TARGET) && kh == 3 &&
        kw == 3 && stride == 1 && pad == 1 && cout % 4 == 0))
    return 0;
  if (cout >= 128 && cin % 64 == 0) return 1;
  if (cout == 64 && cin % 128 == 0) return 2;
  return 0;
}

static FastWgradPlan plan_fast_wgrad(long P, int cout, int ktot, int rowtap = 0) {
  FastWgradPlan p;
  p.bm = cout > 64 ? 128 : 64;
  p.bn = (ktot % 128 == 0) ? 128 : 64;            // Ktot = 9*64 tiles exactly by 64, not by 128
  if (g_wgrad_cfg % 10 == WGRAD_CFG_BN64) p.bn = 64;
  if (g_wgrad_cfg % 10 == WGRAD_CFG_BN128) p.bn = 128;
  p.bk = (g_wgrad_cfg == WGRAD_CFG_BK32 || g_wgrad_cfg == WGRAD_CFG_BK32_BN64) ? 32 : FBK;
  if (g_wgrad_cfg == WGRAD_CFG_BK32_BN64) p.bn = 64;
  if (g_wgrad_cfg == WGRAD_CFG_TILE256) {              // 256-wide tiles: 32 MFMAs per wave per chunk for Cout=256 / Cout=64
    if (cout % 256 == 0 && ktot % 64 == 0) { p.bm = 256; p.bn = 64; }
    else if (cout == 64 && ktot % 256 == 0) { p.bm = 64; p.bn = 256; }
  }
  // split-bf16 wgrad is VALU-issue bound (every wave splits the fragments it reads): where Ktot only tiles by 64
  // (Cin = 64), a 256 x 64 tile doubles the MFMAs per split fragment (measured -10 % on 64->256 convs)
  if (g_conv_math >= 1 && g_wgrad_cfg == WGRAD_CFG_AUTO && p.bn == 64 && cout % 256 == 0) p.bm = 256;
  if (rowtap == 1) { p.bm = 128; p.bn = 192; }
  if (rowtap == 2) { p.bm = 64; p.bn = 384; }
  const long tiles = (long)cdiv(cout, p.bm) * cdiv(ktot, p.bn);
  const int nchunks = cdiv(P, p.bk);
  // blocks aimed at: ~2.5 per CU; the row-tap kernel runs 3 per CU and is fastest with exactly one full wave of
  // blocks (768: measured 0.161 -> 0.128 ms on RAB conv1 against 640; 512 and 1024 are both slower)
  const long target = rowtap ? (g_wgrad_cfg >= WGRAD_CFG_ROWTAP_TARGET ? g_wgrad_cfg : 768) : 640;
  long ns = (target + tiles - 1) / tiles;
  const long maxsplit = (nchunks + 15) / 16;          // at least 16 chunks (256 pixels) per split
  if (ns > maxsplit) ns = maxsplit;
  if (ns > (tiles <= 2 ? 768 : 256)) ns = tiles <= 2 ? 768 : 256;   // one- and two-tile GEMMs (1x1, 64 -> 64) still want a full wave of blocks
  if (ns < 1) ns = 1;
  if (ns >= 8) ns = (ns + 7) / 8 * 8;                  // multiples of 8: one split per XCD lane (see kernels)
  p.chunks_per_split = (int)((nchunks + ns - 1) / ns);
  p.nsplit = cdiv(nchunks, p.chunks_per_split);
  if (p.nsplit >= 8 && p.nsplit % 8 != 0) p.nsplit = (p.nsplit + 7) / 8 * 8;   // empty tail splits write zeros
  return p;
}

// splits per image of wgrad_1x1_scaled_kernel (the attention tail's 64 -> 64 1x1 conv): ~one block per CU, >= 64 pixels per block
static int tail1x1_splits_per_image(int n, int hw) {
  int sp = cdiv(256, n);                               // one block per CU: the split-K reduce of a 64 x 64 tile is latency-bound on the split count
  if (sp > cdiv(hw, 64)) sp = cdiv(hw, 64);
  return sp < 1 ? 1 : sp;
}
size_t fast_conv2d_wgrad_workspace(int n, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad) {
  const int ho = (h + 2 * pad - kh) / stride + 1, wo = (w + 2 * pad - kw) / stride + 1;
  const long P = (long)n * ho * wo;
  if (P <= 0) return 0;
  FastWgradPlan p = plan_fast_wgrad(P, cout, kh * kw * cin, rowtap_ok(cin, cout, kh, kw, stride, pad));
  long ns = p.nsplit;
  if (kh == 1 && kw == 1 && cin == 64 && cout == 64 && stride == 1 && pad == 0) {
    const long t = (long)n * tail1x1_splits_per_image(n, h * w);
    if (t > ns) ns = t;
  }
  return (size_t)ns * ((size_t)cout * kh * kw * cin + cout) * sizeof(float);
}
static int multi_nsplit(const FastWgradPlan& p, int nprob) {
  int ns = p.nsplit / nprob;
  ns = ns / 8 * 8;
  return ns < 8 ? 0 : ns;
}

enum class WgradFamily {
  Tail1x1,   // wgrad_1x1_scaled_kernel
  RowTap,    // wgrad_rowtap_kernel<bm, cis, split>, one problem or a group of nprob
  Dma,       // fast_wgrad_dma_kernel<bm, bn, wm, wn, wbk, math>
  Reg,       // fast_wgrad_kernel<bm, bn, wm, wn>: operand scales, or g_wgrad_cfg >= 10
};
struct WgradRoute {
  WgradFamily family = WgradFamily::Reg;
  FastWgradPlan p;            // tile (Dma / Reg) and the split-K plan
  int nsplit = 0, cps = 0;    // splits per problem and chunks per split as the kernel walks them (what WgradGeom carries)
  int rowtap = 0;             // RowTap: 1 = 128 x (kh, 64 ci), 2 = 64 x (kh, 128 ci)
  bool split = true;          // RowTap: split-bf16 (false: one bf16 product, SRHIP_MATH_HALF)
  int nseg = 0, tail_rem = 0; // RowTap: 16-pixel segments per image row, paired-tail remainder (0: none)
  int wbk = 16, math = 0;     // Dma: pixels per K chunk, arithmetic (0 fp32, 1 split-bf16, 2 one bf16 product)
  int sp = 0, per = 0;        // Tail1x1: splits per image, pixels per split
};

// Which kernels a call takes.  g.nsplit / g.chunks_per_split are not read: the launcher fills them from the route.
// nprob = 1: srhip_conv2d_wgrad; 2..4: the grouped row-tap launch (family RowTap, or nsplit == 0 when the geometry cannot share a launch).
static WgradRoute choose_wgrad_route(const WgradGeom& g, int nprob, bool xrow, bool xchan, size_t workspace_bytes) {
  WgradRoute r;
  const bool scaled = xrow || xchan;
  // (an operand-scaled 3x3 would plan without row-tap and may then need more workspace than the query reported)
  r.rowtap = scaled ? 0 : rowtap_ok(g.C, g.K, g.KH, g.KW, g.stride, g.pad);
  r.p = plan_fast_wgrad(g.P, g.K, g.Ktot, r.rowtap);
  r.nsplit = nprob > 1 ? multi_nsplit(r.p, nprob) : r.p.nsplit;
  r.cps = r.p.chunks_per_split;
  // the attention tail's 1x1 conv with both operand scales: pixel-contraction kernel (workspace permitting)
  if (xrow && xchan && g.KH == 1 && g.KW == 1 && g.C == 64 && g.K == 64 && g.stride == 1 && g.pad == 0 && g.ldx == 64 && g.ldy == 64 &&
      g_wgrad_cfg != WGRAD_CFG_SCALAR_REDUCE && g_wgrad_cfg != WGRAD_CFG_SCALAR_REDUCE_GENERIC && g.N >= 1 &&
      workspace_bytes >= (size_t)g.N * tail1x1_splits_per_image(g.N, g.H * g.W) * ((size_t)g.K * g.Ktot + g.K) * sizeof(float)) {
    r.family = WgradFamily::Tail1x1;
    r.sp = tail1x1_splits_per_image(g.N, g.H * g.W);
    r.per = (cdiv(g.H * g.W, r.sp) + 1) & ~1;          // even: a pixel pair never straddles two blocks
    r.nsplit = g.N * r.sp;
  } else if (r.rowtap) {
    r.family = WgradFamily::RowTap;
    r.split = g_conv_math != 2;
    r.nseg = cdiv(g.Wo, 16);
    // paired tails (see the kernel): rows of 16 q + rem pixels, 0 < rem <= 8, at least two rows per image
    const int rem = g.Wo & 15;
    r.tail_rem = (rem > 0 && rem <= 8 && g.Wo >= 16 && g.Ho >= 2 && g_wgrad_cfg != WGRAD_CFG_NO_PAIRED_TAILS) ? rem : 0;
    const int nchunks = r.tail_rem ? ((g.N * g.Ho + 1) / 2) * (2 * (g.Wo / 16) + 1) : g.N * g.Ho * r.nseg;
    if (r.nsplit > 0) r.cps = cdiv(nchunks, r.nsplit);
  } else if (!scaled && g_wgrad_cfg < WGRAD_CFG_REG) {
    r.family = WgradFamily::Dma;
    r.math = g_conv_math;
    r.wbk = (g_conv_math == 0 && r.p.bk == 32) ? 32 : 16;
  }
  return r;
}

template <int BM, int CIS>
static void launch_rowtap(const WgradRoute& r, const WgradGeom& g, const float* x, const float* dy, float* partial, float* bias_partial,
                          const WgradBatch& bt, int blocks, hipStream_t st) {
  // (tile: BM destination channels x 3 CIS columns; the bn field carries the paired-tail remainder, phases the problems of a grouped launch)
  route_note(RF_ROWTAP, BM, 3 * CIS, r.tail_rem, r.split ? 1 : 2, 0, blocks, g.nsplit, r.cps, bt.nprob);
  auto k = r.split ? wgrad_rowtap_kernel<BM, CIS, true> : wgrad_rowtap_kernel<BM, CIS, false>;
  hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, st, x, dy, partial, bias_partial, g, r.nseg, r.cps, r.tail_rem, bt);
}
template <int BM, int BN, int WM, int WN>
static void launch_wgrad_tile(const WgradRoute& r, const WgradGeom& g, const float* x, const float* dy, float* partial, float* bias_partial,
                              const float* xrow, const float* xchan, int blocks, hipStream_t st) {
  if (r.family == WgradFamily::Reg) {
    route_note(RF_WREG, BM, BN, 16, 0, 0, blocks, g.nsplit, g.chunks_per_split);
    hipLaunchKernelGGL((fast_wgrad_kernel<BM, BN, WM, WN>), dim3(blocks), dim3(256), 0, st, x, dy, partial, bias_partial, xrow, xchan, g);
    return;
  }
  auto k = r.math == 2 ? fast_wgrad_dma_kernel<BM, BN, WM, WN, 16, 2> : r.math == 1 ? fast_wgrad_dma_kernel<BM, BN, WM, WN, 16, 1> :
           r.wbk == 32 ? fast_wgrad_dma_kernel<BM, BN, WM, WN, 32, 0> : fast_wgrad_dma_kernel<BM, BN, WM, WN, 16, 0>;
  route_note(RF_WDMA, BM, BN, r.math == 0 ? r.wbk : 16, r.math, 0, blocks, g.nsplit, g.chunks_per_split);   // (bn field: pixels per K chunk)
  hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, st, x, dy, partial, bias_partial, g);
}
// the split-K main launch of a RowTap / Dma / Reg route (bt: the problems of a grouped row-tap launch, empty for one problem)
static void launch_wgrad_main(const WgradRoute& r, const WgradGeom& g, const float* x, const float* dy, float* partial, float* bias_partial,
                              const WgradBatch& bt, const float* xrow, const float* xchan, int blocks, hipStream_t st) {
  const FastWgradPlan& p = r.p;
  if (r.family == WgradFamily::RowTap) {
    if (r.rowtap == 1) launch_rowtap<128, 64>(r, g, x, dy, partial, bias_partial, bt, blocks, st);
    else launch_rowtap<64, 128>(r, g, x, dy, partial, bias_partial, bt, blocks, st);
    return;
  }
  auto f = (p.bm == 256 && p.bn == 64) ? launch_wgrad_tile<256, 64, 4, 1> : (p.bm == 64 && p.bn == 256) ? launch_wgrad_tile<64, 256, 1, 4> :
           (p.bm == 128 && p.bn == 128) ? launch_wgrad_tile<128, 128, 2, 2> : p.bm == 128 ? launch_wgrad_tile<128, 64, 2, 2> :
           p.bn == 128 ? launch_wgrad_tile<64, 128, 1, 4> : launch_wgrad_tile<64, 64, 2, 2>;
  f(r, g, x, dy, partial, bias_partial, xrow, xchan, blocks, st);
}
// the scalar split-K reduce: where launch_reduce4 declines
static void launch_reduce_scalar(bool sub16, const float* partial, const float* bias_partial, float* dw, float* db, int nsplit, const WgradGeom& g,
                                 int accumulate, hipStream_t st) {
  const long total = (long)g.K * g.Ktot + (db ? g.K : 0);
  route_note(RF_REDUCE_SCALAR, sub16 ? 16 : 4, 1, 0, 0, 0, cdiv(total, 64), nsplit);
  auto k = sub16 ? fast_wgrad_reduce_kernel<16> : fast_wgrad_reduce_kernel<4>;
  hipLaunchKernelGGL(k, dim3(cdiv(total, 64)), dim3(sub16 ? 1024 : 256), 0, st, partial, bias_partial, dw, db, nsplit, g.K, g.C, g.KH * g.KW, g.Ktot,
                     accumulate);
}

int fast_conv2d_wgrad(const float* x, const float* dy, float* dw, float* db, const float* xrow, const float* xchan,
                      int accumulate, void* workspace, size_t workspace_bytes, int n, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad, int ldx, int ldy,
                      hipStream_t st) {
  SRHIP_REQUIRE(ldx % 4 == 0 && ldy % 4 == 0 && (((uintptr_t)x | (uintptr_t)dy) & 15) == 0,
                "conv2d_wgrad: x/dy must be 16-byte aligned with row strides % 4 == 0");
  WgradGeom g;
  g.N = n; g.H = h; g.W = w; g.C = cin; g.ldx = ldx;
  g.Ho = (h + 2 * pad - kh) / stride + 1;
  g.Wo = (w + 2 * pad - kw) / stride + 1;
  SRHIP_REQUIRE(g.Ho > 0 && g.Wo > 0, "conv2d_wgrad: empty output");
  g.K = cout; g.ldy = ldy; g.KH = kh; g.KW = kw; g.stride = stride; g.pad = pad;
  const long P = (long)n * g.Ho * g.Wo;
  SRHIP_REQUIRE(P < (1L << 31) - 64, "conv2d_wgrad: pixel count overflows int32");
  g.P = (int)P; g.Ktot = kh * kw * cin;
  SRHIP_REQUIRE(bytes_ok((long)n * h * w, ldx, cin, &g.x_bytes) && bytes_ok(P, ldy, cout, &g.dy_bytes),
                "conv2d_wgrad: tensor >= 2 GiB");
  const WgradRoute r = choose_wgrad_route(g, 1, xrow != nullptr, xchan != nullptr, workspace_bytes);
  const FastWgradPlan& p = r.p;
  g.nsplit = p.nsplit; g.chunks_per_split = p.chunks_per_split;
  const size_t need = (size_t)p.nsplit * ((size_t)cout * g.Ktot + cout) * sizeof(float);
  if (!workspace || workspace_bytes < need) {
    set_error("conv2d_wgrad: workspace %zu bytes < required %zu", workspace_bytes, need);
    return SRHIP_ERR_WORKSPACE;
  }
  float* partial = static_cast<float*>(workspace);
  float* bias_partial = partial + (size_t)r.nsplit * cout * g.Ktot;
  const float* pp[1] = {partial};
  float* dwp[1] = {dw};
  float* dbp[1] = {db};
  if (r.family == WgradFamily::Tail1x1) {
    float* bp = db ? bias_partial : nullptr;
    const float* bpp[1] = {bp};
    route_note(RF_TAIL1X1, 64, 64, 0, 0, 0, r.nsplit, r.nsplit, r.per);     // (cps: pixels per split)
    hipLaunchKernelGGL(wgrad_1x1_scaled_kernel, dim3(r.nsplit), dim3(256), 0, st, x, dy, xrow, xchan, partial, bp, h * w, r.per, r.sp);
    int rc1 = check_launch("wgrad_1x1_scaled");
    if (rc1) return rc1;
    if (launch_reduce4(1, pp, bpp, dwp, dbp, r.nsplit, cout, cin, 1, g.Ktot, accumulate, st)) return check_launch("fast_wgrad_reduce4");
    launch_reduce_scalar(false, partial, bp, dw, db, r.nsplit, g, accumulate, st);
    return check_launch("fast_wgrad_reduce");
  }
  launch_wgrad_main(r, g, x, dy, partial, db ? bias_partial : nullptr, WgradBatch{}, xrow, xchan, cdiv(cout, p.bm) * cdiv(g.Ktot, p.bn) * p.nsplit, st);
  int rc = check_launch("fast_wgrad");
  if (rc) return rc;
  const float* bp[1] = {bias_partial};
  const bool generic = g_wgrad_cfg == WGRAD_CFG_SCALAR_REDUCE_GENERIC;
  if (!generic && launch_reduce4(1, pp, bp, dwp, dbp, p.nsplit, cout, cin, kh * kw, g.Ktot, accumulate, st))
    return check_launch("fast_wgrad_reduce4");
  launch_reduce_scalar(p.nsplit >= (generic ? 256 : 64), partial, bias_partial, dw, db, p.nsplit, g, accumulate, st);
  return check_launch("fast_wgrad_reduce");
}

// ---- grouped row-tap weight gradient: nprob (2..4) convolutions of one shape, one main launch + nprob reduces ----
int fast_wgrad_multi_ok(int cin, int cout, int kh, int kw, int stride, int pad) {
  return g_conv_math >= 1 ? rowtap_ok(cin, cout, kh, kw, stride, pad) : 0;
}
// largest group size (2..4) a problem of this geometry can share a launch with, 0: none (shape, arithmetic mode or too few chunks)
int fast_wgrad_multi_max(int n, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad) {
  const int rowtap = fast_wgrad_multi_ok(cin, cout, kh, kw, stride, pad);
  if (!rowtap) return 0;
  FastWgradPlan p = plan_fast_wgrad((long)n * h * w, cout, kh * kw * cin, rowtap);
  for (int k = 4; k >= 2; --k)
    if (multi_nsplit(p, k) > 0) return k;
  return 0;
}
size_t fast_conv2d_wgrad_multi_workspace(int nprob, int n, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad) {
  return fast_conv2d_wgrad_workspace(n, h, w, cin, cout, kh, kw, stride, pad);     // nprob * (nsplit / nprob) partial sets
}
int fast_conv2d_wgrad_multi(int nprob, const float* const* x, const float* const* dy, float* const* dw, float* const* db,
                            int accumulate, void* workspace, size_t workspace_bytes, int n, int h, int w, int cin, int cout,
                            int kh, int kw, int stride, int pad, int ldx, int ldy, hipStream_t st) {
  SRHIP_REQUIRE(nprob >= 2 && nprob <= 4, "conv2d_wgrad_multi: 2..4 problems per launch");
  SRHIP_REQUIRE(fast_wgrad_multi_ok(cin, cout, kh, kw, stride, pad) != 0, "conv2d_wgrad_multi: shape / arithmetic mode not served by the row-tap kernel");
  WgradGeom g;
  g.N = n; g.H = h; g.W = w; g.C = cin; g.ldx = ldx;
  g.Ho = h; g.Wo = w;                                     // stride 1, pad 1, 3 x 3
  g.K = cout; g.ldy = ldy; g.KH = kh; g.KW = kw; g.stride = stride; g.pad = pad;
  const long P = (long)n * g.Ho * g.Wo;
  SRHIP_REQUIRE(P < (1L << 31) - 64, "conv2d_wgrad_multi: pixel count overflows int32");
  g.P = (int)P; g.Ktot = kh * kw * cin;
  SRHIP_REQUIRE(ldx % 4 == 0 && ldy % 4 == 0, "conv2d_wgrad_multi: row strides % 4 == 0");
  SRHIP_REQUIRE(bytes_ok((long)n * h * w, ldx, cin, &g.x_bytes) && bytes_ok(P, ldy, cout, &g.dy_bytes), "conv2d_wgrad_multi: tensor >= 2 GiB");
  const WgradRoute r = choose_wgrad_route(g, nprob, false, false, 0);
  const int ns = r.nsplit;
  SRHIP_REQUIRE(ns > 0, "conv2d_wgrad_multi: problem too small to share a launch (use srhip_conv2d_wgrad)");
  g.nsplit = ns; g.chunks_per_split = r.cps;
  const size_t per = (size_t)ns * ((size_t)cout * g.Ktot + cout);
  SRHIP_REQUIRE(workspace && workspace_bytes >= per * nprob * sizeof(float), "conv2d_wgrad_multi: workspace too small");
  WgradBatch bt;
  bt.nprob = nprob;
  bt.bpp = cdiv(cout, r.p.bm) * cdiv(g.Ktot, r.p.bn) * ns;
  for (int i = 0; i < 4; ++i) {
    const int k = i < nprob ? i : 0;
    SRHIP_REQUIRE(x[k] && dy[k] && dw[k] && ((((uintptr_t)x[k]) | ((uintptr_t)dy[k])) & 15) == 0, "conv2d_wgrad_multi: null / unaligned tensor");
    float* part = static_cast<float*>(workspace) + per * k;
    bt.x[i] = x[k];
    bt.dy[i] = dy[k];
    bt.partial[i] = part;
    bt.bias_partial[i] = (db && db[k]) ? part + (size_t)ns * cout * g.Ktot : nullptr;
  }
  launch_wgrad_main(r, g, bt.x[0], bt.dy[0], bt.partial[0], bt.bias_partial[0], bt, nullptr, nullptr, bt.bpp * nprob, st);
  int rc = check_launch("fast_wgrad_multi");
  if (rc) return rc;
  if (launch_reduce4(nprob, bt.partial, bt.bias_partial, dw, db, ns, cout, cin, kh * kw, g.Ktot, accumulate, st))
    return check_launch("fast_wgrad_multi_reduce4");
  for (int k = 0; k < nprob; ++k)
    launch_reduce_scalar(ns >= 64, bt.partial[k], bt.bias_partial[k], dw[k], db ? db[k] : nullptr, ns, g, accumulate, st);
  return check_launch("fast_wgrad_multi_reduce");
}

}  // namespace srhip
