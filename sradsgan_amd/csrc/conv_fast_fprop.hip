// Fast implicit-GEMM convolution kernels for gfx950, forward and data gradient (source channels % 16 == 0, <= 32 taps;
// the weight gradient is conv_wgrad_fast.hip): the
// shapes that carry >95 % of the SRADSGAN step's FLOPs (RAB 3x3 64<->256, 1x1 tails, upsampler,
// discriminator and VGG 3x3 convs).  Exact-fp32 matrix pipe (v_mfma_f32_32x32x2_f32).
//
// What makes them fast compared with the generic kernel (conv_igemm.hip):
//   * both GEMM operands are "row = M/N index, K contiguous" in global memory (NHWC activations,
//     n-major packed weights), so tiles go global -> VGPR -> LDS as 16-byte vectors with NO
//     transpose, and MFMA fragments come back as ds_read_b128: the K order inside an 8-wide group is
//     permuted identically for A and B (lanes 0-31 take k 0..3, lanes 32-63 take k 4..7), which a
//     contraction does not care about.  LDS rows are 80 bytes apart => conflict-free b128 reads;
//   * a K chunk of 16 never straddles a filter tap, so the im2col address of a chunk is
//     "per-thread pixel base + one scalar tap offset"; padding/stride holes are handled by the
//     buffer-load bounds check (offset >= num_records returns 0): no branches, ~3 VALU per load;
//   * strided backward-data is decomposed into stride^2 phase classes, each a dense GEMM over only
//     the taps that hit it (a 3x3 stride-2 dgrad does 9 tap-GEMMs instead of 36);
//   * XCD-aware tile order: each of the 8 XCDs walks a contiguous range of output tiles, so the
//     halo rows and the weights of neighbouring tiles are served by that XCD's L2;
#include "conv_dev.h"

namespace srhip {

int g_fast_ablate = 0;   // srhip_debug_set(3, bits): the FAST_ABL_* bits (conv_dev.h)

// ================================================================================================ //
// fprop / dgrad
// ================================================================================================ //

// MATH >= 1 (BK 16 only): 16-bit products (PROD = MATH - 1), B read from the pre-split / fp16 section of the packed weights
template <int BM, int BN, int WM, int WN, int BK, int MATH = 0>
__global__ __launch_bounds__(WM* WN * 64) void fast_conv_kernel(const float* __restrict__ src,
                                                                 const float* __restrict__ wt,
                                                                 const float* __restrict__ bias,
                                                                 const float* __restrict__ residual,
                                                                 const float* __restrict__ rowscale,
                                                                 const float* __restrict__ chanscale,
                                                                 const float* __restrict__ actmask,
                                                                 float* __restrict__ dst, FastGeom g, int nblk_m,
                                                                 int nblk_n) {
  constexpr int NT = WM * WN * 64;                 // threads
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int LS = BK + 4;                       // LDS row stride (floats): (LS/4) odd => conflict-free b128 reads
  constexpr int QPR = BK / 4;                      // 16-byte quads per row
  constexpr int RPP = NT / QPR;                    // rows covered by one pass of all threads
  constexpr int AR = (BM + RPP - 1) / RPP, BR = (BN + RPP - 1) / RPP;
  constexpr int STAGE = (BM + BN) * LS;
  __shared__ __attribute__((aligned(16))) float lds[2 * STAGE];

  const int tid = threadIdx.x;
  const int tile = xcd_tile(blockIdx.x, nblk_m * nblk_n);
  const int tile_n = tile % nblk_n, tile_m = tile / nblk_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int lrow = tid / QPR, kq = tid % QPR;

  __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(src), 0, g.src_bytes, 0x00020000);
  __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wt), 0, g.w_bytes, 0x00020000);

  // ---- per-thread row bookkeeping, fixed for the whole K loop ----
  int abase[AR], aimg[AR];
  unsigned amask[AR];
  const int OHOW = g.OH * g.OW;
  const bool cscale = (g.flags & SRHIP_EPI_CHANSCALE) != 0;      // A[m][k] *= chanscale[image(m)][c(k)]
#pragma unroll
  for (int i = 0; i < AR; ++i) {
    const int m = m0 + lrow + RPP * i;
    abase[i] = 0;
    amask[i] = 0;
    aimg[i] = 0;
    if (m < g.M && (BM % RPP == 0 || lrow + RPP * i < BM)) {
      const int n = m / OHOW;
      aimg[i] = n;
      const int rem = m - n * OHOW;
      const int oh = rem / g.OW;
      const int ow = rem - oh * g.OW;
      const int sh0 = oh * g.ss, sw0 = ow * g.ss;
      abase[i] = ((n * g.Hs + sh0) * g.Ws + sw0) * g.lds + kq * 4;
      unsigned mk = 0;
      for (int th = 0; th < g.TH; ++th) {
        const int sh = sh0 + g.dh0 + th * g.dhs;
        for (int tw = 0; tw < g.TW; ++tw) {
          const int sw = sw0 + g.dw0 + tw * g.dws;
          if (sh >= 0 && sh < g.Hs && sw >= 0 && sw < g.Ws) mk |= 1u << (th * g.TW + tw);
        }
      }
      amask[i] = mk;
    }
  }
  int bbase[BR];
  bool bval[BR];
#pragma unroll
  for (int j = 0; j < BR; ++j) {
    const int n = n0 + lrow + RPP * j;
    bval[j] = (BN % RPP == 0 || lrow + RPP * j < BN) && n < g.K;
    bbase[j] = n * g.ldw + kq * 4;
  }

  // ---- K-loop state (wave-uniform): tap (th,tw), channel chunk cc ----
  const int CC = g.C / BK;
  const int nk = g.TH * g.TW * CC;
  int th = 0, tw = 0, cc = 0;
  float4 ra[AR], rb[BR], rsc[AR];

  auto load_tiles = [&]() {
    const int tapoff = ((g.dh0 + th * g.dhs) * g.Ws + (g.dw0 + tw * g.dws)) * g.lds + cc * BK;
    if (cscale) {
#pragma unroll
      for (int i = 0; i < AR; ++i)
        rsc[i] = *reinterpret_cast<const float4*>(chanscale + (size_t)aimg[i] * g.C + cc * BK + kq * 4);
    }
    const int wk = ((g.kh0 + th * g.khs) * g.KW + (g.kw0 + tw * g.kws)) * g.C + cc * BK;
    const int bit = th * g.TW + tw;
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      const unsigned off = ((amask[i] >> bit) & 1u) ? (unsigned)(abase[i] + tapoff) * 4u : F_OOB;
      ra[i] = bufload4(rs, off);
    }
#pragma unroll
    for (int j = 0; j < BR; ++j) {
      const unsigned off = bval[j] ? (unsigned)(bbase[j] + wk) * 4u : F_OOB;
      rb[j] = bufload4(rw, off);
    }
    // taps innermost: the 9 taps of one 16-channel chunk re-read the same 64-byte segments of ~3 image
    // rows back to back (L1/L2 hits); with taps outermost a 256-channel input was re-fetched 9x from
    // beyond L2 (FETCH_SIZE 788 MB vs 96 MB algorithmic, profiles/r01_conv_pmc_summary.txt)
    if (++tw == g.TW) {
      tw = 0;
      if (++th == g.TH) {
        th = 0;
        ++cc;
      }
    }
  };
  auto store_tiles = [&](int stage) {
    float* a = lds + stage * STAGE + lrow * LS + kq * 4;
    if (cscale) {
#pragma unroll
      for (int i = 0; i < AR; ++i) {
        ra[i].x *= rsc[i].x;
        ra[i].y *= rsc[i].y;
        ra[i].z *= rsc[i].z;
        ra[i].w *= rsc[i].w;
      }
    }
#pragma unroll
    for (int i = 0; i < AR; ++i)
      if (BM % RPP == 0 || lrow + RPP * i < BM) *reinterpret_cast<float4*>(a + RPP * i * LS) = ra[i];
    float* b = lds + stage * STAGE + BM * LS + lrow * LS + kq * 4;
#pragma unroll
    for (int j = 0; j < BR; ++j)
      if (BN % RPP == 0 || lrow + RPP * j < BN) *reinterpret_cast<float4*>(b + RPP * j * LS) = rb[j];
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

  if (nk > 0) {
    load_tiles();
    store_tiles(0);
    __syncthreads();
    const bool abl_noload = (g.flags & 0x100) != 0, abl_nobar = (g.flags & 0x200) != 0;   // timing ablations only
    for (int kc = 0; kc < nk; ++kc) {
      const int stage = abl_noload ? 0 : (kc & 1);
      if (kc + 1 < nk && !abl_noload) load_tiles();
      if (MATH >= 1) {
        constexpr int PROD = MATH >= 1 ? MATH - 1 : 0;
        const float* a = lds + stage * STAGE + (wm * WTM + l31) * LS + khalf * 8;
        const float* b = lds + stage * STAGE + BM * LS + (wn * WTN + l31) * LS + khalf * 8;
        bf16x8_t ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
        for (int t = 0; t < TM; ++t) {
          const float4 a0 = *reinterpret_cast<const float4*>(a + t * 32 * LS), a1 = *reinterpret_cast<const float4*>(a + t * 32 * LS + 4);
          if (PROD == 0) split_bf16x8(a0, a1, ah[t], al[t]);
          else ah[t] = al[t] = round16x8<PROD>(a0, a1);
        }
#pragma unroll
        for (int u = 0; u < TN; ++u) {
          bh[u] = *reinterpret_cast<const bf16x8_t*>(b + u * 32 * LS);
          bl[u] = PROD == 0 ? *reinterpret_cast<const bf16x8_t*>(b + u * 32 * LS + 4) : bh[u];
        }
#pragma unroll
        for (int i = 0; i < nprod<PROD>() * TM * TN; ++i) {
          const int grp = PROD == 0 ? i / (TM * TN) : 2, t = (i % (TM * TN)) / TN, u = i % TN;
          acc[t][u] = mma16<PROD>(grp == 0 ? al[t] : ah[t], grp == 1 ? bl[u] : bh[u], acc[t][u]);
        }
        if (kc + 1 < nk && !abl_noload) store_tiles(stage ^ 1);
        if (!abl_nobar) __syncthreads();
        continue;
      }
      const float* a = lds + stage * STAGE + (wm * WTM + l31) * LS + khalf * 4;
      const float* b = lds + stage * STAGE + BM * LS + (wn * WTN + l31) * LS + khalf * 4;
      float4 af[2][TM], bf[2][TN];
#pragma unroll
      for (int t = 0; t < TM; ++t) af[0][t] = *reinterpret_cast<const float4*>(a + t * 32 * LS);
#pragma unroll
      for (int u = 0; u < TN; ++u) bf[0][u] = *reinterpret_cast<const float4*>(b + u * 32 * LS);
#pragma unroll
      for (int ks = 0; ks < BK / 8; ++ks) {
        const int cur = ks & 1, nxt = cur ^ 1;
        if (ks + 1 < BK / 8) {
#pragma unroll
          for (int t = 0; t < TM; ++t) af[nxt][t] = *reinterpret_cast<const float4*>(a + t * 32 * LS + (ks + 1) * 8);
#pragma unroll
          for (int u = 0; u < TN; ++u) bf[nxt][u] = *reinterpret_cast<const float4*>(b + u * 32 * LS + (ks + 1) * 8);
        }
#pragma unroll
        for (int t = 0; t < TM; ++t)
#pragma unroll
          for (int u = 0; u < TN; ++u) acc[t][u] = mfma32f(af[cur][t].x, bf[cur][u].x, acc[t][u]);
#pragma unroll
        for (int t = 0; t < TM; ++t)
#pragma unroll
          for (int u = 0; u < TN; ++u) acc[t][u] = mfma32f(af[cur][t].y, bf[cur][u].y, acc[t][u]);
#pragma unroll
        for (int t = 0; t < TM; ++t)
#pragma unroll
          for (int u = 0; u < TN; ++u) acc[t][u] = mfma32f(af[cur][t].z, bf[cur][u].z, acc[t][u]);
#pragma unroll
        for (int t = 0; t < TM; ++t)
#pragma unroll
          for (int u = 0; u < TN; ++u) acc[t][u] = mfma32f(af[cur][t].w, bf[cur][u].w, acc[t][u]);
      }
      if (kc + 1 < nk && !abl_noload) store_tiles(stage ^ 1);
      if (!abl_nobar) __syncthreads();
    }
  }

  // ---- epilogue: C/D map of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5) ----
#pragma unroll
  for (int t = 0; t < TM; ++t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + wm * WTM + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
      if (m >= g.M) continue;
      size_t dpix = (size_t)m;
      if (!g.dst_identity) {
        const int n = m / OHOW;
        const int rem = m - n * OHOW;
        const int oh = rem / g.OW;
        const int ow = rem - oh * g.OW;
        dpix = ((size_t)n * g.Hd + (oh * g.dsd + g.ph)) * g.Wd + (ow * g.dsd + g.pw);
      }
      const float rsc = (g.flags & SRHIP_EPI_ROWSCALE) ? rowscale[dpix] : 1.f;
#pragma unroll
      for (int u = 0; u < TN; ++u) {
        const int n = n0 + wn * WTN + u * 32 + l31;
        if (n >= g.K) continue;
        float v = acc[t][u][r];
        if (g.flags & SRHIP_EPI_ROWSCALE) v *= rsc;
        if (g.flags & SRHIP_EPI_BIAS) v += bias[n];
        if (g.flags & SRHIP_EPI_LRELU) v = v > 0.f ? v : v * g.slope;
        if (g.flags & SRHIP_EPI_ACTMASK) v = actmask[dpix * g.ldd + n] > 0.f ? v : v * g.slope;
        if (g.flags & SRHIP_EPI_RESIDUAL) v += residual[dpix * g.ldr + n];
        float* o = dst + dpix * g.ldd + n;
        if (g.accumulate) v += *o;
        *o = v;
      }
    }
  }
}

// ================================================================================================ //
// fprop / dgrad, LDS-DMA variant: tiles go global -> LDS with global_load_lds_dwordx4 (no VGPR
// staging, no ds_write), 3-stage ring, prefetch distance 2, ONE raw s_barrier per K chunk and a
// counted s_waitcnt vmcnt (the loads of the next chunk stay in flight across the barrier).
//   * the DMA writes lane-linear (wave base + lane*16 B), so an LDS row is 64 B unpadded and the
//     bank spread comes from an XOR swizzle applied on the SOURCE side: 16-byte slot (row, s) holds
//     global quad q = s ^ ((row>>2)&3); fragment reads apply the same involution => conflict-free
//     ds_read_b128 (every 16-lane service group covers all 16 slots of a 256 B bank row once);
//   * padding / stride holes: lanes whose tap falls outside the image pass an out-of-range buffer offset (F_OOB) and the
//     hardware delivers zeros (lds_dma16_buf);
//   * the DMA and its wait are inline asm (hipcc would otherwise drain vmcnt(0) before every ds_read
//     that may alias an in-flight LDS-DMA); the fragment reads stay ordinary loads and are ordered
//     behind the asm wait + barrier by their "memory" clobbers;
//   * EPI >= 0 fixes the epilogue flags at compile time (no per-element branches); EPI < 0 = dynamic.
// ================================================================================================ //
// epilogue of one float4 of output (4 consecutive channels n.. of destination pixel dpix)
// Round 4: the epilogue of a tile row group is TWO loops -- every global operand of its NRD output quads is fetched first
// (epi_fetch), then the arithmetic and the stores follow (epi_finish).  Loads and stores retire in order on this memory pipeline:
// with one fused "load, wait, store" per quad, hipcc's wait for quad k's operands also waited for quad k-1's store to complete
// (8 chained store latencies per wave and tile in the residual / activation-mask / row-scale epilogues, worst inside the step
// where three streams share the memory system).  Same operations in the same order per element: results unchanged.
struct EpiOps {
  float4 bb, a4, r4, p4;
  float rsc;
};
__device__ inline EpiOps epi_fetch(size_t dpix, int n, int flags, const FastGeom& g, const float* __restrict__ bias,
                                   const float* __restrict__ residual, const float* __restrict__ rowscale,
                                   const float* __restrict__ actmask, const float* __restrict__ dst, bool accumulate) {
  EpiOps o;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  // (real branches: written as selects, hipcc turns a run-time-flagged load into a load through a pointer to a zero in scratch)
  o.rsc = 1.f;
  o.bb = z;
  o.a4 = z;
  o.r4 = z;
  if (flags & SRHIP_EPI_ROWSCALE) {
    asm volatile("" ::: "memory");
    o.rsc = rowscale[dpix];
  }
  if (flags & SRHIP_EPI_BIAS) {
    asm volatile("" ::: "memory");
    o.bb = *reinterpret_cast<const float4*>(bias + n);
  }
  if (flags & SRHIP_EPI_ACTMASK) {
    asm volatile("" ::: "memory");
    o.a4 = *reinterpret_cast<const float4*>(actmask + dpix * g.ldd + n);
  }
  if (flags & SRHIP_EPI_RESIDUAL) {
    asm volatile("" ::: "memory");
    o.r4 = *reinterpret_cast<const float4*>(residual + dpix * g.ldr + n);
  }
  o.p4 = z;
  if (accumulate) {                                   // a real branch: as a select hipcc loads through a pointer to a zero in scratch
    asm volatile("" ::: "memory");
    o.p4 = *reinterpret_cast<const float4*>(dst + dpix * g.ldd + n);
  }
  return o;
}
__device__ inline void epi_finish(float4 v, const EpiOps& e, size_t dpix, int n, int flags, const FastGeom& g, float* __restrict__ dst,
                                  bool accumulate) {
  if (flags & SRHIP_EPI_ROWSCALE) {
    v.x *= e.rsc; v.y *= e.rsc; v.z *= e.rsc; v.w *= e.rsc;
  }
  if (flags & SRHIP_EPI_BIAS) {
    v.x += e.bb.x; v.y += e.bb.y; v.z += e.bb.z; v.w += e.bb.w;
  }
  if (flags & SRHIP_EPI_LRELU) {
    v.x = v.x > 0.f ? v.x : v.x * g.slope;
    v.y = v.y > 0.f ? v.y : v.y * g.slope;
    v.z = v.z > 0.f ? v.z : v.z * g.slope;
    v.w = v.w > 0.f ? v.w : v.w * g.slope;
  }
  if (flags & SRHIP_EPI_ACTMASK) {
    v.x = e.a4.x > 0.f ? v.x : v.x * g.slope;
    v.y = e.a4.y > 0.f ? v.y : v.y * g.slope;
    v.z = e.a4.z > 0.f ? v.z : v.z * g.slope;
    v.w = e.a4.w > 0.f ? v.w : v.w * g.slope;
  }
  if (flags & SRHIP_EPI_RESIDUAL) {
    v.x += e.r4.x; v.y += e.r4.y; v.z += e.r4.z; v.w += e.r4.w;
  }
  float4* o = reinterpret_cast<float4*>(dst + dpix * g.ldd + n);
  if (accumulate) {
    v.x += e.p4.x; v.y += e.p4.y; v.z += e.p4.z; v.w += e.p4.w;
  }
  // Conv outputs are streamed out with the non-temporal hint: nothing in this kernel reads them back, and keeping them
  // out of the L2's way is worth 3-4 % on the 64 -> 256 fprop (95.6 MB written) and 0.4 % on the step.
  if (g.dst2_pp != nullptr) {                       // the same four channels as padded planes: octet n / 8, hi half at + (n & 4) * 2, lo 16 bytes further
    const unsigned hwd = (unsigned)(g.Hd * g.Wd);
    const unsigned img = (unsigned)dpix / hwd, rem = (unsigned)dpix - img * hwd;
    const unsigned oy = rem / (unsigned)g.Wd, ox = rem - oy * (unsigned)g.Wd;
    const size_t row = (size_t)g.dst2_guard + ((size_t)img * (g.Hd + 1) + oy) * (g.Wd + 1) + ox;
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    const bf16x2_t h01 = {(__bf16)v.x, (__bf16)v.y}, h23 = {(__bf16)v.z, (__bf16)v.w};
    const unsigned uh01 = __builtin_bit_cast(unsigned, h01), uh23 = __builtin_bit_cast(unsigned, h23);
    const bf16x2_t l01 = {(__bf16)(v.x - __uint_as_float(uh01 << 16)), (__bf16)(v.y - __uint_as_float(uh01 & 0xffff0000u))};
    const bf16x2_t l23 = {(__bf16)(v.z - __uint_as_float(uh23 << 16)), (__bf16)(v.w - __uint_as_float(uh23 & 0xffff0000u))};
    // The two lanes of an octet (adjacent lanes, adjacent quads: the row-group loop's mapping) trade halves so that each stores ONE whole
    // 16-byte piece -- the even lane the octet's 8 hi halves, the odd lane its 8 lo halves: a store instruction then writes whole rows
    // (two 8-byte stores per lane wrote 16 bytes of every 32 per instruction and the memory side counted them as partial lines).
    const bool odd = ((n >> 2) & 1) != 0;
    const unsigned ul01 = __builtin_bit_cast(unsigned, l01), ul23 = __builtin_bit_cast(unsigned, l23);
    const unsigned r0 = pair_swap(odd ? uh01 : ul01), r1 = pair_swap(odd ? uh23 : ul23);   // even lane receives the odd lane's hi, odd lane the even lane's lo
    unsigned* o2 = static_cast<unsigned*>(g.dst2_pp) + row * g.K + (n >> 3) * 8 + (odd ? 4 : 0);
    *reinterpret_cast<uint4*>(o2) = odd ? make_uint4(r0, r1, ul01, ul23) : make_uint4(uh01, uh23, r0, r1);
  }
  if (g.flags & 0x400) {                            // srhip_debug_set(3, 0x400): plain stores (A/B)
    *o = v;
    return;
  }
  __builtin_nontemporal_store(v.x, &o->x);
  __builtin_nontemporal_store(v.y, &o->y);
  __builtin_nontemporal_store(v.z, &o->z);
  __builtin_nontemporal_store(v.w, &o->w);
}
// one output quad, fetch and finish together (kernels whose epilogue is not a row-group loop)
__device__ inline void epi_apply_store(float4 v, size_t dpix, int n, int flags, const FastGeom& g,
                                       const float* __restrict__ bias, const float* __restrict__ residual,
                                       const float* __restrict__ rowscale, const float* __restrict__ actmask,
                                       float* __restrict__ dst) {
  const EpiOps e = epi_fetch(dpix, n, flags, g, bias, residual, rowscale, actmask, dst, g.accumulate != 0);
  epi_finish(v, e, dpix, n, flags, g, dst, g.accumulate != 0);
}

// ================================================================================================ //
template <int BM, int BN, int EPI, int MATH>
__global__ __launch_bounds__(256) void fast_conv_dma_kernel(const float* __restrict__ src, const float* __restrict__ wt,
                                                             const float* __restrict__ bias,
                                                             const float* __restrict__ residual,
                                                             const float* __restrict__ rowscale,
                                                             const float* __restrict__ chanscale,
                                                             const float* __restrict__ actmask,
                                                             float* __restrict__ dst, FastGeom g_in, int nblk_m,
                                                             int nblk_n, PhaseSet ps) {
  constexpr int WM = 2, WN = 2, BK = 16;
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int AI = BM / 64, BI = BN / 64;            // DMA instructions per wave per chunk (16 rows each)
  constexpr int STAGE_B = (BM + BN) * 64;              // bytes per stage (64 B per row)
  __shared__ __attribute__((aligned(1024))) char lds[3 * STAGE_B];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: keeps per-wave control flow on the scalar unit
  FastGeom g = g_in;
  int bid = blockIdx.x;
  if (ps.n > 1) {                                      // the phases of a strided data gradient in one launch (PhaseSet, conv_dev.h)
    int k = 0;
    if (bid >= ps.first[1]) k = 1;
    if (ps.n > 2 && bid >= ps.first[2]) k = 2;
    if (ps.n > 3 && bid >= ps.first[3]) k = 3;
    bid -= ps.first[k];
    const PhaseSet::P q = ps.p[k];
    g.ph = q.ph; g.pw = q.pw; g.OH = q.OH; g.OW = q.OW; g.kh0 = q.kh0; g.kw0 = q.kw0; g.TH = q.TH; g.TW = q.TW;
    g.dh0 = q.dh0; g.dw0 = q.dw0; g.M = q.M;
    nblk_m = q.nblk_m;
  }
  const int tile = xcd_tile(bid, nblk_m * nblk_n);
  const int tile_n = tile % nblk_n, tile_m = tile / nblk_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) char*)lds;

  // ---- DMA bookkeeping: this lane feeds slot (row, s = lane&3) of rows wave*16*AI + 16*i + (lane>>2) ----
  const int OHOW = g.OH * g.OW;
  int abase[AI];
  unsigned amask[AI];
#pragma unroll
  for (int i = 0; i < AI; ++i) {
    const int row = wave * 16 * AI + 16 * i + (lane >> 2);
    const int q = (lane & 3) ^ ((row >> 2) & 3);
    const int m = m0 + row;
    abase[i] = 0;
    amask[i] = 0;
    if (m < g.M) {
      const int n = m / OHOW;
      const int rem = m - n * OHOW;
      const int oh = rem / g.OW;
      const int ow = rem - oh * g.OW;
      const int sh0 = oh * g.ss, sw0 = ow * g.ss;
      abase[i] = ((n * g.Hs + sh0) * g.Ws + sw0) * g.lds + q * 4;
      unsigned mk = 0;
      for (int th = 0; th < g.TH; ++th) {
        const int sh = sh0 + g.dh0 + th * g.dhs;
        for (int tw = 0; tw < g.TW; ++tw) {
          const int sw = sw0 + g.dw0 + tw * g.dws;
          if (sh >= 0 && sh < g.Hs && sw >= 0 && sw < g.Ws) mk |= 1u << (th * g.TW + tw);
        }
      }
      amask[i] = mk;
    }
  }
  int bbase[BI];
  bool bval[BI];
#pragma unroll
  for (int j = 0; j < BI; ++j) {
    const int row = wave * 16 * BI + 16 * j + (lane >> 2);
    const int q = (lane & 3) ^ ((row >> 2) & 3);
    const int n = n0 + row;
    bval[j] = n < g.K;
    bbase[j] = n * g.ldw + q * 4;
  }
  const unsigned a_dst = __builtin_amdgcn_readfirstlane(lds_base + wave * 16 * AI * 64);
  const unsigned b_dst = __builtin_amdgcn_readfirstlane(lds_base + BM * 64 + wave * 16 * BI * 64);

  const int CC = g.C / BK;
  const int nk = g.TH * g.TW * CC;
  int th = 0, tw = 0, cc = 0;
  __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(src), 0, g.src_bytes, 0x00020000);
  __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wt), 0, g.w_bytes, 0x00020000);
  auto issue = [&](int stage) {
    const int tapoff = ((g.dh0 + th * g.dhs) * g.Ws + (g.dw0 + tw * g.dws)) * g.lds + cc * BK;
    const int wk = ((g.kh0 + th * g.khs) * g.KW + (g.kw0 + tw * g.kws)) * g.C + cc * BK;
    const int bit = th * g.TW + tw;
    const unsigned so = stage * STAGE_B;
    // buffer-descriptor DMA: a lane that feeds padding carries an out-of-range offset and the hardware writes zeros
#pragma unroll
    for (int i = 0; i < AI; ++i)
      lds_dma16_buf(((amask[i] >> bit) & 1u) ? (unsigned)(abase[i] + tapoff) * 4u : F_OOB, rs_a, a_dst + so + i * 1024);
#pragma unroll
    for (int j = 0; j < BI; ++j) lds_dma16_buf(bval[j] ? (unsigned)(bbase[j] + wk) * 4u : F_OOB, rs_b, b_dst + so + j * 1024);
    // taps innermost: the 9 taps of one 16-channel chunk re-read the same 64-byte segments of ~3 image
    // rows back to back (L1/L2 hits); with taps outermost a 256-channel input was re-fetched 9x from
    // beyond L2 (FETCH_SIZE 788 MB vs 96 MB algorithmic, profiles/r01_conv_pmc_summary.txt)
    if (++tw == g.TW) {
      tw = 0;
      if (++th == g.TH) {
        th = 0;
        ++cc;
      }
    }
  };

  // ---- fragment addresses (bytes inside a stage): slot (row, q ^ ((row>>2)&3)), q = ks*2 + khalf ----
  const int wm = wave >> 1, wn = wave & 1;
  const int khalf = lane >> 5, l31 = lane & 31;
  // MATH 0 (fp32 MFMA 32x32x2, 4 k per read): lane half h takes quads q = h (ks 0) and q = 2 + h (ks 1)
  // MATH 1 (bf16 MFMA 32x32x16, 8 k per lane):  lane half h takes quads q = 2h and 2h + 1
  int aoff[TM], boff[TN];
#pragma unroll
  for (int t = 0; t < TM; ++t) {
    const int row = wm * WTM + t * 32 + l31;
    aoff[t] = row * 64 + ((((MATH ? 2 : 1) * khalf) ^ ((row >> 2) & 3)) << 4);
  }
#pragma unroll
  for (int u = 0; u < TN; ++u) {
    const int row = wn * WTN + u * 32 + l31;
    boff[u] = BM * 64 + row * 64 + ((((MATH ? 2 : 1) * khalf) ^ ((row >> 2) & 3)) << 4);
  }

  f32x16 acc[TM][TN];
#pragma unroll
  for (int t = 0; t < TM; ++t)
#pragma unroll
    for (int u = 0; u < TN; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][u][r] = 0.f;

  // A-operand channel scale (CLAM's s folded into the attention tail's 1x1 conv): fragment value
  // A[row][k] *= chanscale[image(row)][channel(k)], applied to the registers right after the LDS read
  const bool cscale = ((EPI >= 0 ? EPI : g.flags) & SRHIP_EPI_CHANSCALE) != 0;
  const float* csrow[TM];
#pragma unroll
  for (int t = 0; t < TM; ++t) {
    const int m = m0 + wm * WTM + t * 32 + l31;
    csrow[t] = chanscale + (size_t)((m < g.M ? m : 0) / OHOW) * g.C + khalf * 4;
  }
  const int T_taps = g.TH * g.TW;
  int c_tap = 0, c_cc = 0;                           // compute-side position in the (cc, tap) loop nest

  auto chunk_sync = [&](int kc) {
    if (kc + 1 < nk)
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(AI + BI) : "memory");   // chunk kc landed; kc+1 may still fly
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                  // everyone's chunk kc visible; everyone done with chunk kc-1
    asm volatile("" ::: "memory");
  };
  auto read_frags = [&](int stage, float4 (&af)[2][TM], float4 (&bf)[2][TN]) {
    const char* sb = lds + stage * STAGE_B;
#pragma unroll
    for (int t = 0; t < TM; ++t) af[0][t] = *reinterpret_cast<const float4*>(sb + aoff[t]);
#pragma unroll
    for (int u = 0; u < TN; ++u) bf[0][u] = *reinterpret_cast<const float4*>(sb + boff[u]);
#pragma unroll
    for (int t = 0; t < TM; ++t) af[1][t] = *reinterpret_cast<const float4*>(sb + (aoff[t] ^ (MATH ? 16 : 32)));
#pragma unroll
    for (int u = 0; u < TN; ++u) bf[1][u] = *reinterpret_cast<const float4*>(sb + (boff[u] ^ (MATH ? 16 : 32)));
    if (cscale) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int t = 0; t < TM; ++t) {
          const float4 sc = *reinterpret_cast<const float4*>(csrow[t] + c_cc * BK + (MATH ? ks * 4 + khalf * 4 : ks * 8));
          af[ks][t].x *= sc.x;
          af[ks][t].y *= sc.y;
          af[ks][t].z *= sc.z;
          af[ks][t].w *= sc.w;
        }
      if (++c_tap == T_taps) {
        c_tap = 0;
        ++c_cc;
      }
    }
  };

  if (MATH == 0 && nk > 0) {
    issue(0);
    if (nk > 1) issue(1);
    int stage = 0, nstage = 2;                       // nstage: where chunk kc+2 goes
    for (int kc = 0; kc < nk; ++kc) {
      chunk_sync(kc);
      if (kc + 2 < nk) issue(nstage);
      float4 af[2][TM], bf[2][TN];
      read_frags(stage, af, bf);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
        for (int t = 0; t < TM; ++t)
#pragma unroll
          for (int u = 0; u < TN; ++u) acc[t][u] = mfma32f(af[ks][t].x, bf[ks][u].x, acc[t][u]);
#pragma unroll
        for (int t = 0; t < TM; ++t)
#pragma unroll
          for (int u = 0; u < TN; ++u) acc[t][u] = mfma32f(af[ks][t].y, bf[ks][u].y, acc[t][u]);
#pragma unroll
        for (int t = 0; t < TM; ++t)
#pragma unroll
          for (int u = 0; u < TN; ++u) acc[t][u] = mfma32f(af[ks][t].z, bf[ks][u].z, acc[t][u]);
#pragma unroll
        for (int t = 0; t < TM; ++t)
#pragma unroll
          for (int u = 0; u < TN; ++u) acc[t][u] = mfma32f(af[ks][t].w, bf[ks][u].w, acc[t][u]);
      }
      stage = stage == 2 ? 0 : stage + 1;
      nstage = nstage == 2 ? 0 : nstage + 1;
    }
  }
  if (MATH >= 1 && nk > 0) {
    constexpr int PROD = MATH >= 1 ? MATH - 1 : 0;
    // split-bf16: A fragments are split in registers, B was split when it was packed.  (Interleaving the split of
    // chunk kc+1 with the MFMAs of chunk kc by hand measured the same: the loop is bound by LDS-DMA issue and the
    // per-chunk barrier, not by VALU/MFMA overlap -- DESIGN.md.)
    issue(0);
    if (nk > 1) issue(1);
    int stage = 0, nstage = 2;
    for (int kc = 0; kc < nk; ++kc) {
      chunk_sync(kc);
      if (kc + 2 < nk) issue(nstage);
      float4 af[2][TM], bf[2][TN];
      read_frags(stage, af, bf);
      bf16x8_t ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
      for (int t = 0; t < TM; ++t) {
        if (PROD == 0) split_bf16x8(af[0][t], af[1][t], ah[t], al[t]);
        else ah[t] = al[t] = round16x8<PROD>(af[0][t], af[1][t]);
      }
#pragma unroll
      for (int u = 0; u < TN; ++u) {   // weights were split / rounded when they were packed (fast_pack_store)
        bh[u] = __builtin_bit_cast(bf16x8_t, bf[0][u]);
        bl[u] = PROD == 0 ? __builtin_bit_cast(bf16x8_t, bf[1][u]) : bh[u];
      }
#pragma unroll
      for (int i = 0; i < nprod<PROD>() * TM * TN; ++i) {   // product order al*bh, ah*bl, ah*bh; accumulator chains interleaved
        const int grp = PROD == 0 ? i / (TM * TN) : 2, t = (i % (TM * TN)) / TN, u = i % TN;
        acc[t][u] = mma16<PROD>(grp == 0 ? al[t] : ah[t], grp == 1 ? bl[u] : bh[u], acc[t][u]);
      }
      stage = stage == 2 ? 0 : stage + 1;
      nstage = nstage == 2 ? 0 : nstage + 1;
    }
  }

  // ---- epilogue: accumulators -> LDS (per-wave region of the now idle ring) -> row-contiguous float4s:
  // 16-byte loads of bias / mask / residual and 16-byte stores (4 rows x 256 B per wave instruction)
  // instead of 64 scalar stores per lane.  C/D map of the 32x32 MFMA: col = lane&31,
  // row = (r&3) + 8*(r>>2) + 4*(lane>>5).
  const int flags = EPI >= 0 ? EPI : g.flags;
  __syncthreads();                                   // every wave is done reading the ring
  float* wl = reinterpret_cast<float*>(lds) + wave * (32 * WTN);
  constexpr int QPRW = WTN / 4;                      // float4 per tile row
  constexpr int NRD = 32 * QPRW / 64;                // float4 reads per lane per 32-row half
#pragma unroll
  for (int t = 0; t < TM; ++t) {
#pragma unroll
    for (int u = 0; u < TN; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) wl[((r & 3) + 8 * (r >> 2) + 4 * khalf) * WTN + u * 32 + l31] = acc[t][u][r];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");           // wave-private region: no block barrier needed
    constexpr int EB = NRD < 4 ? NRD : 4;               // quads per fetch / finish batch
#pragma unroll
    for (int i0 = 0; i0 < NRD; i0 += EB) {
      float4 vq[EB];
      EpiOps eo[EB];
      unsigned dpx[EB];                                   // pixel index (< 2^31: checked on the host side)
      int nq[EB];
      bool okq[EB];
#pragma unroll
      for (int j = 0; j < EB; ++j) {                    // every global operand of the batch first ...
        const int idx = (i0 + j) * 64 + lane;
        const int row = idx / QPRW, cq = idx - row * QPRW;
        vq[j] = *reinterpret_cast<const float4*>(wl + row * WTN + cq * 4);
        const int m = m0 + wm * WTM + t * 32 + row;
        nq[j] = n0 + wn * WTN + cq * 4;
        okq[j] = m < g.M && nq[j] < g.K;
        size_t dpix = (size_t)(okq[j] ? m : 0);
        if (!g.dst_identity) {
          const int mm = okq[j] ? m : 0;
          const int nimg = mm / OHOW;
          const int rem = mm - nimg * OHOW;
          const int oh = rem / g.OW;
          const int ow = rem - oh * g.OW;
          dpix = ((size_t)nimg * g.Hd + (oh * g.dsd + g.ph)) * g.Wd + (ow * g.dsd + g.pw);
        }
        dpx[j] = (unsigned)dpix;
        if (!okq[j]) nq[j] = 0;
        eo[j] = epi_fetch(dpix, nq[j], flags, g, bias, residual, rowscale, actmask, dst, EPI < 0 && g.accumulate != 0);
      }
#pragma unroll
      for (int j = 0; j < EB; ++j)                      // ... then the arithmetic and the stores (see epi_fetch)
        if (okq[j]) epi_finish(vq[j], eo[j], dpx[j], nq[j], flags, g, dst, EPI < 0 && g.accumulate != 0);
    }
    if (t + 1 < TM) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // reads done before the region is rewritten
  }
}

// ================================================================================================ //
// fprop / dgrad of stride-1 3x3 convolutions in split-bf16 arithmetic: "patch" kernel.
// In fast_conv_dma_kernel every tap re-fetches its own 128-row A tile from L2; at the bf16 MFMA rate the kernel
// is then bound by LDS-DMA issue (4 x 1 KiB per wave per 12 MFMAs), not by the matrix pipe (ablation in
// DESIGN.md).  Here a block owns a PH x PW patch of output pixels (PH*PW <= 128) and keeps the (PH+2) x (PW+2)
// input halo of one 16-channel chunk in LDS; all nine taps read their A fragments from that one patch at shifted
// row addresses, so A traffic drops ~6x and only the B (weight) tile is streamed per tap.  Each wave converts the
// patch pieces it fetched itself from fp32 to the split hi|lo layout IN PLACE (once per element, instead of once
// per fragment read in every tap and wave), so fragments of both operands come out of LDS ready for the MFMA.
//   LDS: 2 patch buffers (chunk cc / cc+1) + a 3-stage ring of B tiles (one tap each), one barrier per tap.
//   Results are bit-identical to fast_conv_dma_kernel<.., MATH 1>: same split, same product and chunk order.
// ================================================================================================ //

template <int BN, int EPI, int PROD = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void conv_patch_kernel(const float* __restrict__ src, const float* __restrict__ wt,
                                                          const float* __restrict__ bias,
                                                          const float* __restrict__ residual,
                                                          const float* __restrict__ actmask, float* __restrict__ dst,
                                                          FastGeom g, PatchGeom pg, int nblk_m, int nblk_n) {
  constexpr int NW = 4, BK = 16;
  constexpr int WTM = 64, WTN = BN / 2;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int BPW = BN / 64;                      // B DMA pieces per wave per tap
  constexpr int MAXP = 3;                           // A patch pieces per wave: 12 pieces = 192 rows per patch
  constexpr int PATCH_B = 12 * 1024;
  constexpr int BSTAGE_B = BN * 64;
  constexpr int EPI_B = NW * 32 * WTN * 4;
  constexpr int LDS_B = 2 * PATCH_B + 3 * BSTAGE_B > EPI_B ? 2 * PATCH_B + 3 * BSTAGE_B : EPI_B;
  __shared__ __attribute__((aligned(1024))) char lds[LDS_B];
  __shared__ int pix_tab[128];                      // lane-row -> (orow << 16 | ocol): patch_pixel (two integer divisions) once per row

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = xcd_tile(blockIdx.x, nblk_m * nblk_n);
  const int tile_n = tile % nblk_n, pid = tile / nblk_n;
  const int n0 = tile_n * BN;
  const int tpi = pg.tiles_h * pg.tiles_w;
  const int img = pid / tpi;
  const int prem = pid - img * tpi;
  const int ty = prem / pg.tiles_w, tx = prem - ty * pg.tiles_w;
  const int oh0 = ty * pg.PH, ow0 = tx * pg.PW;
  const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) char*)lds;
  if (tid < 128) {
    int pr_, pc_;
    patch_pixel(tid, pg.PH, pg.PW, pg.gmap, pr_, pc_);
    pix_tab[tid] = (pr_ << 16) | pc_;
  }
  __syncthreads();

  // ---- A patch DMA: piece p = k*NW + wave covers patch rows 16p .. 16p+15; this lane feeds (row, slot lane&3).
  // Every wave always moves MAXP pieces (rows past the patch come from the zero block and are never read), so the
  // number of DMAs in flight is the same compile-time constant for all waves.
  const int swz = (lane >> 4) & 3;                  // ((16p + lane/4) >> 2) & 3
  const int aq = (lane & 3) ^ swz;                  // global 16-byte quad held by this lane's slot
  int abase[MAXP];
#pragma unroll
  for (int k = 0; k < MAXP; ++k) {
    const int row = (k * NW + wave) * 16 + (lane >> 2);
    abase[k] = -1;
    if (row < pg.PR) {
      const int pi = row / pg.PWP, pj = row - pi * pg.PWP;
      const int sh = oh0 + pg.lo_h + pi, sw = ow0 + pg.lo_w + pj;
      if (sh >= 0 && sh < g.Hs && sw >= 0 && sw < g.Ws) abase[k] = ((img * g.Hs + sh) * g.Ws + sw) * g.lds + aq * 4;
    }
  }
  int bbase[BPW];
  bool bval[BPW];
#pragma unroll
  for (int j = 0; j < BPW; ++j) {
    const int n = n0 + wave * 16 * BPW + 16 * j + (lane >> 2);
    bval[j] = n < g.K;
    bbase[j] = n * g.ldw + aq * 4;                  // ((row >> 2) & 3) == swz here too (16-row pieces)
  }
  const unsigned a_dst = __builtin_amdgcn_readfirstlane(lds_base + wave * 1024);
  const unsigned b_dst = __builtin_amdgcn_readfirstlane(lds_base + 2 * PATCH_B + wave * BPW * 1024);

  const int CC = g.C / BK;
  int wtap[9];                                      // packed-weight column of tap t (scalar registers)
#pragma unroll
  for (int t = 0; t < 9; ++t) wtap[t] = ((g.kh0 + (t / 3) * g.khs) * g.KW + (g.kw0 + (t % 3) * g.kws)) * g.C;

  // DMA through buffer descriptors: lanes that feed padding (outside the image / past the last destination channel)
  // carry an out-of-range offset and the hardware delivers zeros -- one 32-bit add per DMA instead of a 64-bit
  // address and a pointer select (measured -2.5 % on the 64 -> 256 fprop, bit-identical)
  __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(src), 0, g.src_bytes, 0x00020000);
  __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wt), 0, g.w_bytes, 0x00020000);
  unsigned aoffb[MAXP], boffb[BPW];
#pragma unroll
  for (int k = 0; k < MAXP; ++k) aoffb[k] = abase[k] >= 0 ? (unsigned)abase[k] * 4u : F_OOB;
#pragma unroll
  for (int j = 0; j < BPW; ++j) boffb[j] = bval[j] ? (unsigned)bbase[j] * 4u : F_OOB;
  auto issue_a = [&](int buf, int k, int cc) {      // one 1 KiB piece of the patch of chunk cc
    lds_dma16_buf(aoffb[k] + (unsigned)(cc * BK * 4), rs_a, a_dst + buf * PATCH_B + k * (NW * 1024));
  };
  auto issue_b = [&](int stage, int tap, int cc) {  // the B tile of (chunk cc, tap)
    const int wk = wtap[tap] + cc * BK;
#pragma unroll
    for (int j = 0; j < BPW; ++j) lds_dma16_buf(boffb[j] + (unsigned)(wk * 4), rs_b, b_dst + stage * BSTAGE_B + j * 1024);
  };
  // fp32 -> split bf16 in place for one piece this wave fetched: lanes 2i, 2i+1 hold the two quads (8 consecutive
  // channels) of a half row; the lane with the even quad keeps the 8 hi halves, the odd one the 8 lo halves
  auto convert_piece = [&](int buf, int k) {
    float4* slot = reinterpret_cast<float4*>(lds + buf * PATCH_B + (k * NW + wave) * 1024 + lane * 16);
    const float4 own = *slot;
    float4 oth;
    oth.x = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, own.x), 0xB1, 0xF, 0xF, true));
    oth.y = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, own.y), 0xB1, 0xF, 0xF, true));
    oth.z = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, own.z), 0xB1, 0xF, 0xF, true));
    oth.w = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, own.w), 0xB1, 0xF, 0xF, true));
    const bool odd = aq & 1;                        // this lane's quad is the second half of the 8-group
    bf16x8_t hi, lo;
    if (PROD == 0) {
      split_bf16x8(odd ? oth : own, odd ? own : oth, hi, lo);
      *reinterpret_cast<bf16x8_t*>(slot) = odd ? lo : hi;
    } else if (!odd) {                              // single product: the even lane's slot takes the 8 rounded values
      *reinterpret_cast<bf16x8_t*>(slot) = round16x8<PROD>(own, oth);
    }
  };

  // prologue DMAs first (whole patch of chunk 0, B tiles of taps 0 and 1): the address tables below are computed under their latency
#pragma unroll
  for (int k = 0; k < MAXP; ++k) issue_a(0, k, 0);
  issue_b(0, 0, 0);
  issue_b(1, 1, 0);

  // ---- fragment addressing: everything but the patch-buffer parity is fixed for the whole kernel ----
  const int wm = wave >> 1, wn = wave & 1;
  const int khalf = lane >> 5, l31 = lane & 31;
  int aoff[9][TM];                                  // byte offset (buffer 0) of this lane's hi quad for tap t
#pragma unroll
  for (int t = 0; t < TM; ++t) {
    const int r = wm * WTM + t * 32 + l31;
    const int pt = pix_tab[r];
    const int orow = pt >> 16, ocol = pt & 0xffff;
    const int arow = orow < pg.PH ? orow * pg.PWP + ocol : 0;   // dead rows read pixel 0, never stored
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int a_th = (g.dh0 + (tap / 3) * g.dhs) - pg.lo_h, a_tw = (g.dw0 + (tap % 3) * g.dws) - pg.lo_w;
      const int pr = arow + a_th * pg.PWP + a_tw;
      aoff[tap][t] = pr * 64 + (((2 * khalf) ^ ((pr >> 2) & 3)) << 4);
    }
  }
  int boff[TN];
#pragma unroll
  for (int u = 0; u < TN; ++u) {
    const int row = wn * WTN + u * 32 + l31;
    boff[u] = 2 * PATCH_B + row * 64 + (((2 * khalf) ^ ((row >> 2) & 3)) << 4);
  }
  f32x16 acc[TM][TN];
#pragma unroll
  for (int t = 0; t < TM; ++t)
#pragma unroll
    for (int u = 0; u < TN; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][u][r] = 0.f;

  // One tap of one chunk.  TAP and LAST (= this is the final chunk) are compile-time, so which DMAs are issued,
  // which piece is converted, the ring slots and the vmcnt count are all immediates: the loop body is a straight
  // line of [wait, barrier, <= 3 DMAs, 8 ds_read_b128, 12 MFMAs].
  //   DMA order inside a tap: the A piece (taps 0..2, for chunk cc+1), then the B tile of tap+2.
  //   At tap t the B tile of t (issued at t-2) must have landed; issued after it: the A piece of tap t-1 (if any)
  //   and the B tile of t+1 (if any) -> that many DMAs may stay in flight.
  auto do_tap = [&](auto tapc, auto lastc, int cc) {
    constexpr int TAP = decltype(tapc)::value;
    constexpr bool LAST = decltype(lastc)::value != 0;
    constexpr int NEWER = ((LAST && TAP == 8) ? 0 : BPW) + ((!LAST && TAP >= 1 && TAP <= MAXP) ? 1 : 0);
    wait_vmcnt<NEWER>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's in-place conversions are in LDS
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const int pbuf = cc & 1;
    if (!LAST && TAP < MAXP) issue_a(pbuf ^ 1, TAP, cc + 1);
    if (TAP + 2 < 9) issue_b((TAP + 2) % 3, TAP + 2, cc);
    else if (!LAST) issue_b((TAP + 2) % 3, TAP + 2 - 9, cc + 1);
    if (!LAST && TAP >= 2 && TAP - 2 < MAXP) convert_piece(pbuf ^ 1, TAP - 2);   // landed: it is older than B tile TAP
    const char* pb = lds + pbuf * PATCH_B;
    const char* sb = lds + (TAP % 3) * BSTAGE_B;
    bf16x8_t ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
    for (int t = 0; t < TM; ++t) {
      ah[t] = *reinterpret_cast<const bf16x8_t*>(pb + aoff[TAP][t]);
      al[t] = PROD == 0 ? *reinterpret_cast<const bf16x8_t*>(pb + (aoff[TAP][t] ^ 16)) : ah[t];
    }
#pragma unroll
    for (int u = 0; u < TN; ++u) {
      bh[u] = *reinterpret_cast<const bf16x8_t*>(sb + boff[u]);
      bl[u] = PROD == 0 ? *reinterpret_cast<const bf16x8_t*>(sb + (boff[u] ^ 16)) : bh[u];
    }
#pragma unroll
    for (int i = 0; i < nprod<PROD>() * TM * TN; ++i) {   // same product order as fast_conv_dma_kernel
      const int grp = PROD == 0 ? i / (TM * TN) : 2, t = (i % (TM * TN)) / TN, u = i % TN;
      acc[t][u] = mma16<PROD>(grp == 0 ? al[t] : ah[t], grp == 1 ? bl[u] : bh[u], acc[t][u]);
    }
  };
  auto do_chunk = [&](auto lastc, int cc) {
    do_tap(IC<0>(), lastc, cc);
    do_tap(IC<1>(), lastc, cc);
    do_tap(IC<2>(), lastc, cc);
    do_tap(IC<3>(), lastc, cc);
    do_tap(IC<4>(), lastc, cc);
    do_tap(IC<5>(), lastc, cc);
    do_tap(IC<6>(), lastc, cc);
    do_tap(IC<7>(), lastc, cc);
    do_tap(IC<8>(), lastc, cc);
  };

  // (prologue DMAs: issued above, before the fragment tables) convert the patch once B tile 0 (issued after it) is in
  wait_vmcnt<BPW>();
#pragma unroll
  for (int k = 0; k < MAXP; ++k) convert_piece(0, k);
  for (int cc = 0; cc + 1 < CC; ++cc) do_chunk(IC<0>(), cc);
  do_chunk(IC<1>(), CC - 1);

  // ---- epilogue (as fast_conv_dma_kernel): accumulators -> wave-private LDS -> row-contiguous float4s ----
  const int flags = EPI >= 0 ? EPI : g.flags;
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
    constexpr int EB = NRD < 4 ? NRD : 4;               // quads per fetch / finish batch (register budget: 17 values per quad at most)
#pragma unroll
    for (int i0 = 0; i0 < NRD; i0 += EB) {
      float4 vq[EB];
      EpiOps eo[EB];
      unsigned dpx[EB];                                   // pixel index (< 2^31: checked on the host side)
      int nq[EB];
      bool okq[EB];
#pragma unroll
      for (int j = 0; j < EB; ++j) {                    // every global operand of the batch first (epi_fetch) ...
        const int idx = (i0 + j) * 64 + lane;
        const int row = idx / QPRW, cq = idx - row * QPRW;
        vq[j] = *reinterpret_cast<const float4*>(wl + row * WTN + cq * 4);
        const int r = wm * WTM + t * 32 + row;
        const int pt = pix_tab[r];
        const int orow = pt >> 16, ocol = pt & 0xffff;
        const int oh = oh0 + orow, ow = ow0 + ocol;
        const int n = n0 + wn * WTN + cq * 4;
        okq[j] = !(orow >= pg.PH || oh >= g.OH || ow >= g.OW || n >= g.K);
        dpx[j] = okq[j] ? (unsigned)((img * g.Hd + oh) * g.Wd + ow) : 0u;
        nq[j] = okq[j] ? n : 0;
        eo[j] = epi_fetch(dpx[j], nq[j], flags, g, bias, residual, nullptr, actmask, dst, false);   // (the patch path never accumulates)
      }
#pragma unroll
      for (int j = 0; j < EB; ++j)                      // ... then the arithmetic and the stores
        if (okq[j]) epi_finish(vq[j], eo[j], dpx[j], nq[j], flags, g, dst, false);
    }
    if (t + 1 < TM) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
}

// ================================================================================================ //
// K-split form of the one-tile patch kernel for 64 destination channels (round 4): conv2's fprop (256 -> 64) and conv1's dgrad.
// With BN = 64 the 2 x 2 wave grid above gives a wave 64 pixels x 32 channels: 6 MFMAs for 6 ds_read_b128 per tap, against 12 for
// 8 in the 128-wide tile -- the fragment reads of three blocks per CU then take as long as their MFMAs (12 waves x 6 x 8 clk of
// LDS against 3 waves x 6 x 32 clk per SIMD), which is why these convs sat at 0.40 while the wide ones reached 0.44.  Here the
// second wave column splits K instead of N: wave (wm, wk) owns 64 pixels x ALL 64 channels and every second tap of the
// (chunk, tap) sequence -- T = 2 s + wk at step s --, so a step is one barrier, 8 fragment reads and 12 MFMAs per wave, like the
// wide tile.  The tap sequence of a PAIR of 16-channel chunks (18 taps, 9 steps) is the unit of the compile-time schedule: the
// patch of the pair's second chunk arrives during steps 0-1, the next pair's first patch during steps 5-6, weight tiles run
// four taps ahead in a six-slot ring (T mod 6: the pattern repeats per pair).  At the end the two K halves are added through LDS
// (each wave hands its partner the 32 channels the partner stores), then the usual epilogue.  The sum is grouped differently
// from fast_conv_dma_kernel's (two partial sums per output), so results agree with it to rounding, not bit for bit.
// Requires an even number of chunks (C % 32 == 0).
// ================================================================================================ //
template <int EPI>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void conv_patch_ks_kernel(
    const float* __restrict__ src, const float* __restrict__ wt, const float* __restrict__ bias, const float* __restrict__ residual,
    const float* __restrict__ actmask, float* __restrict__ dst, FastGeom g, PatchGeom pg, int nblk_m, int nblk_n) {
  constexpr int BN = 64, NW = 4, BK = 16, TM = 2, TN = 2, MAXP = 3, NST = 6;
  constexpr int PATCH_B = 12 * 1024, BSTAGE_B = BN * 64;
  constexpr int LDS_B = 2 * PATCH_B + NST * BSTAGE_B;          // 48 KB (the K exchange takes 32 KB of it, the epilogue 16 KB)
  __shared__ __attribute__((aligned(1024))) char lds[LDS_B];
  __shared__ int pix_tab[128];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = xcd_tile(blockIdx.x, nblk_m * nblk_n);
  const int tile_n = tile % nblk_n, pid = tile / nblk_n;
  const int n0 = tile_n * BN;
  const int tpi = pg.tiles_h * pg.tiles_w;
  const int img = pid / tpi;
  const int prem = pid - img * tpi;
  const int ty = prem / pg.tiles_w, tx = prem - ty * pg.tiles_w;
  const int oh0 = ty * pg.PH, ow0 = tx * pg.PW;
  const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) char*)lds;
  if (tid < 128) {
    int pr_, pc_;
    patch_pixel(tid, pg.PH, pg.PW, pg.gmap, pr_, pc_);
    pix_tab[tid] = (pr_ << 16) | pc_;
  }
  __syncthreads();

  const int swz = (lane >> 4) & 3;
  const int aq = (lane & 3) ^ swz;
  unsigned aoffb[MAXP];
#pragma unroll
  for (int k = 0; k < MAXP; ++k) {
    const int row = (k * NW + wave) * 16 + (lane >> 2);
    aoffb[k] = F_OOB;
    if (row < pg.PR) {
      const int pi = row / pg.PWP, pj = row - pi * pg.PWP;
      const int sh = oh0 + pg.lo_h + pi, sw = ow0 + pg.lo_w + pj;
      if (sh >= 0 && sh < g.Hs && sw >= 0 && sw < g.Ws) aoffb[k] = (unsigned)(((img * g.Hs + sh) * g.Ws + sw) * g.lds + aq * 4) * 4u;
    }
  }
  unsigned boffb;
  {
    const int n = n0 + wave * 16 + (lane >> 2);
    boffb = n < g.K ? (unsigned)(n * g.ldw + aq * 4) * 4u : F_OOB;
  }
  const unsigned a_dst = __builtin_amdgcn_readfirstlane(lds_base + wave * 1024);
  const unsigned b_dst = __builtin_amdgcn_readfirstlane(lds_base + 2 * PATCH_B + wave * 1024);
  const int CC = g.C / BK;
  int wtap[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) wtap[t] = ((g.kh0 + (t / 3) * g.khs) * g.KW + (g.kw0 + (t % 3) * g.kws)) * g.C;
  __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(src), 0, g.src_bytes, 0x00020000);
  __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wt), 0, g.w_bytes, 0x00020000);
  auto issue_a = [&](int buf, int k, int cc) {
    lds_dma16_buf(aoffb[k] + (unsigned)(cc * BK * 4), rs_a, a_dst + buf * PATCH_B + k * (NW * 1024));
  };
  auto issue_b = [&](int stage, int tap, int cc) {
    lds_dma16_buf(boffb + (unsigned)((wtap[tap] + cc * BK) * 4), rs_b, b_dst + stage * BSTAGE_B);
  };
  auto convert_piece = [&](int buf, int k) {          // as in conv_patch_kernel (split-bf16)
    float4* slot = reinterpret_cast<float4*>(lds + buf * PATCH_B + (k * NW + wave) * 1024 + lane * 16);
    const float4 own = *slot;
    float4 oth;
    oth.x = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, own.x), 0xB1, 0xF, 0xF, true));
    oth.y = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, own.y), 0xB1, 0xF, 0xF, true));
    oth.z = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, own.z), 0xB1, 0xF, 0xF, true));
    oth.w = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, own.w), 0xB1, 0xF, 0xF, true));
    const bool odd = aq & 1;
    bf16x8_t hi, lo;
    split_bf16x8(odd ? oth : own, odd ? own : oth, hi, lo);
    *reinterpret_cast<bf16x8_t*>(slot) = odd ? lo : hi;
  };

  // prologue DMAs first -- the patch of chunk 0, the weight tiles of taps 0..3 --, so that the address tables below (54 offsets,
  // two integer divisions per row) are computed under their latency: every block of a one-round launch pays this prologue at
  // the same time, with nothing else on the chip to hide it
#pragma unroll
  for (int k = 0; k < MAXP; ++k) issue_a(0, k, 0);
  issue_b(0, 0, 0);
  issue_b(1, 1, 0);
  issue_b(2, 2, 0);
  issue_b(3, 3, 0);

  // ---- fragment addressing by STEP: this wave's tap at step s of a chunk pair is T = 2 s + wk (chunk T / 9, tap T % 9) ----
  const int wm = wave >> 1, wk = wave & 1;
  const int khalf = lane >> 5, l31 = lane & 31;
  int aoffS[9][TM];                                 // byte offset of the hi quad, patch buffer (= chunk parity) included
#pragma unroll
  for (int t = 0; t < TM; ++t) {
    const int r = wm * 64 + t * 32 + l31;
    const int pt = pix_tab[r];
    const int orow = pt >> 16, ocol = pt & 0xffff;
    const int arow = orow < pg.PH ? orow * pg.PWP + ocol : 0;
#pragma unroll
    for (int sidx = 0; sidx < 9; ++sidx) {
      const int T = 2 * sidx + wk;
      const int par = T >= 9 ? 1 : 0, tap = T - 9 * par;
      const int th = tap / 3, tw = tap - 3 * th;
      const int a_th = (g.dh0 + th * g.dhs) - pg.lo_h, a_tw = (g.dw0 + tw * g.dws) - pg.lo_w;
      const int pr = arow + a_th * pg.PWP + a_tw;
      aoffS[sidx][t] = par * PATCH_B + pr * 64 + (((2 * khalf) ^ ((pr >> 2) & 3)) << 4);
    }
  }
  int boffk[TN];                                    // ring base + this K group's slot of a step's pair + the fragment row
#pragma unroll
  for (int u = 0; u < TN; ++u) {
    const int row = u * 32 + l31;
    boffk[u] = 2 * PATCH_B + wk * BSTAGE_B + row * 64 + (((2 * khalf) ^ ((row >> 2) & 3)) << 4);
  }
  f32x16 acc[TM][TN];
#pragma unroll
  for (int t = 0; t < TM; ++t)
#pragma unroll
    for (int u = 0; u < TN; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][u][r] = 0.f;

  // One step of a chunk pair (compile-time step index and "last pair" flag: every DMA, conversion, ring slot and vmcnt count is
  // an immediate).  DMAs per wave and step: s0 A A B B | s1 A B B | s2-s4 B B | s5 A A B B | s6 A B B | s7, s8 B B; the last pair
  // drops the next pair's patch (s5, s6) and weight tiles (s7, s8).  At step s the weight tiles of taps 2 s and 2 s + 1 (the last
  // two DMAs of step s - 2) must have landed: everything issued at step s - 1 may stay in flight.
  auto do_step = [&](auto sc, auto lastc, int cc0) {
    constexpr int S = decltype(sc)::value;
    constexpr bool LAST = decltype(lastc)::value != 0;
    constexpr int NEWER = S == 0 ? 2 : S == 1 ? 4 : S == 2 ? 3 : (S >= 3 && S <= 5) ? 2 : S == 6 ? (LAST ? 2 : 4) : S == 7 ? (LAST ? 2 : 3) : (LAST ? 0 : 2);
    wait_vmcnt<NEWER>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (S == 0) {
      issue_a(1, 0, cc0 + 1);
      issue_a(1, 1, cc0 + 1);
    }
    if (S == 1) issue_a(1, 2, cc0 + 1);
    if (!LAST && S == 5) {
      issue_a(0, 0, cc0 + 2);
      issue_a(0, 1, cc0 + 2);
    }
    if (!LAST && S == 6) issue_a(0, 2, cc0 + 2);
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      constexpr int T0 = 2 * S + 4;
      const int T = T0 + d;
      if (T < 18) issue_b(T % NST, T % 9, cc0 + T / 9);
      else if (!LAST) issue_b(T % NST, (T - 18) % 9, cc0 + 2 + (T - 18) / 9);
    }
    if (S == 2) {
      convert_piece(1, 0);
      convert_piece(1, 1);
    }
    if (S == 3) convert_piece(1, 2);
    if (!LAST && S == 7) {
      convert_piece(0, 0);
      convert_piece(0, 1);
    }
    if (!LAST && S == 8) convert_piece(0, 2);
    const char* sb = lds + ((2 * S) % NST) * BSTAGE_B;
    bf16x8_t ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
    for (int t = 0; t < TM; ++t) {
      ah[t] = *reinterpret_cast<const bf16x8_t*>(lds + aoffS[S][t]);
      al[t] = *reinterpret_cast<const bf16x8_t*>(lds + (aoffS[S][t] ^ 16));
    }
#pragma unroll
    for (int u = 0; u < TN; ++u) {
      bh[u] = *reinterpret_cast<const bf16x8_t*>(sb + boffk[u]);
      bl[u] = *reinterpret_cast<const bf16x8_t*>(sb + (boffk[u] ^ 16));
    }
#pragma unroll
    for (int i = 0; i < 3 * TM * TN; ++i) {         // same product order as the other split-bf16 kernels: al*bh, ah*bl, ah*bh
      const int grp = i / (TM * TN), t = (i % (TM * TN)) / TN, u = i % TN;
      acc[t][u] = mma16<0>(grp == 0 ? al[t] : ah[t], grp == 1 ? bl[u] : bh[u], acc[t][u]);
    }
  };
  auto do_pair = [&](auto lastc, int cc0) {
    do_step(IC<0>(), lastc, cc0);
    do_step(IC<1>(), lastc, cc0);
    do_step(IC<2>(), lastc, cc0);
    do_step(IC<3>(), lastc, cc0);
    do_step(IC<4>(), lastc, cc0);
    do_step(IC<5>(), lastc, cc0);
    do_step(IC<6>(), lastc, cc0);
    do_step(IC<7>(), lastc, cc0);
    do_step(IC<8>(), lastc, cc0);
  };

  // (prologue DMAs: issued above, before the fragment tables) the patch is converted once it is in; the weight tiles stay in flight
  wait_vmcnt<4>();
#pragma unroll
  for (int k = 0; k < MAXP; ++k) convert_piece(0, k);
  for (int cc0 = 0; cc0 + 2 < CC; cc0 += 2) do_pair(IC<0>(), cc0);
  do_pair(IC<1>(), CC - 2);

  // ---- add the two K halves: a wave hands its partner (same pixels, other K group) the 32 channels the partner stores ----
  __syncthreads();
  {
    float* xl = reinterpret_cast<float*>(lds);
#pragma unroll
    for (int t = 0; t < TM; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) xl[((wave * TM + t) * 16 + r) * 64 + lane] = wk ? acc[t][0][r] : acc[t][1][r];
    __syncthreads();
    const int pw = wave ^ 1;
#pragma unroll
    for (int t = 0; t < TM; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float o = xl[((pw * TM + t) * 16 + r) * 64 + lane];
        acc[t][0][r] = (wk ? acc[t][1][r] : acc[t][0][r]) + o;
      }
    __syncthreads();
  }

  // ---- epilogue: as conv_patch_kernel<64> with wn = wk (wave = 64 pixels x 32 channels) ----
  const int flags = EPI >= 0 ? EPI : g.flags;
  constexpr int WTN = 32;
  float* wl = reinterpret_cast<float*>(lds) + wave * (32 * WTN);
  constexpr int QPRW = WTN / 4;
  constexpr int NRD = 32 * QPRW / 64;
#pragma unroll
  for (int t = 0; t < TM; ++t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) wl[((r & 3) + 8 * (r >> 2) + 4 * khalf) * WTN + l31] = acc[t][0][r];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    float4 vq[NRD];
    EpiOps eo[NRD];
    unsigned dpx[NRD];
    int nq[NRD];
    bool okq[NRD];
#pragma unroll
    for (int j = 0; j < NRD; ++j) {
      const int idx = j * 64 + lane;
      const int row = idx / QPRW, cq = idx - row * QPRW;
      vq[j] = *reinterpret_cast<const float4*>(wl + row * WTN + cq * 4);
      const int r = wm * 64 + t * 32 + row;
      const int pt = pix_tab[r];
      const int orow = pt >> 16, ocol = pt & 0xffff;
      const int oh = oh0 + orow, ow = ow0 + ocol;
      const int n = n0 + wk * WTN + cq * 4;
      okq[j] = !(orow >= pg.PH || oh >= g.OH || ow >= g.OW || n >= g.K);
      dpx[j] = okq[j] ? (unsigned)((img * g.Hd + oh) * g.Wd + ow) : 0u;
      nq[j] = okq[j] ? n : 0;
      eo[j] = epi_fetch(dpx[j], nq[j], flags, g, bias, residual, nullptr, actmask, dst, false);
    }
#pragma unroll
    for (int j = 0; j < NRD; ++j)
      if (okq[j]) epi_finish(vq[j], eo[j], dpx[j], nq[j], flags, g, dst, false);
    if (t + 1 < TM) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
}

// ================================================================================================ //
// Stride-1 3x3 convolutions with <= 4 destination channels (generator tail conv 64 -> 3, discriminator head dgrad
// 64 -> 3) at full image size.  A 32-wide MFMA tile wastes 10x the arithmetic there and the op is HBM-bound
// (one read of the source); this kernel does the 1728 multiply-adds per pixel on the VALU in exact fp32:
//   * a block owns a 16 x 16 patch of output pixels, one thread per pixel, ND accumulators each;
//   * the 18 x 18 halo of a 16-channel chunk is staged in LDS (double-buffered, coalesced 16-byte loads,
//     16-byte slots XOR-swizzled by the pixel index so the nine shifted ds_read_b128 streams are conflict-free);
//   * weights are indexed uniformly, so they arrive through scalar loads and enter the FMAs as SGPR operands.
// MASK (64 dense source channels): `smask` holds one 64-bit word per source pixel, bit c = 1 where the LeakyReLU that follows the
// conv whose data gradient this is let channel c through (headconv_fwd_kernel<1>'s record).  A thread keeps the words of the <= 6
// pixels it stages and multiplies each staged float4 by the mask of its four channels (v = bit ? v : v * slope) before it goes to
// LDS: the activation's backward costs 8 bytes per pixel here instead of a pass that reads dy and y and writes g.
// ================================================================================================ //
template <int ND, bool MASK>
__global__ __launch_bounds__(256) void narrow_conv_kernel(const float* __restrict__ src, const float* __restrict__ wt,
                                                           const float* __restrict__ bias, float* __restrict__ dst,
                                                           FastGeom g, int tiles_h, int tiles_w, int lo_h, int lo_w,
                                                           const unsigned long long* __restrict__ smask) {
  constexpr int PW = 16, PH = 16, PWP = PW + 2, PR = (PH + 2) * PWP;   // 324 patch rows of 64 B
  __shared__ __attribute__((aligned(16))) float4 lds[2][PR * 4];
  const int tid = threadIdx.x;
  const int tpi = tiles_h * tiles_w;
  const int img = blockIdx.x / tpi;
  const int prem = blockIdx.x - img * tpi;
  const int ty = prem / tiles_w, tx = prem - ty * tiles_w;
  const int oh0 = ty * PH, ow0 = tx * PW;
  const int py = tid >> 4, px = tid & 15;

  // staging: 324 rows x 4 quads = 1296 float4 per chunk, 256 threads -> 6 per thread (last partially)
  int soff[6];
  int sdst[6];
  unsigned long long mw[MASK ? 6 : 1];                 // MASK: the record words of the pixels this thread stages
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int e = tid + i * 256;
    soff[i] = -1;
    sdst[i] = 0;
    if (MASK) mw[i] = 0ull;
    if (e < PR * 4) {
      const int row = e >> 2, q = e & 3;
      const int pi = row / PWP, pj = row - pi * PWP;
      const int sh = oh0 + lo_h + pi, sw = ow0 + lo_w + pj;
      sdst[i] = row * 4 + (q ^ (row & 3));
      if (sh >= 0 && sh < g.Hs && sw >= 0 && sw < g.Ws) {
        soff[i] = ((img * g.Hs + sh) * g.Ws + sw) * g.lds + q * 4;
        if (MASK) mw[i] = smask[(img * g.Hs + sh) * g.Ws + sw];
      } else {
        soff[i] = -2;                                  // inside the patch, outside the image: zero
      }
    }
  }
  const int CC = g.C / 16;
  float4 stage[6];
  auto fetch = [&](int cc) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      stage[i] = soff[i] >= 0 ? *reinterpret_cast<const float4*>(src + (size_t)soff[i] + cc * 16) : make_float4(0.f, 0.f, 0.f, 0.f);
      if (MASK) {                                      // channels cc * 16 + q * 4 .. + 3 of the pixel (q = tid & 3 for every i); zeros stay zero
        const unsigned b = (unsigned)(mw[i] >> (cc * 16 + (tid & 3) * 4));
        stage[i].x = (b & 1u) ? stage[i].x : stage[i].x * g.slope;
        stage[i].y = (b & 2u) ? stage[i].y : stage[i].y * g.slope;
        stage[i].z = (b & 4u) ? stage[i].z : stage[i].z * g.slope;
        stage[i].w = (b & 8u) ? stage[i].w : stage[i].w * g.slope;
      }
    }
  };
  auto commit = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 6; ++i)
      if (soff[i] != -1) lds[buf][sdst[i]] = stage[i];
  };
  float acc[ND];
#pragma unroll
  for (int n = 0; n < ND; ++n) acc[n] = 0.f;

  fetch(0);
  commit(0);
  __syncthreads();
  for (int cc = 0; cc < CC; ++cc) {
    const int buf = cc & 1;
    if (cc + 1 < CC) fetch(cc + 1);
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {              // not unrolled: one tap's 16 x ND weights fit the SGPR file
      {
        const int th = tap / 3, tw = tap - th * 3;
        const int a_th = (g.dh0 + th * g.dhs) - lo_h, a_tw = (g.dw0 + tw * g.dws) - lo_w;
        const int row = (py + a_th) * PWP + px + a_tw;
        const int wk = ((g.kh0 + th * g.khs) * g.KW + (g.kw0 + tw * g.kws)) * g.C + cc * 16;   // uniform
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 v = lds[buf][row * 4 + (q ^ (row & 3))];
#pragma unroll
          for (int n = 0; n < ND; ++n) {
            const float* w = wt + (size_t)n * g.ldw + wk + q * 4;                              // scalar loads
            acc[n] = fmaf(v.x, w[0], acc[n]);
            acc[n] = fmaf(v.y, w[1], acc[n]);
            acc[n] = fmaf(v.z, w[2], acc[n]);
            acc[n] = fmaf(v.w, w[3], acc[n]);
          }
        }
      }
    }
    if (cc + 1 < CC) commit(buf ^ 1);
    __syncthreads();
  }
  const int oh = oh0 + py, ow = ow0 + px;
  if (oh < g.OH && ow < g.OW) {
    const size_t dpix = ((size_t)img * g.Hd + oh) * g.Wd + ow;
#pragma unroll
    for (int n = 0; n < ND; ++n) {
      if (n < g.K) {
        float v = acc[n];
        if (g.flags & SRHIP_EPI_BIAS) v += bias[n];
        if (g.flags & SRHIP_EPI_LRELU) v = v > 0.f ? v : v * g.slope;
        dst[dpix * g.ldd + n] = v;
      }
    }
  }
}

// ================================================================================================ //
// ONE destination channel on a small grid (the discriminator's head conv 512 -> 1 at 14 x 14: 6272 output pixels, 4608
// multiply-adds each).  The MFMA kernels pad the channel to a 32-wide tile and have 49 blocks to offer, each walking 288
// K chunks serially: 230 us for 58 MFLOP, three times per step in the discriminator's serial chain.  Here a wave owns an
// output pixel: lanes stride the source channels with 16-byte loads (x row and weight row are both contiguous), fp32
// FMAs, one butterfly reduction.  Exact fp32 in every arithmetic mode.
// ================================================================================================ //
__global__ __launch_bounds__(256) void dot_conv_kernel(const float* __restrict__ src, const float* __restrict__ wt,
                                                        const float* __restrict__ bias, float* __restrict__ dst, FastGeom g) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= g.M) return;
  const int ow = m % g.OW, t = m / g.OW;
  const int oh = t % g.OH, n = t / g.OH;
  float acc = 0.f;
  for (int th = 0; th < g.TH; ++th) {
    const int sh = oh * g.ss + g.dh0 + th * g.dhs;
    if (sh < 0 || sh >= g.Hs) continue;
    for (int tw = 0; tw < g.TW; ++tw) {
      const int sw = ow * g.ss + g.dw0 + tw * g.dws;
      if (sw < 0 || sw >= g.Ws) continue;
      const float* xp = src + ((size_t)(n * g.Hs + sh) * g.Ws + sw) * g.lds;
      const float* wp = wt + (size_t)((g.kh0 + th * g.khs) * g.KW + (g.kw0 + tw * g.kws)) * g.C;
      for (int c = lane * 4; c < g.C; c += 256) {
        const float4 a = *reinterpret_cast<const float4*>(xp + c);
        const float4 b = *reinterpret_cast<const float4*>(wp + c);
        acc = fmaf(a.x, b.x, acc);
        acc = fmaf(a.y, b.y, acc);
        acc = fmaf(a.z, b.z, acc);
        acc = fmaf(a.w, b.w, acc);
      }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) {
    float v = acc;
    if (g.flags & SRHIP_EPI_BIAS) v += bias[0];
    if (g.flags & SRHIP_EPI_LRELU) v = v > 0.f ? v : v * g.slope;
    dst[((size_t)(n * g.Hd + oh * g.dsd + g.ph) * g.Wd + ow * g.dsd + g.pw) * g.ldd] = v;
  }
}

// ---- weight packer of the fast path and the shape predicates that decide who takes it (conv_internal.h: the four sections) ----
// OIHW -> n-major packed GEMM operand.
// mode 0 (fprop): P[co][(kh*KW+kw)*Cin + ci]  = w[co][ci][kh][kw]
// mode 1 (dgrad): P[ci][(kh*KW+kw)*Cout + co] = w[co][ci][kh][kw]
__global__ void fast_pack_kernel(const float* __restrict__ w, float* __restrict__ packed, int cout, int cin, int kh,
                                 int kw, int mode) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int total = cout * cin * kh * kw;
  if (idx >= total) return;
  const int khkw = kh * kw;
  if (mode == 0) {
    const int co = idx / (khkw * cin);
    const int rem = idx - co * khkw * cin;
    const int tap = rem / cin, ci = rem - tap * cin;
    fast_pack_store(packed, total, idx, w[((size_t)co * cin + ci) * khkw + tap], cout, cin, khkw);
  } else {
    const int ci = idx / (khkw * cout);
    const int rem = idx - ci * khkw * cout;
    const int tap = rem / cout, co = rem - tap * cout;
    fast_pack_store(packed, total, idx, w[((size_t)co * cin + ci) * khkw + tap], cin, cout, khkw);
  }
}

static bool shape_ok(int csrc, int kh, int kw) { return csrc % 16 == 0 && kh * kw <= 32 && kh == kw; }
bool fast_fwd_ok(int cin, int cout, int kh, int kw) { return shape_ok(cin, kh, kw); }
bool fast_dgrad_ok(int cin, int cout, int kh, int kw) { return shape_ok(cout, kh, kw); }
bool fast_wgrad_ok(int cin, int cout, int kh, int kw) { return cin % 16 == 0 && cout % 4 == 0 && kh == kw; }

int fast_pack_weight(const float* w, float* packed, int cout, int cin, int kh, int kw, int mode, hipStream_t st) {
  const long total = (long)cout * cin * kh * kw;
  hipLaunchKernelGGL(fast_pack_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, w, packed, cout, cin, kh, kw, mode);
  return check_launch("fast_pack_weight");
}

// ================================================================================================ //
// host side: choose_fprop_route says which kernel a call takes, launch_fprop launches it
// ================================================================================================ //
thread_local RouteLog g_route_log;
thread_local Dst2Request g_dst2_req;
thread_local ResRequest g_res_req;
thread_local PhaseRequest g_phase_req;
thread_local SrcMaskRequest g_src_mask_req;
int g_conv_math = 0;     // SRHIP_MATH_*: 0 exact fp32 MFMA; 1 split-bf16 x3 MFMA; 2 one 16-bit product (fp16 activations / bf16 gradients)
int g_patch_ks = 1;      // srhip_debug_set(10, v): 0 = conv_patch_kernel<64> instead of conv_patch_ks_kernel (bit-identical to the DMA kernel; A/B and pinned tests)
int g_fast_cfg = 0;      // srhip_debug_set(0, cfg): a FastCfg value (conv_dev.h), 0 = the heuristic of choose_fprop_route
int g_phase_batch = 1;   // srhip_debug_set(17, v): 1 = the phases of a stride-2 data gradient as one launch of the LDS-DMA kernel

// Patch shape for conv_patch_kernel: PH x PW output pixels per block (<= 128), halo patch <= 192 rows = 12 DMA pieces; picks the
// shape that wastes the fewest of the 128 GEMM rows over the whole image (halo patch <= 192 rows = 12 DMA pieces).  Only stride-1 3x3 geometries.
static bool plan_patch(const FastGeom& g, PatchGeom* pg, double min_eff = 0.70) {
  if (g.TH != 3 || g.TW != 3 || g.ss != 1 || g.dsd != 1 || g.ph != 0 || g.pw != 0) return false;
  if ((g.dhs != 1 && g.dhs != -1) || (g.dws != 1 && g.dws != -1)) return false;
  if (g.Hd != g.OH || g.Wd != g.OW) return false;
  double best = 0.0;
  for (int pw = 4; pw <= 64 && pw <= g.OW + 3; ++pw) {
    int ph = 128 / pw;
    if (ph > g.OH) ph = g.OH;
    if (ph < 1 || (ph + 2) * (pw + 2) > 192) continue;
    const long tiles = (long)cdiv(g.OH, ph) * cdiv(g.OW, pw);
    // among equally efficient shapes prefer the one whose rows are mostly whole 16-pixel runs: those lane groups read
    // the patch without LDS bank conflicts (patch_pixel)
    const double eff = (double)g.OH * g.OW / ((double)tiles * 128.0) + 1e-6 * (double)(pw - pw % 16) / pw;
    if (eff > best + 1e-9) {
      best = eff;
      pg->PH = ph; pg->PW = pw;
    }
  }
  if (best < min_eff || best <= 0.0) return false;
  pg->tiles_h = cdiv(g.OH, pg->PH);
  pg->tiles_w = cdiv(g.OW, pg->PW);
  pg->PWP = pg->PW + 2;
  pg->PR = (pg->PH + 2) * pg->PWP;
  pg->npieces = cdiv(pg->PR, 16);
  pg->lo_h = g.dhs > 0 ? g.dh0 : g.dh0 + 2 * g.dhs;
  pg->lo_w = g.dws > 0 ? g.dw0 : g.dw0 + 2 * g.dws;
  // lane-row group order (patch_pixel): pairs of full 16-pixel runs whose first patch rows are congruent mod 16 first,
  // then the runs without a partner, then the left-over / dead groups
  const int a = pg->PW >> 4;
  const int nfull = pg->PH * a < 8 ? pg->PH * a : 8;
  auto base = [&](int q) { return ((q / a) * pg->PWP + (q % a) * 16) & 15; };
  int fin[8], nf = 0, singles[8], ns = 0;
  bool used[8] = {false, false, false, false, false, false, false, false};
  for (int q = 0; q < nfull; ++q) {
    if (used[q]) continue;
    used[q] = true;
    int partner = -1;
    for (int p2 = q + 1; p2 < nfull; ++p2)
      if (!used[p2] && base(p2) == base(q)) {
        partner = p2;
        break;
      }
    if (partner >= 0) {
      used[partner] = true;
      fin[nf++] = q;
      fin[nf++] = partner;
    } else {
      singles[ns++] = q;
    }
  }
  for (int i = 0; i < ns; ++i) fin[nf++] = singles[i];
  for (int q = nfull; q < 8; ++q) fin[nf++] = q;
  pg->gmap = 0;
  for (int i = 0; i < 8; ++i) pg->gmap |= (unsigned)(fin[i] & 15) << (4 * i);
  return true;
}

// Tiles of the persistent patch kernel's 128-wide walk over a stride-1 3x3 conv with an [n, h, w, cout] destination (the tile
// decomposition depends on nothing else): the size of a sign-word buffer (SignRequest), 2048 bytes per tile.
long pp_sign_tiles(int n, int h, int w, int cout) {
  if (cout < 128 || cout % 128 != 0) return 0;
  FastGeom g;
  g.TH = 3; g.TW = 3; g.ss = 1; g.dsd = 1; g.ph = 0; g.pw = 0; g.dhs = 1; g.dws = 1; g.dh0 = -1; g.dw0 = -1;
  g.Hd = g.OH = h; g.Wd = g.OW = w;
  PatchGeom pg;
  if (!plan_patch(g, &pg, 0.0)) return 0;
  return (long)n * pg.tiles_h * pg.tiles_w * (cout / 128);
}

// The operands of one fprop / dgrad launch.  choose_fprop_route looks only at which are present and how they are aligned.
struct ConvOperands {
  const float *src, *wt, *bias, *residual, *rowscale, *chanscale, *actmask;
  float* dst;
};
static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// packed-weight section an arithmetic reads (fast_pack_store): fp32 | pre-split bf16 (hi quads alone: one bf16 product) | fp16
static const float* weight_section(const ConvOperands& a, const FastGeom& g, int math) {
  return a.wt + (size_t)(g.w_bytes >> 2) * (math == 0 ? 0 : math == 3 ? 2 : 1);
}
template <int BM, int BN, int WM, int WN, int BK, int MATH = 0>
static int launch_reg(const ConvOperands& a, const FastGeom& g, hipStream_t st) {
  const int nbm = cdiv(g.M, BM), nbn = cdiv(g.K, BN);
  route_note(RF_REG, BM, BN, BK, MATH, -1, nbm * nbn);    // (bn field: the K chunk, 16 or 32 source channels)
  hipLaunchKernelGGL((fast_conv_kernel<BM, BN, WM, WN, BK, MATH>), dim3(nbm * nbn), dim3(WM * WN * 64), 0, st, a.src,
                     weight_section(a, g, MATH), a.bias, a.residual, a.rowscale, a.chanscale, a.actmask, a.dst, g, nbm, nbn);
  return check_launch("fast_conv");
}

enum class FpropFamily {
  Nothing,    // empty output grid
  Planes,     // padded-plane operands: conv_patch_pers_kernel (its own file); where it does not take the launch, an argument error
  Narrow,     // narrow_conv_kernel<nd>
  Dot,        // dot_conv_kernel
  Reg,        // fast_conv_kernel<BM, BN, WM, WN, BK, math>
  Patch,      // conv_patch_pers_kernel where it applies, else conv_patch_kernel<bn, epi, math - 1> or, with ks, conv_patch_ks_kernel<epi>
  Dma,        // fast_conv_dma_kernel<128, bn, epi, math>
};
typedef int (*RegLaunch)(const ConvOperands&, const FastGeom&, hipStream_t);
struct FpropRoute {
  FpropFamily family = FpropFamily::Nothing;
  int math = 0;          // MFMA kernels: 0 fp32 products, 1 split-bf16, 2 one bf16 product, 3 one fp16 product (see mma16: PROD = math - 1)
  int epi = -1;          // Patch / Dma: the epilogue flags compiled in, -1 = read at run time
  int bn = 0;            // Patch / Dma: destination channels per tile (64 / 128)
  RegLaunch reg = nullptr;   // Reg: launch_reg<BM, BN, WM, WN, BK, math>
  int nd = 0;            // Narrow: destination channels compiled for
  bool ks = false;       // Patch: the K-split one-tile kernel
  bool try_pers = false;   // Patch / Planes: offer the launch to launch_patch_pers first
  int nbm = 0, nbn = 0;  // Patch / Planes / Dma: tiles along M and N
  bool wide = false;     // Patch / Planes: 128-wide N tiles
  int eflags = 0;        // the SRHIP_EPI_* bits of the call
  PatchGeom pg;          // Patch / Planes
};
// the epilogue flag sets that have a kernel of their own; every other set runs the run-time-flag variant (-1)
static int epi_variant(int eflags, bool with_tail) {
  switch (eflags) {
    case 0: case SRHIP_EPI_BIAS: case SRHIP_EPI_BIAS | SRHIP_EPI_LRELU: case SRHIP_EPI_ACTMASK: case SRHIP_EPI_RESIDUAL: return eflags;
    case 29: return with_tail ? 29 : -1;     // bias | residual | rowscale | chanscale: the attention tail (LDS-DMA kernel only)
    default: return -1;
  }
}

// Which kernel a call takes: geometry, arithmetic mode (g_conv_math) and the knobs g_fast_cfg / g_patch_ks decide; no launch, no request is touched.
static FpropRoute choose_fprop_route(const FastGeom& g, const ConvOperands& a) {
  FpropRoute r;
  const int cfg = g_fast_cfg;
  r.eflags = g.flags & FAST_EPI_MASK;
  if (g.M <= 0) return r;
  const bool scaled_a = r.eflags & (SRHIP_EPI_CHANSCALE | SRHIP_EPI_ROWSCALE);
  if (g.src_pp || g.dst_pp) {                             // padded-plane operands: the persistent patch kernel or nothing
    r.family = FpropFamily::Planes;                       // (neither try flag set: not served)
    if (g_conv_math == 1 && g.K >= 64 && g.K % 8 == 0 && g.C % 32 == 0 && !scaled_a && !g.accumulate &&
        plan_patch(g, &r.pg, 0.0)) {                      // (any patch efficiency: the planes have no other kernel)
      r.math = 1;
      r.nbm = g.N * r.pg.tiles_h * r.pg.tiles_w;
      r.wide = g.K >= 128;
      r.nbn = cdiv(g.K, r.wide ? 128 : 64);
      r.try_pers = true;
    }
    return r;
  }
  const bool valu_ok = cfg != FAST_CFG_REG_ONLY && cfg != FAST_CFG_NO_VALU &&
                       !(g.flags & ~(SRHIP_EPI_BIAS | SRHIP_EPI_LRELU | SRHIP_EPI_GRADDATA)) && !g.accumulate;
  // <= 4 destination channels, stride-1 3x3, big image: exact-fp32 VALU kernel (every arithmetic mode)
  if (g.K <= 4 && valu_ok && g.TH == 3 && g.TW == 3 && g.ss == 1 && g.dsd == 1 && g.ph == 0 && g.pw == 0 && g.Hd == g.OH && g.Wd == g.OW &&
      (g.dhs == 1 || g.dhs == -1) && (g.dws == 1 || g.dws == -1) && g.M >= 65536) {
    r.family = FpropFamily::Narrow;
    r.nd = g.K == 3 ? 3 : 4;
    return r;
  }
  // one destination channel, small grid: a wave per output pixel
  if (g.K == 1 && g.C % 4 == 0 && g.lds % 4 == 0 && aligned16(a.src) && aligned16(a.wt) && g.M < 65536 && valu_ok) {
    r.family = FpropFamily::Dot;
    return r;
  }
  // 16-bit product arithmetic (see mma16): split-bf16 (three products), or under SRHIP_MATH_HALF one bf16 product on gradient
  // data (every dgrad, and forward calls flagged GRADDATA) and one fp16 product on activations
  const int math16 = g_conv_math == 2 ? ((g.flags & SRHIP_EPI_GRADDATA) ? 2 : 3) : 1;
  if (g.K <= 32) {
    static const RegLaunch small[4] = {launch_reg<128, 32, 4, 1, 16>, launch_reg<128, 32, 4, 1, 16, 1>, launch_reg<128, 32, 4, 1, 16, 2>,
                                       launch_reg<128, 32, 4, 1, 16, 3>};
    r.family = FpropFamily::Reg;
    if (g_conv_math >= 1 && cfg != FAST_CFG_REG_ONLY && !(g.flags & (SRHIP_EPI_CHANSCALE | FAST_ABL_TIMING))) r.math = math16;
    r.reg = small[r.math];
    return r;
  }
  // LDS-DMA and patch kernels: no ablation flags, 16-byte rows everywhere
  const bool al16 = g.K % 4 == 0 && g.ldd % 4 == 0 && aligned16(a.dst) && (!a.residual || (g.ldr % 4 == 0 && aligned16(a.residual))) &&
                    aligned16(a.actmask) && aligned16(a.bias);
  const bool dma_ok = fast_cfg_allows_dma(cfg) && !(g.flags & FAST_ABL_TIMING) && g.K >= 64 && al16;
  // stride-1 3x3 in a 16-bit arithmetic: the patch family, from 256 tiles on
  bool patch_to_dma = false;
  if (dma_ok && g_conv_math >= 1 && cfg != FAST_CFG_NO_PATCH && !scaled_a && !g.accumulate && plan_patch(g, &r.pg)) {
    r.nbm = g.N * r.pg.tiles_h * r.pg.tiles_w;
    r.wide = g.K >= 128 && cfg != FAST_CFG_PATCH_NARROW;
    r.bn = r.wide ? 128 : 64;
    r.nbn = cdiv(g.K, r.bn);
    const bool enough = (long)r.nbm * r.nbn >= 256;
    if (cfg == FAST_CFG_PATCH_TO_DMA) {
      patch_to_dma = enough;
    } else if (enough || cfg == FAST_CFG_FORCE_PATCH) {
      r.family = FpropFamily::Patch;
      r.math = math16;
      r.try_pers = !(g.flags & FAST_ABL_PLAIN_STORES);    // persistent tile walk (srhip_debug_set(5, -1): never)
      // the one-tile kernels behind it.  SRHIP_MATH_HALF: run-time epilogue flags keep the variant count down
      r.ks = math16 == 1 && !r.wide && g_patch_ks && g.C % 32 == 0 && g.C >= 32;   // K-split form of the 64-wide tile
      r.epi = math16 != 1 ? -1 : epi_variant(r.eflags, false);
      if (r.ks && r.epi != 0 && r.epi != SRHIP_EPI_BIAS && r.epi != SRHIP_EPI_RESIDUAL) r.epi = -1;
      return r;
    }
  }
  if (dma_ok && (!(r.eflags & SRHIP_EPI_CHANSCALE) || aligned16(a.chanscale))) {
    r.nbm = cdiv(g.M, 128);
    const bool force = cfg == FAST_CFG_FORCE_DMA || patch_to_dma;   // tests: take the DMA kernels at any problem size
    // fp32: the register-staged kernel wins below ~2 tiles per CU; split-bf16: its fp32 MFMAs cost 5x more than
    // the DMA kernel's, so the DMA kernel is taken from half a wave of tiles on
    const long min_tiles = g_conv_math >= 1 ? 128 : 512;
    // (round 5, measured and dropped: 64-wide tiles for launches with fewer than 384 wide tiles -- D's 512 -> 512 stride-2 conv at 14 x 14,
    // 196 -> 392 blocks -- ran 154.5 us against 143.8)
    r.wide = g.K >= 128 && ((long)r.nbm * cdiv(g.K, 128) >= min_tiles || force);
    if (r.wide || (long)r.nbm * cdiv(g.K, 64) >= min_tiles || force) {
      r.family = FpropFamily::Dma;
      r.bn = r.wide ? 128 : 64;
      r.nbn = cdiv(g.K, r.bn);
      r.math = g_conv_math >= 1 ? math16 : 0;
      r.epi = (r.math >= 2 || g.accumulate) ? -1 : epi_variant(r.eflags, true);   // SRHIP_MATH_HALF: run-time epilogue flags
      return r;
    }
  }
  // register-staged kernel, fp32 products in every arithmetic mode: by tile count, or the tile g_fast_cfg 1..8 names where the shape allows it
  struct Forced { int cfg; bool k128, k32; RegLaunch fn; };   // k128: needs >= 128 destination channels, k32: source channels % 32 == 0
  static const Forced forced[] = {
      {FAST_CFG_REG_128x128_K32, true, true, launch_reg<128, 128, 2, 2, 32>}, {FAST_CFG_REG_64x128, true, false, launch_reg<64, 128, 1, 4, 16>},
      {FAST_CFG_REG_64x128_K32, true, true, launch_reg<64, 128, 1, 4, 32>},   {FAST_CFG_REG_256x128, true, false, launch_reg<256, 128, 4, 2, 16>},
      {FAST_CFG_REG_128x128, true, false, launch_reg<128, 128, 2, 2, 16>},    {FAST_CFG_REG_128x64_K32, false, true, launch_reg<128, 64, 2, 2, 32>},
      {FAST_CFG_REG_64x64, false, false, launch_reg<64, 64, 2, 2, 16>},       {FAST_CFG_REG_128x64_4x1_K32, false, true, launch_reg<128, 64, 4, 1, 32>}};
  r.family = FpropFamily::Reg;
  const long b128 = (long)cdiv(g.M, 128) * cdiv(g.K, 128), b64 = (long)cdiv(g.M, 128) * cdiv(g.K, 64);
  r.reg = (g.K >= 128 && b128 >= 512) ? launch_reg<128, 128, 2, 2, 16> : b64 >= 512 ? launch_reg<128, 64, 2, 2, 16> : launch_reg<64, 64, 2, 2, 16>;
  for (const Forced& c : forced)
    if (cfg == c.cfg && (!c.k128 || g.K >= 128) && (!c.k32 || g.C % 32 == 0)) r.reg = c.fn;
  return r;
}

template <int BN, int EPI, int PROD = 0>
static int launch_patch(const ConvOperands& a, const FastGeom& g, const FpropRoute& r, hipStream_t st) {
  route_note(RF_PATCH, r.pg.PH, r.pg.PW, BN, PROD + 1, EPI, r.nbm * r.nbn);
  hipLaunchKernelGGL((conv_patch_kernel<BN, EPI, PROD>), dim3(r.nbm * r.nbn), dim3(256), 0, st, a.src, weight_section(a, g, PROD + 1), a.bias,
                     a.residual, a.actmask, a.dst, g, r.pg, r.nbm, r.nbn);
  return check_launch("conv_patch");
}
template <int EPI>
static int launch_patch_ks(const ConvOperands& a, const FastGeom& g, const FpropRoute& r, hipStream_t st) {
  route_note(RF_PATCH_KS, r.pg.PH, r.pg.PW, 64, 1, EPI, r.nbm * r.nbn);
  hipLaunchKernelGGL((conv_patch_ks_kernel<EPI>), dim3(r.nbm * r.nbn), dim3(256), 0, st, a.src, weight_section(a, g, 1), a.bias, a.residual,
                     a.actmask, a.dst, g, r.pg, r.nbm, r.nbn);
  return check_launch("conv_patch_ks");
}
template <int BN, int EPI, int MATH>
static int launch_dma(const ConvOperands& a, const FastGeom& g, const FpropRoute& r, hipStream_t st) {
  PhaseSet ps;
  int grid = r.nbm * r.nbn;
  if constexpr (MATH <= 1) {                           // (SRHIP_MATH_HALF: neither request is ever served)
    if (g.dst2_pp) g_dst2_req.served = 1;
    if (g_phase_req.active) {                          // all phases of a strided data gradient in this launch
      ps = g_phase_req.ps;
      grid = 0;
      for (int k = 0; k < ps.n; ++k) {
        ps.first[k] = grid;
        grid += ps.p[k].nblk_m * r.nbn;
      }
      ps.first[ps.n] = grid;
      g_phase_req.launched = 1;
    }
  }
  route_note(RF_DMA, 128, BN, 0, MATH, EPI, grid, 0, 0, ps.n);
  hipLaunchKernelGGL((fast_conv_dma_kernel<128, BN, EPI, MATH>), dim3(grid), dim3(256), 0, st, a.src, weight_section(a, g, MATH),
                     a.bias, a.residual, a.rowscale, a.chanscale, a.actmask, a.dst, g, r.nbm, r.nbn, ps);
  return check_launch("fast_conv_dma");
}
// f(IC<EPI>) for the epilogue variant a route names (epi_variant); 29 exists for the LDS-DMA kernel alone (TAIL)
template <bool TAIL, class F>
static int with_epi(int epi, F f) {
  switch (epi) {
    case 0: return f(IC<0>{});
    case 1: return f(IC<1>{});
    case 3: return f(IC<3>{});
    case 32: return f(IC<32>{});
    case 4: return f(IC<4>{});
    case 29: if constexpr (TAIL) return f(IC<29>{}); [[fallthrough]];
    default: return f(IC<-1>{});
  }
}

static int launch_fprop(const ConvOperands& a, const FastGeom& g, const FpropRoute& r, hipStream_t st) {
  const bool wide = r.bn == 128;
  switch (r.family) {
    case FpropFamily::Nothing:
      return SRHIP_OK;
    case FpropFamily::Planes:
    case FpropFamily::Patch: {
      if (r.try_pers) {
        const int rc = launch_patch_pers(a.src, a.wt, a.bias, a.residual, a.actmask, a.dst, g, r.pg, r.nbm, r.nbn, r.wide, r.math - 1, r.eflags, st);
        if (rc >= 0) return rc;
      }
      if (r.family == FpropFamily::Planes) break;
      if (r.math == 2) return wide ? launch_patch<128, -1, 1>(a, g, r, st) : launch_patch<64, -1, 1>(a, g, r, st);
      if (r.math == 3) return wide ? launch_patch<128, -1, 2>(a, g, r, st) : launch_patch<64, -1, 2>(a, g, r, st);
      if (wide) return with_epi<false>(r.epi, [&](auto e) { return launch_patch<128, decltype(e)::value>(a, g, r, st); });
      if (!r.ks) return with_epi<false>(r.epi, [&](auto e) { return launch_patch<64, decltype(e)::value>(a, g, r, st); });
      switch (r.epi) {
        case 0: return launch_patch_ks<0>(a, g, r, st);
        case 1: return launch_patch_ks<1>(a, g, r, st);
        case 4: return launch_patch_ks<4>(a, g, r, st);
        default: return launch_patch_ks<-1>(a, g, r, st);
      }
    }
    case FpropFamily::Narrow: {
      const int th = cdiv(g.OH, 16), tw = cdiv(g.OW, 16);
      const int lo_h = g.dhs > 0 ? g.dh0 : g.dh0 + 2 * g.dhs, lo_w = g.dws > 0 ? g.dw0 : g.dw0 + 2 * g.dws;
      const unsigned long long* smask = nullptr;
      if (g_src_mask_req.words != nullptr && g.C == 64 && g.lds == 64) {    // srhip_conv2d_dgrad_head_mask
        smask = static_cast<const unsigned long long*>(g_src_mask_req.words);
        g_src_mask_req.served = 1;
      }
      auto k = smask ? (r.nd == 3 ? narrow_conv_kernel<3, true> : narrow_conv_kernel<4, true>)
                     : (r.nd == 3 ? narrow_conv_kernel<3, false> : narrow_conv_kernel<4, false>);
      route_note(RF_NARROW, 16, 16, r.nd, 0, -1, g.N * th * tw);
      hipLaunchKernelGGL(k, dim3(g.N * th * tw), dim3(256), 0, st, a.src, a.wt, a.bias, a.dst, g, th, tw, lo_h, lo_w, smask);
      return check_launch("narrow_conv");
    }
    case FpropFamily::Dot:
      route_note(RF_DOT, 4, 1, 0, 0, -1, cdiv(g.M, 4));
      hipLaunchKernelGGL(dot_conv_kernel, dim3(cdiv(g.M, 4)), dim3(256), 0, st, a.src, a.wt, a.bias, a.dst, g);
      return check_launch("dot_conv");
    case FpropFamily::Dma:
      if (r.math == 2) return wide ? launch_dma<128, -1, 2>(a, g, r, st) : launch_dma<64, -1, 2>(a, g, r, st);
      if (r.math == 3) return wide ? launch_dma<128, -1, 3>(a, g, r, st) : launch_dma<64, -1, 3>(a, g, r, st);
      if (r.math == 1 && wide) return with_epi<true>(r.epi, [&](auto e) { return launch_dma<128, decltype(e)::value, 1>(a, g, r, st); });
      if (r.math == 1) return with_epi<true>(r.epi, [&](auto e) { return launch_dma<64, decltype(e)::value, 1>(a, g, r, st); });
      if (wide) return with_epi<true>(r.epi, [&](auto e) { return launch_dma<128, decltype(e)::value, 0>(a, g, r, st); });
      return with_epi<true>(r.epi, [&](auto e) { return launch_dma<64, decltype(e)::value, 0>(a, g, r, st); });
    case FpropFamily::Reg:
      return r.reg(a, g, st);
  }
  set_error("conv2d (padded planes): shape / arithmetic mode not served by the persistent patch kernel");
  return SRHIP_ERR_ARG;
}

static int run_fast(const ConvOperands& a, const FastGeom& g, hipStream_t st) { return launch_fprop(a, g, choose_fprop_route(g, a), st); }

int fast_conv2d_fwd(const float* x, const float* packed, const float* bias, const float* residual,
                    const float* rowscale, const float* chanscale, float* y, int n, int h, int w, int cin, int cout, int kh, int kw,
                    int stride, int pad, int ldx, int ldy, int ldr, float slope, int flags, hipStream_t st) {
  SRHIP_REQUIRE(ldx % 4 == 0 && (((uintptr_t)x | (uintptr_t)packed) & 15) == 0, "conv2d_fwd: x/packed must be 16-byte aligned with ldx % 4 == 0");
  FastGeom g;
  g.N = n; g.Hs = h; g.Ws = w; g.C = cin; g.lds = ldx;
  g.OH = (h + 2 * pad - kh) / stride + 1;
  g.OW = (w + 2 * pad - kw) / stride + 1;
  SRHIP_REQUIRE(g.OH > 0 && g.OW > 0, "conv2d_fwd: empty output");
  const long M = (long)n * g.OH * g.OW;
  SRHIP_REQUIRE(M < (1L << 31), "conv2d_fwd: pixel count overflows int32");
  g.M = (int)M; g.ss = stride;
  g.TH = kh; g.TW = kw; g.dh0 = -pad; g.dhs = 1; g.dw0 = -pad; g.dws = 1;
  g.kh0 = 0; g.khs = 1; g.kw0 = 0; g.kws = 1; g.KW = kw;
  g.Hd = g.OH; g.Wd = g.OW; g.dsd = 1; g.ph = 0; g.pw = 0; g.ldd = ldy; g.K = cout;
  g.ldw = kh * kw * cin; g.ldr = ldr; g.slope = slope; g.flags = flags | g_fast_ablate; g.accumulate = 0; g.dst_identity = 1;
  SRHIP_REQUIRE(bytes_ok((long)n * h * w, ldx, cin, &g.src_bytes), "conv2d_fwd: source tensor >= 2 GiB");
  g.w_bytes = (unsigned)((long)cout * g.ldw * 4);
  if (g_dst2_req.pp != nullptr && stride == 1 && cout % 8 == 0 && g.OH == g.Hd && g.OW == g.Wd) {   // srhip_conv2d_fwd_dual
    g.dst2_pp = g_dst2_req.pp;
    g.dst2_guard = pp_guard(g.Wd);
  }
  return run_fast({x, packed, bias, residual, rowscale, chanscale, nullptr, y}, g, st);
}

// 3x3 stride-1 pad-1 forward / data gradient with padded-plane operands (src_pp / dst_pp; with dst_pp an activation mask is pp too)
int fast_conv2d_fwd_pp(const void* x, int x_pp, const float* packed, const float* bias, void* y, int y_pp, int n, int h, int w, int cin,
                       int cout, int ldx, int ldy, float slope, int flags, hipStream_t st) {
  FastGeom g;
  g.N = n; g.Hs = h; g.Ws = w; g.C = cin; g.lds = x_pp ? cin : ldx;
  g.OH = h; g.OW = w;
  const long M = (long)n * h * w;
  SRHIP_REQUIRE(M < (1L << 31), "conv2d_fwd_pp: pixel count overflows int32");
  g.M = (int)M; g.ss = 1;
  g.TH = 3; g.TW = 3; g.dh0 = -1; g.dhs = 1; g.dw0 = -1; g.dws = 1;
  g.kh0 = 0; g.khs = 1; g.kw0 = 0; g.kws = 1; g.KW = 3;
  g.Hd = h; g.Wd = w; g.dsd = 1; g.ph = 0; g.pw = 0; g.ldd = y_pp ? cout : ldy; g.K = cout;
  g.ldw = 9 * cin; g.ldr = 0; g.slope = slope; g.flags = flags; g.accumulate = 0; g.dst_identity = 1;
  const long ppx = pp_plane_pixels(n, h, w);
  g.src_pp = x_pp; g.dst_pp = y_pp;
  g.src_guard = g.dst_guard = pp_guard(w);
  if (x_pp) {
    SRHIP_REQUIRE(ppx * cin * 4L < (1L << 31), "conv2d_fwd_pp: source planes >= 2 GiB");
    g.src_plane_bytes = (unsigned)(ppx * cin * 2L);
    g.src_bytes = 2u * g.src_plane_bytes;
  } else {
    SRHIP_REQUIRE(bytes_ok(M, ldx, cin, &g.src_bytes), "conv2d_fwd_pp: source tensor >= 2 GiB");
  }
  if (y_pp) {
    SRHIP_REQUIRE(ppx * cout * 4L < (1L << 31), "conv2d_fwd_pp: destination planes >= 2 GiB");
    g.dst_plane_bytes = (unsigned)(ppx * cout * 2L);
  }
  g.w_bytes = (unsigned)((long)cout * g.ldw * 4);
  return run_fast({static_cast<const float*>(x), packed, bias, nullptr, nullptr, nullptr, nullptr, static_cast<float*>(y)}, g, st);
}

int fast_conv2d_dgrad_pp(const void* dy, int dy_pp, const float* packed, void* dx, int dx_pp, const float* residual, const void* actmask,
                         float slope, int n, int h, int w, int cin, int cout, int ldy, int ldx, int ldr, hipStream_t st) {
  FastGeom g;
  g.N = n; g.Hs = h; g.Ws = w; g.C = cout; g.lds = dy_pp ? cout : ldy;
  g.KW = 3; g.Hd = h; g.Wd = w; g.dsd = 1; g.ldd = dx_pp ? cin : ldx; g.K = cin;
  g.ldw = 9 * cout; g.ldr = ldr; g.slope = slope; g.accumulate = 0;
  g.flags = (residual ? SRHIP_EPI_RESIDUAL : 0) | (actmask ? SRHIP_EPI_ACTMASK : 0) | SRHIP_EPI_GRADDATA;
  g.ss = 1; g.dhs = -1; g.dws = -1; g.khs = 1; g.kws = 1;
  g.dst_identity = 1;
  // stride 1, pad 1, 3 x 3: ONE phase (fast_conv2d_dgrad's general code with stride = 1, pad = 1): tap th reads dy row hh + 1 - th
  g.ph = 0; g.pw = 0; g.OH = h; g.OW = w; g.kh0 = 0; g.kw0 = 0;
  g.TH = 3; g.TW = 3;
  g.dh0 = 1; g.dw0 = 1;
  const long M = (long)n * h * w;
  SRHIP_REQUIRE(M < (1L << 31), "conv2d_dgrad_pp: pixel count overflows int32");
  g.M = (int)M;
  const long ppx = pp_plane_pixels(n, h, w);
  g.src_pp = dy_pp; g.dst_pp = dx_pp;
  g.src_guard = g.dst_guard = pp_guard(w);
  if (dy_pp) {
    SRHIP_REQUIRE(ppx * cout * 4L < (1L << 31), "conv2d_dgrad_pp: dy planes >= 2 GiB");
    g.src_plane_bytes = (unsigned)(ppx * cout * 2L);
    g.src_bytes = 2u * g.src_plane_bytes;
  } else {
    SRHIP_REQUIRE(bytes_ok(M, ldy, cout, &g.src_bytes), "conv2d_dgrad_pp: dy tensor >= 2 GiB");
  }
  if (dx_pp) {
    SRHIP_REQUIRE(ppx * cin * 4L < (1L << 31), "conv2d_dgrad_pp: dx planes >= 2 GiB");
    g.dst_plane_bytes = (unsigned)(ppx * cin * 2L);
  }
  g.w_bytes = (unsigned)((long)cin * g.ldw * 4);
  if (residual && !dx_pp) {                           // srhip_conv2d_dgrad_pp_res3: the kernel that takes them marks the request served
    g.res2 = g_res_req.r2;
    g.res3 = g_res_req.r3;
  }
  return run_fast({static_cast<const float*>(dy), packed, nullptr, residual, nullptr, nullptr, static_cast<const float*>(actmask),
                   static_cast<float*>(dx)}, g, st);
}

int fast_conv2d_dgrad(const float* dy, const float* packed, float* dx, const float* residual, const float* actmask,
                      float slope, int n, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad, int ldy,
                      int ldx, int ldr, int accumulate, hipStream_t st) {
  SRHIP_REQUIRE(ldy % 4 == 0 && (((uintptr_t)dy | (uintptr_t)packed) & 15) == 0, "conv2d_dgrad: dy/packed must be 16-byte aligned with ldy % 4 == 0");
  const int ho = (h + 2 * pad - kh) / stride + 1, wo = (w + 2 * pad - kw) / stride + 1;
  SRHIP_REQUIRE(ho > 0 && wo > 0, "conv2d_dgrad: empty dy");
  FastGeom g;
  g.N = n; g.Hs = ho; g.Ws = wo; g.C = cout; g.lds = ldy;
  g.KW = kw; g.Hd = h; g.Wd = w; g.dsd = stride; g.ldd = ldx; g.K = cin;
  g.ldw = kh * kw * cout; g.ldr = ldr; g.slope = slope; g.accumulate = accumulate ? 1 : 0;
  g.flags = (residual ? SRHIP_EPI_RESIDUAL : 0) | (actmask ? SRHIP_EPI_ACTMASK : 0) | SRHIP_EPI_GRADDATA;
  g.ss = 1; g.dhs = -1; g.dws = -1; g.khs = stride; g.kws = stride;
  g.dst_identity = stride == 1 ? 1 : 0;
  SRHIP_REQUIRE(bytes_ok((long)n * ho * wo, ldy, cout, &g.src_bytes), "conv2d_dgrad: dy tensor >= 2 GiB");
  g.w_bytes = (unsigned)((long)cin * g.ldw * 4);
  if (residual && stride == 1 && !accumulate) {       // srhip_conv2d_dgrad_res3: the kernel that takes them marks the request served
    g.res2 = g_res_req.r2;
    g.res3 = g_res_req.r3;
  }
  // dx[hh] gathers dy[(hh + pad - kh)/stride] for kh == (hh + pad) mod stride: one dense GEMM per phase
  // Round 5: where the LDS-DMA kernel takes the phases (split-bf16 / fp32 arithmetic), ALL of them go out as ONE launch (PhaseSet):
  // the request rides beside the first phase's run_fast call, which launches every phase when it reaches that kernel.
  PhaseRequest& pq = g_phase_req;
  pq = PhaseRequest();
  if (stride == 2 && g_conv_math != 2 && g_phase_batch) {          // (srhip_debug_set(17, 0): one launch per phase, rounds 1-4)
    bool all = true;
    int k = 0;
    for (int ph = 0; ph < stride && all; ++ph)
      for (int pw = 0; pw < stride && all; ++pw) {
        PhaseSet::P& q = pq.ps.p[k++];
        q.ph = ph; q.pw = pw;
        q.OH = (h - ph + stride - 1) / stride;
        q.OW = (w - pw + stride - 1) / stride;
        q.kh0 = (ph + pad) % stride; q.kw0 = (pw + pad) % stride;
        q.TH = q.kh0 < kh ? (kh - q.kh0 + stride - 1) / stride : 0;
        q.TW = q.kw0 < kw ? (kw - q.kw0 + stride - 1) / stride : 0;
        q.dh0 = (ph + pad - q.kh0) / stride; q.dw0 = (pw + pad - q.kw0) / stride;
        const long M = (long)n * q.OH * q.OW;
        all = q.OH > 0 && q.OW > 0 && q.TH > 0 && q.TW > 0 && M < (1L << 31);
        q.M = (int)M;
        q.nblk_m = cdiv(M, 128);
      }
    if (all) {
      pq.ps.n = stride * stride;
      pq.active = 1;
    }
  }
  for (int ph = 0; ph < stride; ++ph) {
    for (int pw = 0; pw < stride; ++pw) {
      g.ph = ph; g.pw = pw;
      g.OH = (h - ph + stride - 1) / stride;
      g.OW = (w - pw + stride - 1) / stride;
      if (g.OH <= 0 || g.OW <= 0) continue;
      g.kh0 = (ph + pad) % stride; g.kw0 = (pw + pad) % stride;
      g.TH = g.kh0 < kh ? (kh - g.kh0 + stride - 1) / stride : 0;
      g.TW = g.kw0 < kw ? (kw - g.kw0 + stride - 1) / stride : 0;
      if (g.TH == 0 || g.TW == 0) { g.TH = 0; g.TW = 0; }
      g.dh0 = (ph + pad - g.kh0) / stride; g.dw0 = (pw + pad - g.kw0) / stride;
      const long M = (long)n * g.OH * g.OW;
      SRHIP_REQUIRE(M < (1L << 31), "conv2d_dgrad: pixel count overflows int32");
      g.M = (int)M;
      int rc = run_fast({dy, packed, nullptr, residual, nullptr, nullptr, actmask, dx}, g, st);
      const bool all_out = pq.active && pq.launched;
      pq = PhaseRequest();                              // (a request only ever rides beside the first phase)
      if (rc) return rc;
      if (all_out) return SRHIP_OK;
    }
  }
  return SRHIP_OK;
}


}  // namespace srhip
