// Average-pool-only channel attention with the block's residual add (DSSR's WAB, reference model/dssr.py:69-104):
//     s[n,c] = sigmoid(fc2 relu(fc1 mean_hw u))          out = s * u + x
// with optional biases on the two 1x1 convs (RCAN's CALayer.conv_du, reference model/drcan.py:94-111):
//     s[n,c] = sigmoid(fc2 relu(fc1 mean_hw u + b1) + b2)
// NULL biases add nothing, so the bias-free entry points keep their arithmetic bit for bit.
// and its backward, plus the two small passes of the DSSR upsampler fold (out = a + G * b broadcast over the batch and its
// batch-sum backward).  u, x, g: NHWC, C == 64 channels, ld == C.  Every reduction is a fixed-order two-stage sum (per
// (image, segment) partials, then one fixed walk over the segments): no atomics, bit-identical from run to run.
// The element-wise passes are HBM-bound: 16-byte loads and stores, 16 lanes per pixel (4 channels per lane).
#include "common.h"

namespace srhip {

constexpr int CA_C = 64;        // channels
constexpr int CA_SEG = 32;      // reduction segments per image for the stand-alone passes
constexpr int CA_MAXHID = 16;   // most hidden units of the channel MLP

// part[(b * CA_SEG + seg) * 64 + c] = sum over the segment's pixels of a[p,c] (PROD: a[p,c] * b[p,c]).
// 256 threads = 16 pixel lanes x 16 channel quads; the 16 pixel lanes are combined in a fixed order through LDS.
template <bool PROD>
__global__ __launch_bounds__(256) void ca_chan_partial_kernel(const float4* __restrict__ a, const float4* __restrict__ b,
                                                              float* __restrict__ part, int hw) {
  __shared__ float4 red[16][16];
  const int img = blockIdx.x / CA_SEG, seg = blockIdx.x % CA_SEG;
  const int per = (hw + CA_SEG - 1) / CA_SEG;
  const int p0 = seg * per, p1 = min(p0 + per, hw);
  const int q = threadIdx.x & 15, r = threadIdx.x >> 4;
  const size_t base = (size_t)img * hw * 16 + q;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  int p = p0 + r;
  for (; p + 48 < p1; p += 64) {                       // four independent loads in flight per lane
    float4 v[4], w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = a[base + (size_t)(p + 16 * j) * 16];
      if (PROD) w[j] = b[base + (size_t)(p + 16 * j) * 16];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (PROD) {
        v[j].x *= w[j].x; v[j].y *= w[j].y; v[j].z *= w[j].z; v[j].w *= w[j].w;
      }
      acc.x += v[j].x; acc.y += v[j].y; acc.z += v[j].z; acc.w += v[j].w;
    }
  }
  for (; p < p1; p += 16) {
    float4 v = a[base + (size_t)p * 16];
    if (PROD) {
      const float4 w = b[base + (size_t)p * 16];
      v.x *= w.x; v.y *= w.y; v.z *= w.z; v.w *= w.w;
    }
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  red[r][q] = acc;
  __syncthreads();
  if (threadIdx.x < 64) {                              // thread = channel; fixed order over the 16 pixel lanes
    const int cq = threadIdx.x >> 2, cc = threadIdx.x & 3;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const float4 t = red[k][cq];
      s += cc == 0 ? t.x : (cc == 1 ? t.y : (cc == 2 ? t.z : t.w));
    }
    part[(size_t)blockIdx.x * CA_C + threadIdx.x] = s;
  }
}

// sum over the nseg partials of image b, channel c: lane q of the 4 walks segments q, q + 4, ...; the four sums are added in
// lane order (fixed order).  256 threads, every thread of the block must call it; the result is valid in threads 0..63.
__device__ inline float ca_seg_sum(const float* __restrict__ part, int b, int nseg, float (*red)[CA_C]) {
  const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
  float s = 0.f;
  for (int k = q; k < nseg; k += 4) s += part[((size_t)b * nseg + k) * CA_C + c];
  red[q][c] = s;
  __syncthreads();
  return (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}

// 64-long dot product of row j (16 lanes per hidden unit, lanes 16 j .. 16 j + 15) with v[0..63]: fixed butterfly, all lanes get it
__device__ inline float ca_dot64(const float* __restrict__ row, const float* v) {
  const int l = threadIdx.x & 15;
  float t = (row[l] * v[l] + row[l + 16] * v[l + 16]) + (row[l + 32] * v[l + 32] + row[l + 48] * v[l + 48]);
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) t += __shfl_xor(t, o, 16);
  return t;
}

// one block of 256 threads per image: avg, hidden = relu(fc1 avg + b1), s = sigmoid(fc2 hidden + b2); b1 / b2 may be NULL
__global__ __launch_bounds__(256) void ca_mlp_fwd_kernel(const float* __restrict__ psum, int nseg, float inv_hw,
                                                         const float* __restrict__ fc1, const float* __restrict__ b1,
                                                         const float* __restrict__ fc2, const float* __restrict__ b2,
                                                         float* __restrict__ avg, float* __restrict__ hid, float* __restrict__ s,
                                                         int hidden) {
  __shared__ float red[4][CA_C], sa[CA_C], sh[CA_MAXHID];
  const int b = blockIdx.x, t = threadIdx.x;
  const float a = ca_seg_sum(psum, b, nseg, red) * inv_hw;
  if (t < CA_C) {
    sa[t] = a;
    avg[b * CA_C + t] = a;
  }
  __syncthreads();
  const int j = t >> 4;
  if (j < hidden) {
    float d = ca_dot64(fc1 + j * CA_C, sa);
    if (b1) d += b1[j];
    const float v = d < 0.f ? 0.f : d;                  // ReLU that lets a NaN through like ATen's (fmaxf would return 0)
    if ((t & 15) == 0) {
      sh[j] = v;
      hid[b * hidden + j] = v;
    }
  }
  __syncthreads();
  if (t < CA_C) {
    float l = 0.f;
    for (int k = 0; k < hidden; ++k) l += fc2[t * hidden + k] * sh[k];
    if (b2) l += b2[t];
    s[b * CA_C + t] = 1.f / (1.f + expf(-l));
  }
}

// out = s[n,c] * u + x   (16 lanes per pixel)
__global__ __launch_bounds__(256) void ca_scale_res_kernel(const float4* __restrict__ u, const float4* __restrict__ s,
                                                           const float4* __restrict__ x, float4* __restrict__ out, long quads,
                                                           long quads_per_image) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < quads; i += (long)gridDim.x * 256) {
    const float4 sv = s[(i / quads_per_image) * 16 + (i & 15)], uv = u[i], xv = x[i];
    out[i] = make_float4(sv.x * uv.x + xv.x, sv.y * uv.y + xv.y, sv.z * uv.z + xv.z, sv.w * uv.w + xv.w);
  }
}

// MLP backward, per image (one block of 256 threads each):
//   ds = sum_seg part, dl = ds s (1 - s), dh[j] = [hid > 0] sum_c fc2[c,j] dl[c], dmean[c] = sum_j fc1[j,c] dh[j] / hw
// dl [n][64] and dh [n][hidden] go to scratch for the weight gradients
__global__ __launch_bounds__(256) void ca_mlp_bwd_kernel(const float* __restrict__ part, int nseg, const float* __restrict__ hid,
                                                         const float* __restrict__ s, const float* __restrict__ fc1,
                                                         const float* __restrict__ fc2, float* __restrict__ dmean,
                                                         float* __restrict__ dl_out, float* __restrict__ dh_out, int hidden,
                                                         float inv_hw) {
  __shared__ float red[4][CA_C], sdl[CA_C], sdh[CA_MAXHID], fc2t[CA_MAXHID][CA_C];
  const int b = blockIdx.x, t = threadIdx.x;
  for (int i = t; i < CA_C * hidden; i += 256) fc2t[i % hidden][i / hidden] = fc2[i];      // fc2 [64][hidden] -> rows of 64
  const float ds = ca_seg_sum(part, b, nseg, red);
  if (t < CA_C) {
    const float sv = s[b * CA_C + t];
    const float d = ds * sv * (1.f - sv);
    sdl[t] = d;
    dl_out[b * CA_C + t] = d;
  }
  __syncthreads();
  const int j = t >> 4;
  if (j < hidden) {
    const float d = ca_dot64(fc2t[j], sdl);
    if ((t & 15) == 0) {
      const float v = hid[b * hidden + j] > 0.f ? d : 0.f;
      sdh[j] = v;
      dh_out[b * hidden + j] = v;
    }
  }
  __syncthreads();
  if (t < CA_C) {
    float d = 0.f;
    for (int k = 0; k < hidden; ++k) d += fc1[k * CA_C + t] * sdh[k];
    dmean[b * CA_C + t] = d * inv_hw;
  }
}

// weight gradients, images in order: dfc2[c,j] = sum_b dl[b,c] hid[b,j], dfc1[j,c] = sum_b dh[b,j] avg[b,c]; one thread per element.
// Bias gradients (when db1 / db2 are not NULL), images in order: db2[c] = sum_b dl[b,c] (threads 0..63), db1[j] = sum_b dh[b,j]
// (threads 0..hidden-1); 64 * hidden >= 64 threads, so every bias element has its thread.
__global__ __launch_bounds__(256) void ca_mlp_wgrad_kernel(const float* __restrict__ dl, const float* __restrict__ dh,
                                                           const float* __restrict__ hid, const float* __restrict__ avg,
                                                           float* __restrict__ dfc1, float* __restrict__ dfc2,
                                                           float* __restrict__ db1, float* __restrict__ db2, int n, int hidden) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= CA_C * hidden) return;
  const int c2 = i / hidden, j2 = i % hidden, j1 = i / CA_C, c1 = i % CA_C;
  float g2 = 0.f, g1 = 0.f;
  for (int b = 0; b < n; ++b) {
    g2 += dl[b * CA_C + c2] * hid[b * hidden + j2];
    g1 += dh[b * hidden + j1] * avg[b * CA_C + c1];
  }
  dfc2[i] = g2;
  dfc1[i] = g1;
  if (db2 && i < CA_C) {
    float s2 = 0.f;
    for (int b = 0; b < n; ++b) s2 += dl[b * CA_C + i];
    db2[i] = s2;
  }
  if (db1 && i < hidden) {
    float s1 = 0.f;
    for (int b = 0; b < n; ++b) s1 += dh[b * hidden + i];
    db1[i] = s1;
  }
}

// du = s[n,c] * g + dmean[n,c]
__global__ __launch_bounds__(256) void ca_bwd_du_kernel(const float4* __restrict__ g, const float4* __restrict__ s,
                                                        const float4* __restrict__ dmean, float4* __restrict__ du, long quads,
                                                        long quads_per_image) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < quads; i += (long)gridDim.x * 256) {
    const long k = (i / quads_per_image) * 16 + (i & 15);
    const float4 sv = s[k], dm = dmean[k], gv = g[i];
    du[i] = make_float4(sv.x * gv.x + dm.x, sv.y * gv.y + dm.y, sv.z * gv.z + dm.z, sv.w * gv.w + dm.w);
  }
}

// out[b, i] = a[b, i] + scale * bcast[i]
__global__ __launch_bounds__(256) void add_bcast_scaled_kernel(const float4* __restrict__ a, const float4* __restrict__ bc, float scale,
                                                               float4* __restrict__ out, long quads, long quads_per_image) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < quads; i += (long)gridDim.x * 256) {
    const float4 av = a[i], bv = bc[i % quads_per_image];
    out[i] = make_float4(av.x + scale * bv.x, av.y + scale * bv.y, av.z + scale * bv.z, av.w + scale * bv.w);
  }
}

// out[i] = scale * sum_b g[b, i], images in order
__global__ __launch_bounds__(256) void batch_sum_scaled_kernel(const float4* __restrict__ g, float scale, float4* __restrict__ out,
                                                               int n, long quads_per_image) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < quads_per_image; i += (long)gridDim.x * 256) {
    float4 acc = g[i];
    for (int b = 1; b < n; ++b) {
      const float4 v = g[(size_t)b * quads_per_image + i];
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    out[i] = make_float4(scale * acc.x, scale * acc.y, scale * acc.z, scale * acc.w);
  }
}

static int stream_blocks(long quads) {
  long b = (quads + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 256 * 16 ? 256 * 16 : b));
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace srhip

using namespace srhip;

extern "C" {

int srhip_ca_segments(void) { return CA_SEG; }

int srhip_ca_pool_sum(const float* u, float* psum, int n, int hw, int c, void* stream) {
  SRHIP_REQUIRE(u && psum && c == CA_C && n > 0 && hw > 0 && aligned16(u), "ca_pool_sum: C must be 64, 16-byte aligned input");
  hipLaunchKernelGGL(ca_chan_partial_kernel<false>, dim3(n * CA_SEG), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const float4*>(u), nullptr, psum, hw);
  return check_launch("ca_pool_sum");
}

static int ca_mlp_fwd(const char* what, const float* psum, int nseg, const float* fc1, const float* b1, const float* fc2,
                      const float* b2, float* avg, float* hid, float* s, int n, int hw, int c, int hidden, void* stream) {
  SRHIP_REQUIRE(psum && fc1 && fc2 && avg && hid && s, "%s: null tensor", what);
  SRHIP_REQUIRE(c == CA_C && hidden >= 1 && hidden <= CA_MAXHID && n > 0 && hw > 0 && nseg >= 1 && nseg <= POOL_MAXSEG,
                "%s: C must be 64, 1 <= hidden <= 16, 1 <= nseg <= %d", what, POOL_MAXSEG);
  hipLaunchKernelGGL(ca_mlp_fwd_kernel, dim3(n), dim3(256), 0, as_stream(stream), psum, nseg, (float)(1.0 / (double)hw), fc1, b1, fc2,
                     b2, avg, hid, s, hidden);
  return check_launch(what);
}

int srhip_ca_mlp_fwd(const float* psum, int nseg, const float* fc1, const float* fc2, float* avg, float* hid, float* s, int n, int hw,
                     int c, int hidden, void* stream) {
  return ca_mlp_fwd("ca_mlp_fwd", psum, nseg, fc1, nullptr, fc2, nullptr, avg, hid, s, n, hw, c, hidden, stream);
}

int srhip_ca_mlp_fwd_bias(const float* psum, int nseg, const float* fc1, const float* b1, const float* fc2, const float* b2, float* avg,
                          float* hid, float* s, int n, int hw, int c, int hidden, void* stream) {
  return ca_mlp_fwd("ca_mlp_fwd_bias", psum, nseg, fc1, b1, fc2, b2, avg, hid, s, n, hw, c, hidden, stream);
}

int srhip_ca_scale_res(const float* u, const float* s, const float* x, float* out, int n, int hw, int c, void* stream) {
  SRHIP_REQUIRE(u && s && x && out && c == CA_C && n > 0 && hw > 0, "ca_scale_res: null tensor or C != 64");
  SRHIP_REQUIRE(aligned16(u) && aligned16(s) && aligned16(x) && aligned16(out), "ca_scale_res: tensors must be 16-byte aligned");
  const long qpi = (long)hw * 16, quads = qpi * n;
  hipLaunchKernelGGL(ca_scale_res_kernel, dim3(stream_blocks(quads)), dim3(256), 0, as_stream(stream), reinterpret_cast<const float4*>(u),
                     reinterpret_cast<const float4*>(s), reinterpret_cast<const float4*>(x), reinterpret_cast<float4*>(out), quads, qpi);
  return check_launch("ca_scale_res");
}

int srhip_ca_bwd_partial(const float* g, const float* u, float* part, int n, int hw, int c, void* stream) {
  SRHIP_REQUIRE(g && u && part && c == CA_C && n > 0 && hw > 0 && aligned16(g) && aligned16(u),
                "ca_bwd_partial: C must be 64, 16-byte aligned inputs");
  hipLaunchKernelGGL(ca_chan_partial_kernel<true>, dim3(n * CA_SEG), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const float4*>(g), reinterpret_cast<const float4*>(u), part, hw);
  return check_launch("ca_bwd_partial");
}

size_t srhip_ca_mlp_bwd_workspace(int n, int hidden) { return (size_t)n * (CA_C + (hidden > 0 ? hidden : 0)) * sizeof(float); }

static int ca_mlp_bwd(const char* what, const float* part, const float* avg, const float* hid, const float* s, const float* fc1,
                      const float* fc2, float* dmean, float* dfc1, float* db1, float* dfc2, float* db2, void* workspace,
                      size_t workspace_bytes, int n, int hw, int c, int hidden, void* stream) {
  SRHIP_REQUIRE(part && avg && hid && s && fc1 && fc2 && dmean && dfc1 && dfc2, "%s: null tensor", what);
  SRHIP_REQUIRE(c == CA_C && hidden >= 1 && hidden <= CA_MAXHID && n > 0 && hw > 0, "%s: C must be 64, 1 <= hidden <= 16", what);
  SRHIP_REQUIRE(workspace && workspace_bytes >= srhip_ca_mlp_bwd_workspace(n, hidden), "%s: workspace too small", what);
  float* dl = static_cast<float*>(workspace);
  float* dh = dl + (size_t)n * CA_C;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(ca_mlp_bwd_kernel, dim3(n), dim3(256), 0, st, part, CA_SEG, hid, s, fc1, fc2, dmean, dl, dh, hidden,
                     (float)(1.0 / (double)hw));
  hipLaunchKernelGGL(ca_mlp_wgrad_kernel, dim3(cdiv(CA_C * hidden, 256)), dim3(256), 0, st, dl, dh, hid, avg, dfc1, dfc2, db1, db2, n,
                     hidden);
  return check_launch(what);
}

int srhip_ca_mlp_bwd(const float* part, const float* avg, const float* hid, const float* s, const float* fc1, const float* fc2,
                     float* dmean, float* dfc1, float* dfc2, void* workspace, size_t workspace_bytes, int n, int hw, int c, int hidden,
                     void* stream) {
  return ca_mlp_bwd("ca_mlp_bwd", part, avg, hid, s, fc1, fc2, dmean, dfc1, nullptr, dfc2, nullptr, workspace, workspace_bytes, n, hw, c,
                    hidden, stream);
}

int srhip_ca_mlp_bwd_bias(const float* part, const float* avg, const float* hid, const float* s, const float* fc1, const float* fc2,
                          float* dmean, float* dfc1, float* db1, float* dfc2, float* db2, void* workspace, size_t workspace_bytes, int n,
                          int hw, int c, int hidden, void* stream) {
  return ca_mlp_bwd("ca_mlp_bwd_bias", part, avg, hid, s, fc1, fc2, dmean, dfc1, db1, dfc2, db2, workspace, workspace_bytes, n, hw, c,
                    hidden, stream);
}

int srhip_ca_bwd_du(const float* g, const float* s, const float* dmean, float* du, int n, int hw, int c, void* stream) {
  SRHIP_REQUIRE(g && s && dmean && du && c == CA_C && n > 0 && hw > 0, "ca_bwd_du: null tensor or C != 64");
  SRHIP_REQUIRE(aligned16(g) && aligned16(s) && aligned16(dmean) && aligned16(du), "ca_bwd_du: tensors must be 16-byte aligned");
  const long qpi = (long)hw * 16, quads = qpi * n;
  hipLaunchKernelGGL(ca_bwd_du_kernel, dim3(stream_blocks(quads)), dim3(256), 0, as_stream(stream), reinterpret_cast<const float4*>(g),
                     reinterpret_cast<const float4*>(s), reinterpret_cast<const float4*>(dmean), reinterpret_cast<float4*>(du), quads, qpi);
  return check_launch("ca_bwd_du");
}

int srhip_add_bcast_scaled(const float* a, const float* b, float scale, float* out, int n, long per_image, void* stream) {
  SRHIP_REQUIRE(a && b && out && n > 0 && per_image > 0 && per_image % 4 == 0, "add_bcast_scaled: per-image count must be a multiple of 4");
  SRHIP_REQUIRE(aligned16(a) && aligned16(b) && aligned16(out), "add_bcast_scaled: tensors must be 16-byte aligned");
  const long qpi = per_image / 4, quads = qpi * n;
  hipLaunchKernelGGL(add_bcast_scaled_kernel, dim3(stream_blocks(quads)), dim3(256), 0, as_stream(stream), reinterpret_cast<const float4*>(a),
                     reinterpret_cast<const float4*>(b), scale, reinterpret_cast<float4*>(out), quads, qpi);
  return check_launch("add_bcast_scaled");
}

int srhip_batch_sum_scaled(const float* g, float scale, float* out, int n, long per_image, void* stream) {
  SRHIP_REQUIRE(g && out && n > 0 && per_image > 0 && per_image % 4 == 0, "batch_sum_scaled: per-image count must be a multiple of 4");
  SRHIP_REQUIRE(aligned16(g) && aligned16(out), "batch_sum_scaled: tensors must be 16-byte aligned");
  const long qpi = per_image / 4;
  hipLaunchKernelGGL(batch_sum_scaled_kernel, dim3(stream_blocks(qpi)), dim3(256), 0, as_stream(stream), reinterpret_cast<const float4*>(g),
                     scale, reinterpret_cast<float4*>(out), n, qpi);
  return check_launch("batch_sum_scaled");
}

}  // extern "C"
