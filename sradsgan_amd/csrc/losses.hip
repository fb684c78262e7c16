// Loss reductions of the training step (SRADSGAN/model/sradsgan.py): nn.L1Loss (:686, used :834, :838), nn.MSELoss (DSSR's
// loss_Lp_norm='L2', model/dssr.py:266-269), nn.SmoothL1Loss (NDSRGAN, model/ndsrgan.py:325-351), the WGAN
// critic means of GANLoss (:35-67, used :847, :876-878) and the gradient-penalty reduction (:630-637: per-pixel L2
// norm over channels, (norm - 1)^2, mean; :624-637 for the L1 / Linf norms and the hinge penalty).  Each is one pass over its input (HBM-bound, 16-byte loads where the
// layout allows) into per-block partial sums, and one single-block pass that adds the partials in a fixed order:
// deterministic, no atomics.  The scalar results stay on the device; backward kernels read the incoming scalar
// gradient through a device pointer, so nothing synchronises with the host.
#include "common.h"

namespace srhip {

constexpr int LS_MAXB = 1024;     // partial sums per reduction

__device__ inline float block_sum_256(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// partial[block] = sum |a - b| over a grid-stride range
__global__ __launch_bounds__(256) void l1_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                         float* __restrict__ partial, long n) {
  __shared__ float red[4];
  const long n4 = n >> 2;
  float s = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const float4 x = reinterpret_cast<const float4*>(a)[i], y = reinterpret_cast<const float4*>(b)[i];
    s += (fabsf(x.x - y.x) + fabsf(x.y - y.y)) + (fabsf(x.z - y.z) + fabsf(x.w - y.w));
  }
  if (blockIdx.x == 0)
    for (long i = (n4 << 2) + threadIdx.x; i < n; i += 256) s += fabsf(a[i] - b[i]);
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// partial[block] = sum (a - b)^2 over a grid-stride range (nn.MSELoss, DSSR's loss_Lp_norm='L2')
__global__ __launch_bounds__(256) void sq_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                         float* __restrict__ partial, long n) {
  __shared__ float red[4];
  const long n4 = n >> 2;
  float s = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const float4 x = reinterpret_cast<const float4*>(a)[i], y = reinterpret_cast<const float4*>(b)[i];
    const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
    s += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
  }
  if (blockIdx.x == 0)
    for (long i = (n4 << 2) + threadIdx.x; i < n; i += 256) {
      const float d = a[i] - b[i];
      s += d * d;
    }
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// SmoothL1 with beta = 1 (torch's smooth_l1_loss): |d| < 1 ? 0.5 d^2 : |d| - 0.5
__device__ __forceinline__ float smooth_l1(float d) {
  const float z = fabsf(d);
  return z < 1.f ? 0.5f * z * z : z - 0.5f;
}

// partial[block] = sum smooth_l1(a - t), t = b[i] or the scalar tgt when b == NULL (NDSRGAN's valid / fake targets)
__global__ __launch_bounds__(256) void smooth_l1_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, float tgt,
                                                                float* __restrict__ partial, long n) {
  __shared__ float red[4];
  const long n4 = n >> 2;
  float s = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const float4 x = reinterpret_cast<const float4*>(a)[i];
    const float4 y = b ? reinterpret_cast<const float4*>(b)[i] : make_float4(tgt, tgt, tgt, tgt);
    s += (smooth_l1(x.x - y.x) + smooth_l1(x.y - y.y)) + (smooth_l1(x.z - y.z) + smooth_l1(x.w - y.w));
  }
  if (blockIdx.x == 0)
    for (long i = (n4 << 2) + threadIdx.x; i < n; i += 256) s += smooth_l1(a[i] - (b ? b[i] : tgt));
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// partial[block] = sum x
__global__ __launch_bounds__(256) void sum_partial_kernel(const float* __restrict__ x, float* __restrict__ partial, long n) {
  __shared__ float red[4];
  float s = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) s += x[i];
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// partial[block] = sum over pixels of (||g_pixel||_2 - 1)^2, pixel = c consecutive floats (c <= 4)
__global__ __launch_bounds__(256) void gp_partial_kernel(const float* __restrict__ g, float* __restrict__ partial, long npix, int c) {
  __shared__ float red[4];
  float s = 0.f;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
    float q = 0.f;
    for (int j = 0; j < c; ++j) {
      const float v = g[p * c + j];
      q += v * v;
    }
    const float d = sqrtf(q) - 1.f;
    s += d * d;
  }
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// out[0] = scale * sum(partial[0..nb))
__global__ __launch_bounds__(256) void finish_sum_kernel(const float* __restrict__ partial, int nb, float scale, float* __restrict__ out) {
  __shared__ float red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) s += partial[i];
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) out[0] = s * scale;
}

// da = sign(a - b) * gout / n  (torch: sign(0) = 0); db = -da when asked for
__global__ __launch_bounds__(256) void l1_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                     const float* __restrict__ gout, float* __restrict__ da,
                                                     float* __restrict__ db, long n, float inv_n) {
  const float gs = gout[0] * inv_n;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float d = a[i] - b[i];
    const float v = d > 0.f ? gs : (d < 0.f ? -gs : 0.f);
    da[i] = v;
    if (db) db[i] = -v;
  }
}

// da = 2 (a - b) * gout / n; db = -da when asked for
__global__ __launch_bounds__(256) void sq_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                     const float* __restrict__ gout, float* __restrict__ da,
                                                     float* __restrict__ db, long n, float inv_n) {
  const float gs = 2.f * gout[0] * inv_n;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float v = gs * (a[i] - b[i]);
    da[i] = v;
    if (db) db[i] = -v;
  }
}

// da = clamp(a - t, -1, 1) * gout / n; db = -da when asked for (t = b[i], or tgt when b == NULL)
__global__ __launch_bounds__(256) void smooth_l1_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b, float tgt,
                                                            const float* __restrict__ gout, float* __restrict__ da,
                                                            float* __restrict__ db, long n, float inv_n) {
  const float gs = gout[0] * inv_n;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float d = a[i] - (b ? b[i] : tgt);
    const float v = (d <= -1.f ? -1.f : (d >= 1.f ? 1.f : d)) * gs;
    da[i] = v;
    if (db) db[i] = -v;
  }
}

// dx = gout * scale everywhere (backward of a mean)
__global__ __launch_bounds__(256) void fill_scaled_kernel(const float* __restrict__ gout, float* __restrict__ dx, long n, float scale) {
  const float v = gout[0] * scale;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) dx[i] = v;
}

// d penalty / d g = gout * 2 (norm - 1) / npix * g / norm; 0 where norm == 0 (torch's norm backward)
__global__ __launch_bounds__(256) void gp_bwd_kernel(const float* __restrict__ g, const float* __restrict__ gout,
                                                     float* __restrict__ dg, long npix, int c, float inv_npix) {
  const float gs = gout[0] * 2.f * inv_npix;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
    float q = 0.f;
    for (int j = 0; j < c; ++j) {
      const float v = g[p * c + j];
      q += v * v;
    }
    const float nrm = sqrtf(q);
    const float f = nrm > 0.f ? gs * (nrm - 1.f) / nrm : 0.f;
    for (int j = 0; j < c; ++j) dg[p * c + j] = f * g[p * c + j];
  }
}

static inline int ls_blocks(long work_items) {
  long b = (work_items + 255) / 256;
  return (int)(b < 1 ? 1 : (b > LS_MAXB ? LS_MAXB : b));
}

// ---- the gradient penalty under every option of sradsgan.py:624-637: norm L2 / L1 / Linf over the channels of a pixel, penalty LS
// (norm - 1)^2 or hinge relu(norm - 1).  One templated pair; the kinds arrive by value and pick the instantiation on the host.
enum { GP_L2 = 0, GP_L1 = 1, GP_LINF = 2 };
enum { GP_LS = 0, GP_HINGE = 1 };

template <int NORM>
__device__ __forceinline__ float gp_pixel_norm(const float* __restrict__ g, long p, int c) {
  float q = 0.f;
  for (int j = 0; j < c; ++j) {
    const float v = g[p * c + j];
    if (NORM == GP_L2) q += v * v;
    else if (NORM == GP_L1) q += fabsf(v);
    else {
      const float a = fabsf(v);
      q = (a > q || a != a) ? a : q;               // torch.max(dim): a NaN channel makes the norm NaN (fmaxf would drop it)
    }
  }
  return NORM == GP_L2 ? sqrtf(q) : q;
}

// partial[block] = sum over pixels of penalty(norm(g_pixel) - 1), pixel = c consecutive floats (c <= 4)
template <int NORM, int PEN>
__global__ __launch_bounds__(256) void gp_opt_partial_kernel(const float* __restrict__ g, float* __restrict__ partial, long npix, int c) {
  __shared__ float red[4];
  float s = 0.f;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
    const float d = gp_pixel_norm<NORM>(g, p, c) - 1.f;
    s += PEN == GP_LS ? d * d : (d < 0.f ? 0.f : d);   // ReLU that lets a NaN norm through like ATen's
  }
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// d penalty / d g = gout / npix * penalty'(norm - 1) * d norm / d g, as autograd has it:
//   penalty'  LS: 2 (norm - 1); hinge: 1 where norm - 1 > 0 (in fp32), else 0 (relu's backward: 0 at exactly 1)
//   d norm    L2: g / norm, 0 where norm == 0; L1: sign(g), sign(0) = 0; Linf: sign(g) at the FIRST channel that attains max|g|
//             (torch.max(dim) returns the first maximal index), 0 at the others -- an all-zero pixel gets sign(0) = 0
template <int NORM, int PEN>
__global__ __launch_bounds__(256) void gp_opt_bwd_kernel(const float* __restrict__ g, const float* __restrict__ gout,
                                                         float* __restrict__ dg, long npix, int c, float inv_npix) {
  const float gs = gout[0] * inv_npix;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
    const float nrm = gp_pixel_norm<NORM>(g, p, c);
    const float d = nrm - 1.f;
    const float f = (PEN == GP_LS ? 2.f * d : (d > 0.f ? 1.f : 0.f)) * gs;
    if (NORM == GP_L2) {
      const float r = nrm > 0.f ? f / nrm : 0.f;
      for (int j = 0; j < c; ++j) dg[p * c + j] = r * g[p * c + j];
    } else if (NORM == GP_L1) {
      for (int j = 0; j < c; ++j) {
        const float v = g[p * c + j];
        dg[p * c + j] = v > 0.f ? f : (v < 0.f ? -f : 0.f);
      }
    } else {
      bool taken = false;
      for (int j = 0; j < c; ++j) {
        const float v = g[p * c + j];
        const bool here = !taken && fabsf(v) == nrm;
        dg[p * c + j] = here ? (v > 0.f ? f : (v < 0.f ? -f : 0.f)) : 0.f;
        taken = taken || here;
      }
    }
  }
}

template <int NORM, int PEN>
static void gp_opt_launch_fwd(const float* g, float* part, int nb, long npix, int c, hipStream_t st) {
  hipLaunchKernelGGL((gp_opt_partial_kernel<NORM, PEN>), dim3(nb), dim3(256), 0, st, g, part, npix, c);
}

template <int NORM, int PEN>
static void gp_opt_launch_bwd(const float* g, const float* gout, float* dg, long npix, int c, hipStream_t st) {
  hipLaunchKernelGGL((gp_opt_bwd_kernel<NORM, PEN>), dim3(ls_blocks(npix)), dim3(256), 0, st, g, gout, dg, npix, c,
                     (float)(1.0 / (double)npix));
}

}  // namespace srhip

using namespace srhip;

extern "C" {

size_t srhip_reduce_workspace(void) { return LS_MAXB * sizeof(float); }

static int ws_ok(const char* what, void* ws, size_t bytes) {
  if (!ws || bytes < srhip_reduce_workspace()) {
    set_error("%s: workspace %zu bytes < required %zu", what, bytes, srhip_reduce_workspace());
    return 0;
  }
  return 1;
}

int srhip_l1_mean_fwd(const float* a, const float* b, float* out, void* workspace, size_t workspace_bytes, long count, void* stream) {
  SRHIP_REQUIRE(count > 0, "l1_mean_fwd: empty input");
  SRHIP_REQUIRE((((uintptr_t)a | (uintptr_t)b) & 15) == 0, "l1_mean_fwd: inputs must be 16-byte aligned");
  if (!ws_ok("l1_mean_fwd", workspace, workspace_bytes)) return SRHIP_ERR_WORKSPACE;
  const int nb = ls_blocks(count / 4 + 1);
  float* part = static_cast<float*>(workspace);
  hipLaunchKernelGGL(l1_partial_kernel, dim3(nb), dim3(256), 0, as_stream(stream), a, b, part, count);
  hipLaunchKernelGGL(finish_sum_kernel, dim3(1), dim3(256), 0, as_stream(stream), part, nb, (float)(1.0 / (double)count), out);
  return check_launch("l1_mean_fwd");
}

int srhip_l1_mean_bwd(const float* a, const float* b, const float* gout, float* da, float* db, long count, void* stream) {
  SRHIP_REQUIRE(count > 0 && da != nullptr, "l1_mean_bwd: empty input / missing output");
  hipLaunchKernelGGL(l1_bwd_kernel, dim3(ls_blocks(count)), dim3(256), 0, as_stream(stream), a, b, gout, da, db, count,
                     (float)(1.0 / (double)count));
  return check_launch("l1_mean_bwd");
}

int srhip_mse_mean_fwd(const float* a, const float* b, float* out, void* workspace, size_t workspace_bytes, long count, void* stream) {
  SRHIP_REQUIRE(count > 0, "mse_mean_fwd: empty input");
  SRHIP_REQUIRE((((uintptr_t)a | (uintptr_t)b) & 15) == 0, "mse_mean_fwd: inputs must be 16-byte aligned");
  if (!ws_ok("mse_mean_fwd", workspace, workspace_bytes)) return SRHIP_ERR_WORKSPACE;
  const int nb = ls_blocks(count / 4 + 1);
  float* part = static_cast<float*>(workspace);
  hipLaunchKernelGGL(sq_partial_kernel, dim3(nb), dim3(256), 0, as_stream(stream), a, b, part, count);
  hipLaunchKernelGGL(finish_sum_kernel, dim3(1), dim3(256), 0, as_stream(stream), part, nb, (float)(1.0 / (double)count), out);
  return check_launch("mse_mean_fwd");
}

int srhip_mse_mean_bwd(const float* a, const float* b, const float* gout, float* da, float* db, long count, void* stream) {
  SRHIP_REQUIRE(count > 0 && da != nullptr, "mse_mean_bwd: empty input / missing output");
  hipLaunchKernelGGL(sq_bwd_kernel, dim3(ls_blocks(count)), dim3(256), 0, as_stream(stream), a, b, gout, da, db, count,
                     (float)(1.0 / (double)count));
  return check_launch("mse_mean_bwd");
}

int srhip_smooth_l1_mean_fwd(const float* a, const float* b, float target, float* out, void* workspace, size_t workspace_bytes,
                             long count, void* stream) {
  SRHIP_REQUIRE(count > 0, "smooth_l1_mean_fwd: empty input");
  SRHIP_REQUIRE((((uintptr_t)a | (uintptr_t)b) & 15) == 0, "smooth_l1_mean_fwd: inputs must be 16-byte aligned");
  if (!ws_ok("smooth_l1_mean_fwd", workspace, workspace_bytes)) return SRHIP_ERR_WORKSPACE;
  const int nb = ls_blocks(count / 4 + 1);
  float* part = static_cast<float*>(workspace);
  hipLaunchKernelGGL(smooth_l1_partial_kernel, dim3(nb), dim3(256), 0, as_stream(stream), a, b, target, part, count);
  hipLaunchKernelGGL(finish_sum_kernel, dim3(1), dim3(256), 0, as_stream(stream), part, nb, (float)(1.0 / (double)count), out);
  return check_launch("smooth_l1_mean_fwd");
}

int srhip_smooth_l1_mean_bwd(const float* a, const float* b, float target, const float* gout, float* da, float* db, long count,
                             void* stream) {
  SRHIP_REQUIRE(count > 0 && da != nullptr && (b != nullptr || db == nullptr), "smooth_l1_mean_bwd: empty input / missing output");
  hipLaunchKernelGGL(smooth_l1_bwd_kernel, dim3(ls_blocks(count)), dim3(256), 0, as_stream(stream), a, b, target, gout, da, db, count,
                     (float)(1.0 / (double)count));
  return check_launch("smooth_l1_mean_bwd");
}

int srhip_mean_fwd(const float* x, float* out, void* workspace, size_t workspace_bytes, long count, void* stream) {
  SRHIP_REQUIRE(count > 0, "mean_fwd: empty input");
  if (!ws_ok("mean_fwd", workspace, workspace_bytes)) return SRHIP_ERR_WORKSPACE;
  const int nb = ls_blocks(count);
  float* part = static_cast<float*>(workspace);
  hipLaunchKernelGGL(sum_partial_kernel, dim3(nb), dim3(256), 0, as_stream(stream), x, part, count);
  hipLaunchKernelGGL(finish_sum_kernel, dim3(1), dim3(256), 0, as_stream(stream), part, nb, (float)(1.0 / (double)count), out);
  return check_launch("mean_fwd");
}

int srhip_mean_bwd(const float* gout, float* dx, long count, void* stream) {
  SRHIP_REQUIRE(count > 0, "mean_bwd: empty input");
  hipLaunchKernelGGL(fill_scaled_kernel, dim3(ls_blocks(count)), dim3(256), 0, as_stream(stream), gout, dx, count,
                     (float)(1.0 / (double)count));
  return check_launch("mean_bwd");
}

int srhip_gp_norm_penalty_fwd(const float* grads, float* out, void* workspace, size_t workspace_bytes, long npix, int c, void* stream) {
  SRHIP_REQUIRE(npix > 0 && c >= 1 && c <= 4, "gp_norm_penalty_fwd: needs npix > 0 and 1 <= C <= 4 (image channels), got %ld / %d", npix, c);
  if (!ws_ok("gp_norm_penalty_fwd", workspace, workspace_bytes)) return SRHIP_ERR_WORKSPACE;
  const int nb = ls_blocks(npix);
  float* part = static_cast<float*>(workspace);
  hipLaunchKernelGGL(gp_partial_kernel, dim3(nb), dim3(256), 0, as_stream(stream), grads, part, npix, c);
  hipLaunchKernelGGL(finish_sum_kernel, dim3(1), dim3(256), 0, as_stream(stream), part, nb, (float)(1.0 / (double)npix), out);
  return check_launch("gp_norm_penalty_fwd");
}

int srhip_gp_norm_penalty_bwd(const float* grads, const float* gout, float* dgrads, long npix, int c, void* stream) {
  SRHIP_REQUIRE(npix > 0 && c >= 1 && c <= 4, "gp_norm_penalty_bwd: needs npix > 0 and 1 <= C <= 4, got %ld / %d", npix, c);
  hipLaunchKernelGGL(gp_bwd_kernel, dim3(ls_blocks(npix)), dim3(256), 0, as_stream(stream), grads, gout, dgrads, npix, c,
                     (float)(1.0 / (double)npix));
  return check_launch("gp_norm_penalty_bwd");
}

static int gp_kinds_ok(const char* what, long npix, int c, int norm_kind, int penalty_kind) {
  if (!(npix > 0 && c >= 1 && c <= 4)) {
    set_error("%s: needs npix > 0 and 1 <= C <= 4 (image channels), got %ld / %d", what, npix, c);
    return 0;
  }
  if (norm_kind < SRHIP_GP_NORM_L2 || norm_kind > SRHIP_GP_NORM_LINF || penalty_kind < SRHIP_GP_PENALTY_LS ||
      penalty_kind > SRHIP_GP_PENALTY_HINGE) {
    set_error("%s: unknown kind: norm_kind %d (0 L2, 1 L1, 2 Linf), penalty_kind %d (0 LS, 1 hinge)", what, norm_kind, penalty_kind);
    return 0;
  }
  return 1;
}

int srhip_gp_penalty_fwd(const float* grads, float* out, void* workspace, size_t workspace_bytes, long npix, int c, int norm_kind,
                         int penalty_kind, void* stream) {
  if (!gp_kinds_ok("gp_penalty_fwd", npix, c, norm_kind, penalty_kind)) return SRHIP_ERR_ARG;
  if (!ws_ok("gp_penalty_fwd", workspace, workspace_bytes)) return SRHIP_ERR_WORKSPACE;
  const int nb = ls_blocks(npix);
  float* part = static_cast<float*>(workspace);
  hipStream_t st = as_stream(stream);
  switch (norm_kind * 2 + penalty_kind) {
    case 0: gp_opt_launch_fwd<GP_L2, GP_LS>(grads, part, nb, npix, c, st); break;
    case 1: gp_opt_launch_fwd<GP_L2, GP_HINGE>(grads, part, nb, npix, c, st); break;
    case 2: gp_opt_launch_fwd<GP_L1, GP_LS>(grads, part, nb, npix, c, st); break;
    case 3: gp_opt_launch_fwd<GP_L1, GP_HINGE>(grads, part, nb, npix, c, st); break;
    case 4: gp_opt_launch_fwd<GP_LINF, GP_LS>(grads, part, nb, npix, c, st); break;
    default: gp_opt_launch_fwd<GP_LINF, GP_HINGE>(grads, part, nb, npix, c, st); break;
  }
  hipLaunchKernelGGL(finish_sum_kernel, dim3(1), dim3(256), 0, st, part, nb, (float)(1.0 / (double)npix), out);
  return check_launch("gp_penalty_fwd");
}

int srhip_gp_penalty_bwd(const float* grads, const float* gout, float* dgrads, long npix, int c, int norm_kind, int penalty_kind,
                         void* stream) {
  if (!gp_kinds_ok("gp_penalty_bwd", npix, c, norm_kind, penalty_kind)) return SRHIP_ERR_ARG;
  hipStream_t st = as_stream(stream);
  switch (norm_kind * 2 + penalty_kind) {
    case 0: gp_opt_launch_bwd<GP_L2, GP_LS>(grads, gout, dgrads, npix, c, st); break;
    case 1: gp_opt_launch_bwd<GP_L2, GP_HINGE>(grads, gout, dgrads, npix, c, st); break;
    case 2: gp_opt_launch_bwd<GP_L1, GP_LS>(grads, gout, dgrads, npix, c, st); break;
    case 3: gp_opt_launch_bwd<GP_L1, GP_HINGE>(grads, gout, dgrads, npix, c, st); break;
    case 4: gp_opt_launch_bwd<GP_LINF, GP_LS>(grads, gout, dgrads, npix, c, st); break;
    default: gp_opt_launch_bwd<GP_LINF, GP_HINGE>(grads, gout, dgrads, npix, c, st); break;
  }
  return check_launch("gp_penalty_bwd");
}

}  // extern "C"
