// NDSRGAN's element-wise passes (SRADSGAN/model/ndsrgan.py:57-211): the scaled residuals of DenseBlock / DCRDB / DRRDBnet with
// their running trunk sums, the LeakyReLU backward over one CL's channel slice of a dense-block buffer, and
// nn.UpsamplingNearest2d(r).  Every pass is one HBM sweep with 16-byte accesses; every operand of the residual passes has its own
// row stride, so a result can land in channels 0:64 of the next dense block's [n, h, w, 192] buffer.  No atomics: reruns are
// bit-identical.
#include "common.h"

namespace srhip {

// y = r + alpha * c (c == NULL: y = r), z = s + beta * y; y / z skipped when NULL.  One float4 of one pixel per thread.
// Operation order of the reference: `out1 + x * 0.2` (:75), `x + 0.2 * out1` (:89-91, 121-146).
__global__ __launch_bounds__(256) void scaled_res_fwd_kernel(const float* __restrict__ r, int ldr, const float* __restrict__ c, int ldc,
                                                             const float* __restrict__ s, int lds, float alpha, float beta,
                                                             float* __restrict__ y, int ldy, float* __restrict__ z, int ldz,
                                                             long rows, int cq) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * cq) return;
  const long p = i / cq;
  const int q = (int)(i - p * cq) * 4;
  float4 v = *reinterpret_cast<const float4*>(r + p * ldr + q);
  if (c) {
    const float4 cv = *reinterpret_cast<const float4*>(c + p * ldc + q);
    v.x = v.x + cv.x * alpha; v.y = v.y + cv.y * alpha; v.z = v.z + cv.z * alpha; v.w = v.w + cv.w * alpha;
  }
  if (y) *reinterpret_cast<float4*>(y + p * ldy + q) = v;
  if (z) {
    const float4 sv = *reinterpret_cast<const float4*>(s + p * lds + q);
    float4 o;
    o.x = sv.x + beta * v.x; o.y = sv.y + beta * v.y; o.z = sv.z + beta * v.z; o.w = sv.w + beta * v.w;
    *reinterpret_cast<float4*>(z + p * ldz + q) = o;
  }
}

// dc = ka * dz (dc != NULL); dr[0:ch] = kb * dz (+ kc * e), dr[ch:width] = 0 (dr != NULL).  One float4 of a dr row per thread
// (width = ch when dr is NULL).
__global__ __launch_bounds__(256) void scaled_res_bwd_kernel(const float* __restrict__ dz, int ldz, const float* __restrict__ e, int lde,
                                                             float ka, float kb, float kc, float* __restrict__ dc, int ldc,
                                                             float* __restrict__ dr, int ldr, long rows, int cq, int wq) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * wq) return;
  const long p = i / wq;
  const int q = (int)(i - p * wq) * 4;
  if (q >= cq * 4) {
    *reinterpret_cast<float4*>(dr + p * ldr + q) = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  const float4 g = *reinterpret_cast<const float4*>(dz + p * ldz + q);
  if (dc) *reinterpret_cast<float4*>(dc + p * ldc + q) = make_float4(ka * g.x, ka * g.y, ka * g.z, ka * g.w);
  if (dr) {
    float4 o = make_float4(kb * g.x, kb * g.y, kb * g.z, kb * g.w);
    if (e) {
      const float4 ev = *reinterpret_cast<const float4*>(e + p * lde + q);
      o.x = o.x + kc * ev.x; o.y = o.y + kc * ev.y; o.z = o.z + kc * ev.z; o.w = o.w + kc * ev.w;
    }
    *reinterpret_cast<float4*>(dr + p * ldr + q) = o;
  }
}

// dx = dy * (y > 0 ? 1 : slope) over ch channels of rows with their own strides (in place when dx == dy)
__global__ __launch_bounds__(256) void lrelu_bwd_strided_kernel(const float* dy, int ldg, const float* __restrict__ y, int ldy,
                                                                float* dx, int ldx, float slope, long rows, int cq) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * cq) return;
  const long p = i / cq;
  const int q = (int)(i - p * cq) * 4;
  const float4 g = *reinterpret_cast<const float4*>(dy + p * ldg + q);
  const float4 a = *reinterpret_cast<const float4*>(y + p * ldy + q);
  float4 o;
  o.x = a.x > 0.f ? g.x : g.x * slope; o.y = a.y > 0.f ? g.y : g.y * slope;
  o.z = a.z > 0.f ? g.z : g.z * slope; o.w = a.w > 0.f ? g.w : g.w * slope;
  *reinterpret_cast<float4*>(dx + p * ldx + q) = o;
}

// y[b, oy, ox] = x[b, oy / r, ox / r]: one float4 of one output pixel per thread
__global__ __launch_bounds__(256) void upsample_nearest_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int n, int h, int w,
                                                                   int cq, int r) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int wo = w * r, ho = h * r;
  if (i >= (long)n * ho * wo * cq) return;
  const int q = (int)(i % cq);
  const long op = i / cq;
  const int ox = (int)(op % wo);
  const long t = op / wo;
  const int oy = (int)(t % ho);
  const int b = (int)(t / ho);
  const long ip = ((long)b * h + oy / r) * w + ox / r;
  reinterpret_cast<float4*>(y)[op * cq + q] = reinterpret_cast<const float4*>(x)[ip * cq + q];
}

// dx[b, iy, ix] = sum over the r x r block of dy, rows then columns in order (fixed order, no atomics)
__global__ __launch_bounds__(256) void upsample_nearest_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int n, int h, int w,
                                                                   int cq, int r) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)n * h * w * cq) return;
  const int q = (int)(i % cq);
  const long ip = i / cq;
  const int ix = (int)(ip % w);
  const long t = ip / w;
  const int iy = (int)(t % h);
  const int b = (int)(t / h);
  const int wo = w * r;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int a = 0; a < r; ++a) {
    const long row = ((long)b * h * r + iy * r + a) * wo + (long)ix * r;
    for (int e = 0; e < r; ++e) {
      const float4 g = reinterpret_cast<const float4*>(dy)[(row + e) * cq + q];
      acc.x += g.x; acc.y += g.y; acc.z += g.z; acc.w += g.w;
    }
  }
  reinterpret_cast<float4*>(dx)[ip * cq + q] = acc;
}

static inline bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

}  // namespace srhip

using namespace srhip;

extern "C" {

int srhip_scaled_res_fwd(const float* r, int ldr, const float* c, int ldc, const float* s, int lds, float alpha, float beta, float* y,
                         int ldy, float* z, int ldz, long rows, int ch, void* stream) {
  SRHIP_REQUIRE(r && (y || z) && (!z || s) && rows > 0 && ch > 0 && ch % 4 == 0, "scaled_res_fwd: bad arguments");
  SRHIP_REQUIRE(ldr >= ch && ldr % 4 == 0 && (!c || (ldc >= ch && ldc % 4 == 0)) && (!s || (lds >= ch && lds % 4 == 0)) &&
                    (!y || (ldy >= ch && ldy % 4 == 0)) && (!z || (ldz >= ch && ldz % 4 == 0)),
                "scaled_res_fwd: row strides must be >= ch and multiples of 4");
  SRHIP_REQUIRE(al16(r) && al16(c) && al16(s) && al16(y) && al16(z), "scaled_res_fwd: 16-byte aligned tensors");
  const long total = rows * (ch / 4);
  hipLaunchKernelGGL(scaled_res_fwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, as_stream(stream), r, ldr, c, ldc, s, lds, alpha, beta, y,
                     ldy, z, ldz, rows, ch / 4);
  return check_launch("scaled_res_fwd");
}

int srhip_scaled_res_bwd(const float* dz, int ldz, const float* e, int lde, float ka, float kb, float kc, float* dc, int ldc, float* dr,
                         int ldr, int width, long rows, int ch, void* stream) {
  SRHIP_REQUIRE(dz && (dc || dr) && rows > 0 && ch > 0 && ch % 4 == 0, "scaled_res_bwd: bad arguments");
  SRHIP_REQUIRE(width % 4 == 0 && width >= ch && (dr ? ldr >= width : width == ch), "scaled_res_bwd: width must be >= ch, <= ldr");
  SRHIP_REQUIRE(ldz >= ch && ldz % 4 == 0 && (!e || (lde >= ch && lde % 4 == 0)) && (!dc || (ldc >= ch && ldc % 4 == 0)) &&
                    (!dr || ldr % 4 == 0),
                "scaled_res_bwd: row strides must be >= ch and multiples of 4");
  SRHIP_REQUIRE(al16(dz) && al16(e) && al16(dc) && al16(dr), "scaled_res_bwd: 16-byte aligned tensors");
  const long total = rows * (width / 4);
  hipLaunchKernelGGL(scaled_res_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, as_stream(stream), dz, ldz, e, lde, ka, kb, kc, dc, ldc,
                     dr, ldr, rows, ch / 4, width / 4);
  return check_launch("scaled_res_bwd");
}

int srhip_lrelu_bwd_strided(const float* dy, int ldg, const float* y, int ldy, float* dx, int ldx, float slope, long rows, int ch,
                            void* stream) {
  SRHIP_REQUIRE(dy && y && dx && rows > 0 && ch > 0 && ch % 4 == 0, "lrelu_bwd_strided: bad arguments");
  SRHIP_REQUIRE(ldg >= ch && ldy >= ch && ldx >= ch && (ldg | ldy | ldx) % 4 == 0, "lrelu_bwd_strided: row strides");
  SRHIP_REQUIRE(al16(dy) && al16(y) && al16(dx), "lrelu_bwd_strided: 16-byte aligned tensors");
  SRHIP_REQUIRE(ldx == ldg, "lrelu_bwd_strided: dy and dx must have one row stride, in place (dx == dy) or not");
  const long total = rows * (ch / 4);
  hipLaunchKernelGGL(lrelu_bwd_strided_kernel, dim3(cdiv(total, 256)), dim3(256), 0, as_stream(stream), dy, ldg, y, ldy, dx, ldx, slope,
                     rows, ch / 4);
  return check_launch("lrelu_bwd_strided");
}

int srhip_upsample_nearest_fwd(const float* x, float* y, int n, int h, int w, int c, int r, void* stream) {
  SRHIP_REQUIRE(x && y && n > 0 && h > 0 && w > 0 && c > 0 && c % 4 == 0 && (r == 2 || r == 3), "upsample_nearest_fwd: bad arguments");
  SRHIP_REQUIRE(al16(x) && al16(y), "upsample_nearest_fwd: 16-byte aligned tensors");
  const long total = (long)n * h * r * w * r * (c / 4);
  hipLaunchKernelGGL(upsample_nearest_fwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, as_stream(stream), x, y, n, h, w, c / 4, r);
  return check_launch("upsample_nearest_fwd");
}

int srhip_upsample_nearest_bwd(const float* dy, float* dx, int n, int h, int w, int c, int r, void* stream) {
  SRHIP_REQUIRE(dy && dx && n > 0 && h > 0 && w > 0 && c > 0 && c % 4 == 0 && (r == 2 || r == 3), "upsample_nearest_bwd: bad arguments");
  SRHIP_REQUIRE(al16(dy) && al16(dx), "upsample_nearest_bwd: 16-byte aligned tensors");
  const long total = (long)n * h * w * (c / 4);
  hipLaunchKernelGGL(upsample_nearest_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, as_stream(stream), dy, dx, n, h, w, c / 4, r);
  return check_launch("upsample_nearest_bwd");
}

}  // extern "C"
