// Dilated 3x3 convolutions, stride 1, pad = dilation (AMSSRN's ASPP, SRADSGAN/model/amssrn.py:200-217), as d^2 plain 3x3 convs.
//
// Polyphase identity: for y[h, w] = sum_ij W[i, j] x[h + d (i - 1), w + d (j - 1)] every tap of the output pixel (d a + p, d b + q)
// lies on the sub-grid {(d a' + p, d b' + q)}.  Sub-image (p, q) of x, xs[a, b] = x[d a + p, d b + q], convolved with W by a plain
// 3x3 pad-1 conv gives sub-image (p, q) of y, and a tap that leaves the sub-image leaves x: its zero padding is exactly the plain
// conv's.  So the d^2 sub-images become d^2 images of one batch of ceil(h / d) x ceil(w / d) pixels (positions past the end of a
// shorter sub-image are zero on the way in and dropped on the way out), and the existing 3x3 kernels of conv_api.hip run them
// unchanged: every arithmetic mode, tile shape and debug knob applies as it does to any other 3x3 conv.  The cost is one gather
// of the conv's input and one scatter of its output (two float4 HBM sweeps each), no change to any existing kernel.
//
// Backward: the data gradient is the same plain data gradient on the sub-image batch (the padded positions of dy gathered as 0,
// so they contribute nothing), the weight gradient the plain weight gradient of the gathered x and dy (bias: the column sums of dy,
// unchanged by zeros).  No atomics anywhere: reruns are bit-identical whenever the plain kernels' are.
#include "common.h"
#include "conv_internal.h"

namespace srhip {

// xs[b, a, c, :] = x[img, a d + p, c d + q, :] (0 outside x; x read as x * chanscale[img][:] when chanscale != NULL),
// b = (img d + p) d + q.  One float4 of one sub-image pixel per thread.
__global__ __launch_bounds__(256) void dil_gather_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ chanscale,
                                                         float* __restrict__ xs, int n, int h, int w, int hs, int ws, int d, int cq) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long total = (long)n * d * d * hs * ws * cq;
  if (i >= total) return;
  const int q4 = (int)(i % cq);
  long r = i / cq;
  const int c = (int)(r % ws);
  r /= ws;
  const int a = (int)(r % hs);
  const int b = (int)(r / hs);
  const int img = b / (d * d), ph = (b / d) % d, pw = b % d;
  const int hh = a * d + ph, ww = c * d + pw;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (hh < h && ww < w) {
    v = *reinterpret_cast<const float4*>(x + ((long)(img * h + hh) * w + ww) * ldx + 4 * q4);
    if (chanscale) {
      const float4 s = *reinterpret_cast<const float4*>(chanscale + (long)img * cq * 4 + 4 * q4);
      v.x *= s.x; v.y *= s.y; v.z *= s.z; v.w *= s.w;
    }
  }
  *reinterpret_cast<float4*>(xs + i * 4) = v;
}

// y[img, hh, ww, :] (=|+=) ys[b, hh / d, ww / d, :], b = (img d + hh % d) d + ww % d.  One float4 of one pixel of y per thread.
__global__ __launch_bounds__(256) void dil_scatter_kernel(const float* __restrict__ ys, float* __restrict__ y, int ldy, int n, int h, int w,
                                                          int hs, int ws, int d, int cq, int accumulate) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long total = (long)n * h * w * cq;
  if (i >= total) return;
  const int q4 = (int)(i % cq);
  long r = i / cq;
  const int ww = (int)(r % w);
  r /= w;
  const int hh = (int)(r % h);
  const int img = (int)(r / h);
  const int b = (img * d + hh % d) * d + ww % d;
  const float4 v = *reinterpret_cast<const float4*>(ys + ((long)(b * hs + hh / d) * ws + ww / d) * cq * 4 + 4 * q4);
  float4* dst = reinterpret_cast<float4*>(y + ((long)(img * h + hh) * w + ww) * ldy + 4 * q4);
  if (accumulate) {
    float4 o = *dst;
    o.x += v.x; o.y += v.y; o.z += v.z; o.w += v.w;
    *dst = o;
  } else {
    *dst = v;
  }
}

static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

static size_t sub_bytes(int n, int h, int w, int d, int c) {
  const long hs = (h + d - 1) / d, ws = (w + d - 1) / d;
  return align256((size_t)n * d * d * hs * ws * c * sizeof(float));
}

static int gather(const float* x, int ldx, const float* chanscale, float* xs, int n, int h, int w, int d, int c, hipStream_t st) {
  const int hs = (h + d - 1) / d, ws = (w + d - 1) / d;
  const long total = (long)n * d * d * hs * ws * (c / 4);
  if (total == 0) return SRHIP_OK;
  route_note(RF_DIL_GATHER, hs, ws, d, 0, 0, cdiv(total, 256));     // (bn field: the dilation)
  hipLaunchKernelGGL(dil_gather_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, x, ldx, chanscale, xs, n, h, w, hs, ws, d, c / 4);
  return check_launch("conv2d_dil: gather");
}

static int scatter(const float* ys, float* y, int ldy, int n, int h, int w, int d, int c, int accumulate, hipStream_t st) {
  const int hs = (h + d - 1) / d, ws = (w + d - 1) / d;
  const long total = (long)n * h * w * (c / 4);
  if (total == 0) return SRHIP_OK;
  route_note(RF_DIL_SCATTER, hs, ws, d, 0, 0, cdiv(total, 256));
  hipLaunchKernelGGL(dil_scatter_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, ys, y, ldy, n, h, w, hs, ws, d, c / 4, accumulate);
  return check_launch("conv2d_dil: scatter");
}

static bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

}  // namespace srhip

using namespace srhip;

extern "C" {

size_t srhip_conv2d_dil_workspace(int kind, int n, int h, int w, int cin, int cout, int dilation) {
  if (n <= 0 || h <= 0 || w <= 0 || cin <= 0 || cout <= 0 || dilation < 1 || dilation > 3) return 0;
  if (dilation == 1) return kind == 3 ? srhip_conv2d_wgrad_workspace(n, h, w, cin, cout, 3, 3, 1, 1) : 0;
  const int d = dilation, hs = (h + d - 1) / d, ws = (w + d - 1) / d;
  const size_t in_b = sub_bytes(n, h, w, d, cin), out_b = sub_bytes(n, h, w, d, cout);
  if (kind == 1 || kind == 2) return in_b + out_b;
  if (kind == 3) return in_b + out_b + align256(srhip_conv2d_wgrad_workspace(n * d * d, hs, ws, cin, cout, 3, 3, 1, 1));
  return 0;
}

int srhip_conv2d_fwd_dil(const float* x, const float* packed, const float* bias, const float* chanscale, float* y, void* workspace,
                         size_t workspace_bytes, int n, int h, int w, int cin, int cout, int dilation, int ldx, int ldy, float slope,
                         int flags, void* stream) {
  RouteScope route_scope;
  SRHIP_REQUIRE(x && packed && y, "conv2d_fwd_dil: null tensor");
  SRHIP_REQUIRE(n > 0 && h > 0 && w > 0 && cin > 0 && cout > 0 && dilation >= 1 && dilation <= 3, "conv2d_fwd_dil: bad geometry");
  SRHIP_REQUIRE(cin % 4 == 0 && cout % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && ldx >= cin && ldy >= cout && aligned16(x) && aligned16(y),
                "conv2d_fwd_dil: channels and row strides % 4 == 0, row strides >= channels, 16-byte aligned tensors");
  SRHIP_REQUIRE((flags & ~(SRHIP_EPI_BIAS | SRHIP_EPI_LRELU | SRHIP_EPI_CHANSCALE)) == 0, "conv2d_fwd_dil: bias / LeakyReLU / chanscale epilogue only");
  SRHIP_REQUIRE(!(flags & SRHIP_EPI_BIAS) || bias, "conv2d_fwd_dil: EPI_BIAS without bias");
  SRHIP_REQUIRE(!(flags & SRHIP_EPI_CHANSCALE) || (chanscale && aligned16(chanscale)), "conv2d_fwd_dil: EPI_CHANSCALE without chanscale");
  if (dilation == 1)
    return srhip_conv2d_fwd(x, packed, bias, nullptr, nullptr, chanscale, y, n, h, w, cin, cout, 3, 3, 1, 1, ldx, ldy, 0, slope, flags, stream);
  const int d = dilation, hs = (h + d - 1) / d, ws = (w + d - 1) / d;
  const size_t in_b = sub_bytes(n, h, w, d, cin);
  const size_t need = srhip_conv2d_dil_workspace(1, n, h, w, cin, cout, d);
  if (!workspace || workspace_bytes < need || !aligned16(workspace)) {
    set_error("conv2d_fwd_dil: workspace %zu bytes < required %zu (or not 16-byte aligned)", workspace_bytes, need);
    return SRHIP_ERR_WORKSPACE;
  }
  float* xs = static_cast<float*>(workspace);
  float* ys = reinterpret_cast<float*>(static_cast<char*>(workspace) + in_b);
  hipStream_t st = as_stream(stream);
  // the channel scale is applied on the way in (the plain kernels would multiply the same fp32 values before their split)
  int rc = gather(x, ldx, (flags & SRHIP_EPI_CHANSCALE) ? chanscale : nullptr, xs, n, h, w, d, cin, st);
  if (rc) return rc;
  rc = srhip_conv2d_fwd(xs, packed, bias, nullptr, nullptr, nullptr, ys, n * d * d, hs, ws, cin, cout, 3, 3, 1, 1, cin, cout, 0, slope,
                        flags & ~SRHIP_EPI_CHANSCALE, stream);
  if (rc) return rc;
  return scatter(ys, y, ldy, n, h, w, d, cout, 0, st);
}

int srhip_conv2d_dgrad_dil(const float* dy, const float* packed, float* dx, void* workspace, size_t workspace_bytes, int n, int h, int w,
                           int cin, int cout, int dilation, int ldy, int ldx, int accumulate, void* stream) {
  RouteScope route_scope;
  SRHIP_REQUIRE(dy && packed && dx, "conv2d_dgrad_dil: null tensor");
  SRHIP_REQUIRE(n > 0 && h > 0 && w > 0 && cin > 0 && cout > 0 && dilation >= 1 && dilation <= 3, "conv2d_dgrad_dil: bad geometry");
  SRHIP_REQUIRE(cin % 4 == 0 && cout % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && ldx >= cin && ldy >= cout && aligned16(dy) && aligned16(dx),
                "conv2d_dgrad_dil: channels and row strides % 4 == 0, row strides >= channels, 16-byte aligned tensors");
  if (dilation == 1)
    return srhip_conv2d_dgrad(dy, packed, dx, nullptr, nullptr, 0.f, n, h, w, cin, cout, 3, 3, 1, 1, ldy, ldx, cin, accumulate, stream);
  const int d = dilation, hs = (h + d - 1) / d, ws = (w + d - 1) / d;
  const size_t out_b = sub_bytes(n, h, w, d, cout);
  const size_t need = srhip_conv2d_dil_workspace(2, n, h, w, cin, cout, d);
  if (!workspace || workspace_bytes < need || !aligned16(workspace)) {
    set_error("conv2d_dgrad_dil: workspace %zu bytes < required %zu (or not 16-byte aligned)", workspace_bytes, need);
    return SRHIP_ERR_WORKSPACE;
  }
  float* dys = static_cast<float*>(workspace);
  float* dxs = reinterpret_cast<float*>(static_cast<char*>(workspace) + out_b);
  hipStream_t st = as_stream(stream);
  int rc = gather(dy, ldy, nullptr, dys, n, h, w, d, cout, st);
  if (rc) return rc;
  rc = srhip_conv2d_dgrad(dys, packed, dxs, nullptr, nullptr, 0.f, n * d * d, hs, ws, cin, cout, 3, 3, 1, 1, cout, cin, cin, 0, stream);
  if (rc) return rc;
  return scatter(dxs, dx, ldx, n, h, w, d, cin, accumulate, st);
}

int srhip_conv2d_wgrad_dil(const float* x, const float* dy, float* dw, float* db, int accumulate, void* workspace, size_t workspace_bytes,
                           int n, int h, int w, int cin, int cout, int dilation, int ldx, int ldy, void* stream) {
  RouteScope route_scope;
  SRHIP_REQUIRE(x && dy && dw, "conv2d_wgrad_dil: null tensor");
  SRHIP_REQUIRE(n > 0 && h > 0 && w > 0 && cin > 0 && cout > 0 && dilation >= 1 && dilation <= 3, "conv2d_wgrad_dil: bad geometry");
  SRHIP_REQUIRE(cin % 4 == 0 && cout % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && ldx >= cin && ldy >= cout && aligned16(x) && aligned16(dy),
                "conv2d_wgrad_dil: channels and row strides % 4 == 0, row strides >= channels, 16-byte aligned tensors");
  if (dilation == 1)
    return srhip_conv2d_wgrad(x, dy, dw, db, nullptr, nullptr, accumulate, workspace, workspace_bytes, n, h, w, cin, cout, 3, 3, 1, 1, ldx,
                              ldy, stream);
  const int d = dilation, hs = (h + d - 1) / d, ws = (w + d - 1) / d;
  const size_t in_b = sub_bytes(n, h, w, d, cin), out_b = sub_bytes(n, h, w, d, cout);
  const size_t need = srhip_conv2d_dil_workspace(3, n, h, w, cin, cout, d);
  if (!workspace || workspace_bytes < need || !aligned16(workspace)) {
    set_error("conv2d_wgrad_dil: workspace %zu bytes < required %zu (or not 16-byte aligned)", workspace_bytes, need);
    return SRHIP_ERR_WORKSPACE;
  }
  float* xs = static_cast<float*>(workspace);
  float* dys = reinterpret_cast<float*>(static_cast<char*>(workspace) + in_b);
  char* inner = static_cast<char*>(workspace) + in_b + out_b;
  hipStream_t st = as_stream(stream);
  int rc = gather(x, ldx, nullptr, xs, n, h, w, d, cin, st);
  if (rc) return rc;
  rc = gather(dy, ldy, nullptr, dys, n, h, w, d, cout, st);
  if (rc) return rc;
  return srhip_conv2d_wgrad(xs, dys, dw, db, nullptr, nullptr, accumulate, inner, workspace_bytes - in_b - out_b, n * d * d, hs, ws, cin,
                            cout, 3, 3, 1, 1, cin, cout, stream);
}

}  // extern "C"
