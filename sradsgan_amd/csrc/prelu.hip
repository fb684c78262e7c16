// nn.PReLU() with one learnable slope (AMSSRN, SRADSGAN/model/amssrn.py:176, 189, 212) as stand-alone passes over rows of their own
// stride, so a result can land in its channel slice of a wider buffer (ASPP's [n, h, w, 768] concatenation) without a copy.
//   forward   y = z > 0 ? z : a z
//   backward  dz = z > 0 ? g : a g,   da = sum (z > 0 ? 0 : z g)
// The slope a stays on the device: the passes read it from a pointer, so no host synchronisation is needed.  The slope gradient is
// PRELU_PARTS fixed-order block partials per backward call plus one reduce over any number of them (a slope shared by several
// PReLU applications reduces all their partials at once); no atomics, reruns are bit-identical.  The backward works from the
// pre-activation z, not from the sign of y: it stays right when training drives the slope to 0 or below.
#include "common.h"

namespace srhip {

constexpr int PRELU_PARTS = 512;

__global__ __launch_bounds__(256) void prelu_fwd_kernel(const float* z, int ldz, float* y, int ldy, const float* __restrict__ slope, long rows,
                                                        int cq) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * cq) return;
  const long p = i / cq;
  const int q = (int)(i - p * cq) * 4;
  const float a = *slope;
  const float4 v = *reinterpret_cast<const float4*>(z + p * ldz + q);
  float4 o;
  o.x = v.x > 0.f ? v.x : a * v.x; o.y = v.y > 0.f ? v.y : a * v.y;
  o.z = v.z > 0.f ? v.z : a * v.z; o.w = v.w > 0.f ? v.w : a * v.w;
  *reinterpret_cast<float4*>(y + p * ldy + q) = o;
}

// grid = PRELU_PARTS blocks walking the float4 items in a fixed stride; block b writes partials[b]
__global__ __launch_bounds__(256) void prelu_bwd_kernel(const float* g, int ldg, const float* z, int ldz, float* dz, int lddz,
                                                        const float* __restrict__ slope, float* __restrict__ partials, long rows, int cq) {
  __shared__ float red[4];
  const float a = *slope;
  const long total = rows * cq;
  float acc = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)PRELU_PARTS * 256) {
    const long p = i / cq;
    const int q = (int)(i - p * cq) * 4;
    const float4 gv = *reinterpret_cast<const float4*>(g + p * ldg + q);
    const float4 zv = *reinterpret_cast<const float4*>(z + p * ldz + q);
    float4 o;
    o.x = zv.x > 0.f ? gv.x : a * gv.x; o.y = zv.y > 0.f ? gv.y : a * gv.y;
    o.z = zv.z > 0.f ? gv.z : a * gv.z; o.w = zv.w > 0.f ? gv.w : a * gv.w;
    acc += zv.x > 0.f ? 0.f : zv.x * gv.x;
    acc += zv.y > 0.f ? 0.f : zv.y * gv.y;
    acc += zv.z > 0.f ? 0.f : zv.z * gv.z;
    acc += zv.w > 0.f ? 0.f : zv.w * gv.w;
    *reinterpret_cast<float4*>(dz + p * lddz + q) = o;
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// da (=|+=) sum of nparts partials, in a fixed order (one block)
__global__ __launch_bounds__(256) void prelu_slope_reduce_kernel(const float* __restrict__ partials, int nparts, float* da, int accumulate) {
  __shared__ float red[4];
  float acc = 0.f;
  for (int i = threadIdx.x; i < nparts; i += 256) acc += partials[i];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float s = ((red[0] + red[1]) + red[2]) + red[3];
    *da = accumulate ? *da + s : s;
  }
}

static bool prelu_args_ok(const void* a, const void* b, int lda, int ldb, int ch) {
  return ch > 0 && ch % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 && lda >= ch && ldb >= ch && ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0;
}

}  // namespace srhip

using namespace srhip;

extern "C" {

int srhip_prelu_parts(void) { return PRELU_PARTS; }

int srhip_prelu_fwd(const float* z, int ldz, float* y, int ldy, const float* slope, long rows, int ch, void* stream) {
  SRHIP_REQUIRE(z && y && slope && rows >= 0, "prelu_fwd: null tensor or bad size");
  SRHIP_REQUIRE(prelu_args_ok(z, y, ldz, ldy, ch), "prelu_fwd: channels and row strides % 4 == 0, row strides >= channels, 16-byte aligned");
  SRHIP_REQUIRE(z != y || ldz == ldy, "prelu_fwd: in place needs equal row strides");
  const long total = rows * (ch / 4);
  if (total == 0) return SRHIP_OK;
  hipLaunchKernelGGL(prelu_fwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, as_stream(stream), z, ldz, y, ldy, slope, rows, ch / 4);
  return check_launch("prelu_fwd");
}

int srhip_prelu_bwd(const float* g, int ldg, const float* z, int ldz, float* dz, int lddz, const float* slope, float* partials, long rows,
                    int ch, void* stream) {
  SRHIP_REQUIRE(g && z && dz && slope && partials && rows >= 0, "prelu_bwd: null tensor or bad size");
  SRHIP_REQUIRE(prelu_args_ok(g, z, ldg, ldz, ch) && prelu_args_ok(dz, dz, lddz, lddz, ch),
                "prelu_bwd: channels and row strides % 4 == 0, row strides >= channels, 16-byte aligned");
  SRHIP_REQUIRE(z != dz || ldz == lddz, "prelu_bwd: in place over z needs equal row strides");
  SRHIP_REQUIRE(g != dz || ldg == lddz, "prelu_bwd: in place over g needs equal row strides");
  hipLaunchKernelGGL(prelu_bwd_kernel, dim3(PRELU_PARTS), dim3(256), 0, as_stream(stream), g, ldg, z, ldz, dz, lddz, slope, partials, rows,
                     ch / 4);
  return check_launch("prelu_bwd");
}

int srhip_prelu_slope_reduce(const float* partials, int nparts, float* da, int accumulate, void* stream) {
  SRHIP_REQUIRE(partials && da && nparts > 0, "prelu_slope_reduce: null tensor or no partials");
  hipLaunchKernelGGL(prelu_slope_reduce_kernel, dim3(1), dim3(256), 0, as_stream(stream), partials, nparts, da, accumulate);
  return check_launch("prelu_slope_reduce");
}

}  // extern "C"
