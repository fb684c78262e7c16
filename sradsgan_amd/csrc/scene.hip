// Whole-scene super-resolution in overlapping tiles (sradsgan_amd/scene.py): the two per-tile steps outside the generator.
//   scene_tiles_kernel  uint8 HWC scene -> one float batch of tiles, data.to_tensor's layout and value (NHWC, value / 255)
//   scene_blend_kernel  float SR tiles -> feathered blend -> uint8 HWC (or the un-quantised fp32 blend), gather form:
//                       one output pixel walks the tiles that cover it in row-major tile order, so the result does not
//                       depend on launch order (no atomics)
// Both are bandwidth-bound and tiny next to the generator; nothing here is tuned beyond coalesced rows and dword stores.
#include "common.h"

namespace srhip {

// dst [n][th][tw][3] float; origins [n][2] = (y, x) of every tile in the scene.  One thread per output element: the 3*tw
// bytes of a tile row are contiguous in the scene, and so are its floats in dst.  An origin outside the scene (the host
// wrapper refuses it; the device copy cannot be checked there) writes zeros instead of reading out of bounds.
__global__ void scene_tiles_kernel(const unsigned char* __restrict__ scene, int h, int w, const int* __restrict__ origins,
                                   long total, int th, int tw, float* __restrict__ dst) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int row_elems = tw * 3;
  const int e = (int)(idx % row_elems);
  long t = idx / row_elems;
  const int y = (int)(t % th);
  const int tile = (int)(t / th);
  const int y0 = origins[2 * tile], x0 = origins[2 * tile + 1];
  float v = 0.0f;
  if (y0 >= 0 && x0 >= 0 && y0 <= h - th && x0 <= w - tw)
    v = (float)scene[((long)(y0 + y) * w + x0) * 3 + e] / 255.0f;   // srhip_u8_to_float's expression: the same bits
  dst[idx] = v;
}

struct BlendArgs {
  const float* const* tiles;   // [depth][nx] base pointer of every tile held in the ring; tile row j lives in slot j % depth
  int depth;
  long sc, sy, sx;             // element strides of one tile: channel, row, column
  const int* ycover;           // [hr_h][2] first and one-past-last tile row covering an HR row
  const int* xcover;           // [hr_w][2] the same per HR column
  const int* ay;               // [ny] HR origin of every tile row
  const int* ax;               // [nx] HR origin of every tile column
  const float* wy;             // [ny][th] feather weights per tile row
  const float* wx;             // [nx][tw]
  int ny, nx, th, tw, hr_h, hr_w;
};

// fp32: out = (sum_k w_k v_k) / (sum_k w_k), k over the covering tiles in row-major tile order, w_k = wy * wx
__device__ __forceinline__ void blend_pixel(const BlendArgs& a, int y, int x, float out[3]) {
  float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f, wsum = 0.0f;
  const int j0 = max(a.ycover[2 * y], 0), j1 = min(a.ycover[2 * y + 1], a.ny);
  const int i0 = max(a.xcover[2 * x], 0), i1 = min(a.xcover[2 * x + 1], a.nx);
  for (int j = j0; j < j1; ++j) {
    const int qy = y - a.ay[j];
    if (qy < 0 || qy >= a.th) continue;          // inconsistent tables must not become an out-of-bounds read
    const float wyv = a.wy[(long)j * a.th + qy];
    const float* const* slot = a.tiles + (long)(j % a.depth) * a.nx;
    for (int i = i0; i < i1; ++i) {
      const int qx = x - a.ax[i];
      if (qx < 0 || qx >= a.tw) continue;
      const float* p = slot[i];
      if (!p) continue;
      const float wgt = wyv * a.wx[(long)i * a.tw + qx];
      p += (long)qy * a.sy + (long)qx * a.sx;
      acc0 += wgt * p[0];
      acc1 += wgt * p[a.sc];
      acc2 += wgt * p[2 * a.sc];
      wsum += wgt;
    }
  }
  out[0] = acc0 / wsum;
  out[1] = acc1 / wsum;
  out[2] = acc2 / wsum;
}

// save_img1: trunc(clamp(255 v, 0, 255)); fmaxf drops a NaN operand, so NaN -> 0
__device__ __forceinline__ unsigned quant_u8(float v) { return (unsigned)fminf(fmaxf(255.0f * v, 0.0f), 255.0f); }

// HR rows [row0, row1).  A row is cut into a scalar head of 0..3 pixels up to the first pixel whose byte address is a
// multiple of 4, groups of 4 pixels = 12 bytes = 3 whole dwords, and a scalar tail; one thread per head / group.
__global__ void scene_blend_kernel(BlendArgs a, int row0, int row1, unsigned char* __restrict__ out_u8,
                                   float* __restrict__ out_f32) {
  const int groups = (a.hr_w + 3) / 4 + 1;       // slot 0 = the head
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)(row1 - row0) * groups) return;
  const int y = row0 + (int)(idx / groups);
  const int g = (int)(idx % groups);
  const long row_px = (long)y * a.hr_w;
  const int head = (int)((4 - (row_px & 3)) & 3);  // 3 (row_px + head) % 4 == 0  <=>  (row_px + head) % 4 == 0
  int xb, xe;
  if (g == 0) {
    xb = 0;
    xe = min(head, a.hr_w);
  } else {
    xb = head + 4 * (g - 1);
    xe = min(xb + 4, a.hr_w);
  }
  if (xb >= xe) return;
  float v[4][3];
  for (int k = 0; k < xe - xb; ++k) blend_pixel(a, y, xb + k, v[k]);
  if (out_f32) {
    float* o = out_f32 + (row_px + xb) * 3;
    for (int k = 0; k < xe - xb; ++k) {
      o[3 * k] = v[k][0];
      o[3 * k + 1] = v[k][1];
      o[3 * k + 2] = v[k][2];
    }
  }
  if (out_u8) {
    unsigned char* o = out_u8 + (row_px + xb) * 3;
    if (g > 0 && xe - xb == 4) {
      unsigned b[12];
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) b[3 * k + c] = quant_u8(v[k][c]);
      unsigned* o4 = reinterpret_cast<unsigned*>(o);   // 4-byte aligned by the choice of `head` (out_u8 itself is checked)
#pragma unroll
      for (int d = 0; d < 3; ++d) o4[d] = b[4 * d] | (b[4 * d + 1] << 8) | (b[4 * d + 2] << 16) | (b[4 * d + 3] << 24);
    } else {
      for (int k = 0; k < xe - xb; ++k)
        for (int c = 0; c < 3; ++c) o[3 * k + c] = (unsigned char)quant_u8(v[k][c]);
    }
  }
}

}  // namespace srhip

using namespace srhip;

extern "C" {

int srhip_scene_tiles_u8(const unsigned char* scene, int h, int w, const int* origins_dev, int n, int th, int tw, float* dst,
                         void* stream) {
  SRHIP_REQUIRE(scene && origins_dev && dst, "scene_tiles_u8: null tensor");
  SRHIP_REQUIRE(h > 0 && w > 0 && n > 0 && th > 0 && tw > 0 && th <= h && tw <= w, "scene_tiles_u8: tile %dx%d does not fit scene %dx%d",
                th, tw, h, w);
  const long total = (long)n * th * tw * 3;
  SRHIP_REQUIRE(total / 256 < 0x7fffffffL, "scene_tiles_u8: batch too large for one launch");
  hipLaunchKernelGGL(scene_tiles_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, as_stream(stream), scene, h, w,
                     origins_dev, total, th, tw, dst);
  return check_launch("scene_tiles_u8");
}

int srhip_scene_blend_u8(const float* const* tiles_dev, int depth, long sc, long sy, long sx, const int* ycover_dev,
                         const int* xcover_dev, const int* ay_dev, const int* ax_dev, const float* wy_dev, const float* wx_dev,
                         int ny, int nx, int th, int tw, int hr_h, int hr_w, int row0, int row1, unsigned char* out_u8,
                         float* out_f32, void* stream) {
  SRHIP_REQUIRE(tiles_dev && ycover_dev && xcover_dev && ay_dev && ax_dev && wy_dev && wx_dev, "scene_blend_u8: null tensor");
  SRHIP_REQUIRE(out_u8 || out_f32, "scene_blend_u8: no output");
  SRHIP_REQUIRE(((size_t)out_u8 & 3) == 0, "scene_blend_u8: the uint8 output must be 4-byte aligned");
  SRHIP_REQUIRE(depth > 0 && ny > 0 && nx > 0 && th > 0 && tw > 0 && hr_h > 0 && hr_w > 0, "scene_blend_u8: bad size");
  SRHIP_REQUIRE(0 <= row0 && row0 <= row1 && row1 <= hr_h, "scene_blend_u8: rows [%d, %d) outside [0, %d)", row0, row1, hr_h);
  if (row0 == row1) return SRHIP_OK;
  BlendArgs a{tiles_dev, depth, sc, sy, sx, ycover_dev, xcover_dev, ay_dev, ax_dev, wy_dev, wx_dev, ny, nx, th, tw, hr_h, hr_w};
  const long total = (long)(row1 - row0) * ((hr_w + 3) / 4 + 1);
  SRHIP_REQUIRE(total / 256 < 0x7fffffffL, "scene_blend_u8: band too large for one launch");
  hipLaunchKernelGGL(scene_blend_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, as_stream(stream), a, row0, row1,
                     out_u8, out_f32);
  return check_launch("scene_blend_u8");
}

}  // extern "C"
