// The dihedral group (the 8 symmetries of the square) on image batches: training augmentation and x8 self-ensemble.
//   augment_u8_kernel       uint8 [N][H][W][C] -> uint8 [N][cs][cs][C]: crop + optional Gaussian noise + one of the 8 ops per
//                           sample, one fused gather (data.Augment; Dataset.__getitem__ of the reference, dataset.py:273-306)
//   dihedral_f32_kernel     one op on a float [N][H][W][C] tensor given by element strides (ensemble.py: the eight views)
//   ensemble_merge_kernel   out = (((v_0 + v_1) + ...) + v_{m-1}) * (1/m), every view read back through the inverse of its op
// Op encoding (the same everywhere): bit 0 transpose, bit 1 flip top-bottom, bit 2 flip left-right, applied in that order,
//   y = fliplr^b2(flipud^b1(transpose^b0(x))).  With (OH, OW) = the shape of y, element (i, j) of y is the element
//   (i', j') = (b1 ? OH-1-i : i, b2 ? OW-1-j : j) of transpose^b0(x), that is x[j'][i'] when b0 is set and x[i'][j'] otherwise.
// All three are exact permutations (the merge: fixed-order fp32 sums), bandwidth-bound and small next to a generator pass; reads
// are gathers out of a batch that sits in cache, stores are whole dwords.  Nothing here is tuned beyond that.
#include "common.h"
#include "philox.h"

namespace srhip {

// position in x of element (i, j) of y = op(x), y of shape oh x ow
__device__ __forceinline__ void dihedral_source(int op, int i, int j, int oh, int ow, int& sy, int& sx) {
  const int ii = (op & 2) ? oh - 1 - i : i;
  const int jj = (op & 4) ? ow - 1 - j : j;
  sy = (op & 1) ? jj : ii;
  sx = (op & 1) ? ii : jj;
}

// position in y = op(x) of element (y, x) of x (x of shape h x w): the inverse map
__device__ __forceinline__ void dihedral_dest(int op, int y, int x, int h, int w, int& i, int& j) {
  const int oh = (op & 1) ? w : h, ow = (op & 1) ? h : w;
  const int ii = (op & 1) ? x : y;
  const int jj = (op & 1) ? y : x;
  i = (op & 2) ? oh - 1 - ii : ii;
  j = (op & 4) ? ow - 1 - jj : jj;
}

// NOISE: 0 none, 1 z supplied, 2 z drawn (philox_normal4 of (seed, step), element index of the un-rotated crop)
struct AugmentArgs {
  const unsigned char* in;   // [n][h][w][c]
  const int* params;         // [n][4] = {y0, x0, op, 0}
  const float* z;            // [n][cs][cs][c] or null
  unsigned char* out;        // [n][cs][cs][c]
  int n, h, w, c, cs;
  double sigma;
  unsigned long long seed, step;
};

template <int NOISE>
__device__ __forceinline__ unsigned augment_byte(const AugmentArgs& a, int n, int y0, int x0, int op, int i, int b) {
  const int j = b / a.c, ch = b - j * a.c;
  int sy, sx;
  dihedral_source(op, i, j, a.cs, a.cs, sy, sx);
  const unsigned v = a.in[(((long)n * a.h + y0 + sy) * a.w + x0 + sx) * a.c + ch];
  if (NOISE == 0) return v;
  const long e = (((long)n * a.cs + sy) * a.cs + sx) * a.c + ch;       // element of the crop BEFORE the op
  float zv;
  if (NOISE == 1) {
    zv = a.z[e];
  } else {
    float z4[4];
    philox_normal4(a.seed, a.step, (unsigned long long)(e >> 2), z4);
    zv = z4[e & 3];
  }
  // numpy: (img + sigma * z).clip(0, 255).astype(uint8) in float64 -- the cast truncates
  const double t = fmin(fmax((double)v + a.sigma * (double)zv, 0.0), 255.0);
  return (unsigned)(int)t;
}

// One thread per dword of an output row.  A row of cs * c bytes is cut into a scalar head of 0..3 bytes up to the first byte
// whose address is a multiple of 4, whole dwords, and a scalar tail (scene.hip's partial-line writer, in bytes instead of pixels).
template <int NOISE>
__global__ void augment_u8_kernel(AugmentArgs a) {
  const int row_bytes = a.cs * a.c;
  const int groups = (row_bytes + 3) / 4 + 1;           // slot 0 = the head
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)a.n * a.cs * groups) return;
  const int g = (int)(idx % groups);
  const long row = idx / groups;                        // n * cs + i
  const int i = (int)(row % a.cs), n = (int)(row / a.cs);
  const long row_b = row * row_bytes;
  const int head = (int)((4 - (row_b & 3)) & 3);
  int bb, be;
  if (g == 0) {
    bb = 0;
    be = min(head, row_bytes);
  } else {
    bb = head + 4 * (g - 1);
    be = min(bb + 4, row_bytes);
  }
  if (bb >= be) return;
  const int y0 = a.params[4 * n], x0 = a.params[4 * n + 1], op = a.params[4 * n + 2];
  // the table lives on the device and cannot be checked by the host wrapper: a crop outside the source writes zeros
  const bool ok = y0 >= 0 && x0 >= 0 && y0 <= a.h - a.cs && x0 <= a.w - a.cs && op >= 0 && op < 8;
  unsigned char* o = a.out + row_b + bb;
  if (g > 0 && be - bb == 4) {
    unsigned word = 0;
    if (ok) {
#pragma unroll
      for (int k = 0; k < 4; ++k) word |= augment_byte<NOISE>(a, n, y0, x0, op, i, bb + k) << (8 * k);
    }
    *reinterpret_cast<unsigned*>(o) = word;             // 4-byte aligned by the choice of `head` (out itself is checked)
  } else {
    for (int k = 0; k < be - bb; ++k) o[k] = ok ? (unsigned char)augment_byte<NOISE>(a, n, y0, x0, op, i, bb + k) : (unsigned char)0;
  }
}

struct Strides4 {
  long n, c, h, w;   // element strides of a logical [N][C][H][W] tensor
};

// y = op(x).  x is [n][c][h][w] logically, y [n][c][oh][ow]; one thread per element of y (VEC = 1) or per 4 channels (VEC = 4,
// both channel strides 1).  c_inner: the channel index runs fastest in the thread index (channels-last outputs), otherwise the
// column does (NCHW outputs) -- either way neighbouring threads store neighbouring addresses.
template <int VEC>
__global__ void dihedral_f32_kernel(const float* __restrict__ x, Strides4 xs, float* __restrict__ y, Strides4 ys, int n, int c, int oh,
                                    int ow, int op, int c_inner) {
  const int cv = c / VEC;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)n * cv * oh * ow) return;
  long t = idx;
  int ch, i, j;
  if (c_inner) {
    ch = (int)(t % cv) * VEC, t /= cv;
    j = (int)(t % ow), t /= ow;
    i = (int)(t % oh), t /= oh;
  } else {
    j = (int)(t % ow), t /= ow;
    i = (int)(t % oh), t /= oh;
    ch = (int)(t % cv) * VEC, t /= cv;
  }
  const long b = t;
  int sy, sx;
  dihedral_source(op, i, j, oh, ow, sy, sx);
  const float* src = x + b * xs.n + ch * xs.c + sy * xs.h + sx * xs.w;
  float* dst = y + b * ys.n + ch * ys.c + i * ys.h + j * ys.w;
  if (VEC == 4)
    *reinterpret_cast<f32x4*>(dst) = *reinterpret_cast<const f32x4*>(src);
  else
    *dst = *src;
}

constexpr int MERGE_MAX_VIEWS = 8;

struct MergeArgs {
  const float* v[MERGE_MAX_VIEWS];
  Strides4 vs[MERGE_MAX_VIEWS];
  int op[MERGE_MAX_VIEWS];
  int m;
  float inv_m;
};

// out [n][c][h][w] (strides os); view k has the shape of op_k(out) and is read at the position op_k sends (y, x) to
__global__ void ensemble_merge_kernel(MergeArgs a, float* __restrict__ out, Strides4 os, int n, int c, int h, int w, int c_inner) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)n * c * h * w) return;
  long t = idx;
  int ch, y, x;
  if (c_inner) {
    ch = (int)(t % c), t /= c;
    x = (int)(t % w), t /= w;
    y = (int)(t % h), t /= h;
  } else {
    x = (int)(t % w), t /= w;
    y = (int)(t % h), t /= h;
    ch = (int)(t % c), t /= c;
  }
  const long b = t;
  float acc = 0.0f;
#pragma unroll
  for (int k = 0; k < MERGE_MAX_VIEWS; ++k) {
    if (k < a.m) {
      int i, j;
      dihedral_dest(a.op[k], y, x, h, w, i, j);
      const float v = a.v[k][b * a.vs[k].n + ch * a.vs[k].c + i * a.vs[k].h + j * a.vs[k].w];
      acc = k == 0 ? v : acc + v;
    }
  }
  out[b * os.n + ch * os.c + y * os.h + x * os.w] = acc * a.inv_m;
}

// largest element offset of a [n][c][h][w] tensor with these strides must stay addressable with the 32-bit factors above
static bool strides_ok(const long* s) { return s[0] >= 0 && s[1] >= 0 && s[2] >= 0 && s[3] >= 0; }

}  // namespace srhip

using namespace srhip;

extern "C" {

int srhip_augment_u8(const unsigned char* in, const int* params_dev, const float* z, unsigned char* out, int n, int h, int w, int c,
                     int cs, double sigma, int drawn, unsigned long long seed, unsigned long long step, void* stream) {
  SRHIP_REQUIRE(in && params_dev && out, "augment_u8: null tensor");
  SRHIP_REQUIRE(n > 0 && h > 0 && w > 0 && c > 0 && c <= 4 && cs > 0, "augment_u8: bad size (n %d, %dx%dx%d, crop %d)", n, h, w, c, cs);
  SRHIP_REQUIRE(cs <= h && cs <= w, "augment_u8: crop %d does not fit the %dx%d source", cs, h, w);
  SRHIP_REQUIRE(((size_t)out & 3) == 0, "augment_u8: the output must be 4-byte aligned");
  SRHIP_REQUIRE(!(z && drawn), "augment_u8: noise is either supplied (z) or drawn, not both");
  SRHIP_REQUIRE(sigma == sigma && sigma >= 0.0, "augment_u8: sigma must be a non-negative number");
  SRHIP_REQUIRE(sigma == 0.0 || z || drawn, "augment_u8: sigma > 0 needs z or drawn != 0");
  SRHIP_REQUIRE(((size_t)z & 3) == 0, "augment_u8: z must be 4-byte aligned");
  const long total = (long)n * cs * (((long)cs * c + 3) / 4 + 1);
  SRHIP_REQUIRE((long)n * h * w * c < (1L << 40) && total / 256 < 0x7fffffffL, "augment_u8: batch too large for one launch");
  AugmentArgs a{in, params_dev, z, out, n, h, w, c, cs, sigma, seed, step};
  const dim3 grid((unsigned)cdiv(total, 256)), block(256);
  if (sigma == 0.0)                                     // no noise path at all
    hipLaunchKernelGGL(augment_u8_kernel<0>, grid, block, 0, as_stream(stream), a);
  else if (z)
    hipLaunchKernelGGL(augment_u8_kernel<1>, grid, block, 0, as_stream(stream), a);
  else
    hipLaunchKernelGGL(augment_u8_kernel<2>, grid, block, 0, as_stream(stream), a);
  return check_launch("augment_u8");
}

int srhip_dihedral_f32(const float* x, const long* x_strides, float* y, const long* y_strides, int n, int c, int h, int w, int op,
                       void* stream) {
  SRHIP_REQUIRE(x && y && x_strides && y_strides, "dihedral_f32: null tensor");
  SRHIP_REQUIRE(n > 0 && c > 0 && h > 0 && w > 0, "dihedral_f32: bad size");
  SRHIP_REQUIRE(op >= 0 && op < 8, "dihedral_f32: op %d outside 0..7", op);
  SRHIP_REQUIRE(strides_ok(x_strides) && strides_ok(y_strides), "dihedral_f32: negative stride");
  SRHIP_REQUIRE(x != y, "dihedral_f32: not in place");
  const Strides4 xs{x_strides[0], x_strides[1], x_strides[2], x_strides[3]}, ys{y_strides[0], y_strides[1], y_strides[2], y_strides[3]};
  const int oh = (op & 1) ? w : h, ow = (op & 1) ? h : w;
  const long total = (long)n * c * h * w;
  SRHIP_REQUIRE(total / 256 < 0x7fffffffL, "dihedral_f32: tensor too large for one launch");
  const int c_inner = ys.c == 1 && c > 1;
  auto mult4 = [](const Strides4& s) { return !(s.n & 3) && !(s.h & 3) && !(s.w & 3); };
  const bool vec = c % 4 == 0 && xs.c == 1 && ys.c == 1 && mult4(xs) && mult4(ys) && !((size_t)x & 15) && !((size_t)y & 15);
  if (vec)
    hipLaunchKernelGGL(dihedral_f32_kernel<4>, dim3((unsigned)cdiv(total / 4, 256)), dim3(256), 0, as_stream(stream), x, xs, y, ys, n,
                       c, oh, ow, op, 1);
  else
    hipLaunchKernelGGL(dihedral_f32_kernel<1>, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, as_stream(stream), x, xs, y, ys, n, c,
                       oh, ow, op, c_inner);
  return check_launch("dihedral_f32");
}

int srhip_ensemble_merge_f32(const float* const* views, const long* view_strides, const int* ops, int m, float* out,
                             const long* out_strides, int n, int c, int h, int w, void* stream) {
  SRHIP_REQUIRE(views && view_strides && ops && out && out_strides, "ensemble_merge_f32: null tensor");
  SRHIP_REQUIRE(m >= 1 && m <= MERGE_MAX_VIEWS, "ensemble_merge_f32: %d views, takes 1..%d", m, MERGE_MAX_VIEWS);
  SRHIP_REQUIRE(n > 0 && c > 0 && h > 0 && w > 0, "ensemble_merge_f32: bad size");
  SRHIP_REQUIRE(strides_ok(out_strides), "ensemble_merge_f32: negative stride");
  MergeArgs a{};
  for (int k = 0; k < m; ++k) {
    SRHIP_REQUIRE(views[k] && views[k] != out, "ensemble_merge_f32: view %d is null or the output", k);
    SRHIP_REQUIRE(ops[k] >= 0 && ops[k] < 8, "ensemble_merge_f32: op %d of view %d outside 0..7", ops[k], k);
    SRHIP_REQUIRE(strides_ok(view_strides + 4 * k), "ensemble_merge_f32: negative stride");
    a.v[k] = views[k];
    a.vs[k] = Strides4{view_strides[4 * k], view_strides[4 * k + 1], view_strides[4 * k + 2], view_strides[4 * k + 3]};
    a.op[k] = ops[k];
  }
  a.m = m;
  a.inv_m = 1.0f / (float)m;
  const Strides4 os{out_strides[0], out_strides[1], out_strides[2], out_strides[3]};
  const long total = (long)n * c * h * w;
  SRHIP_REQUIRE(total / 256 < 0x7fffffffL, "ensemble_merge_f32: tensor too large for one launch");
  hipLaunchKernelGGL(ensemble_merge_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, as_stream(stream), a, out, os, n, c, h, w,
                     os.c == 1 && c > 1);
  return check_launch("ensemble_merge_f32");
}

}  // extern "C"
