// ESRGAN's pieces that no other model here needs (SRADSGAN/model/architecture.py, model/sradsgan.py:35-67, :840-844, :868-878):
//   * the GAN criteria of GANLoss('vanilla' | 'lsgan') -- BCEWithLogitsLoss / MSELoss against a filled label, mean-reduced -- plain
//     or relativistic (the logit minus the mean of the other batch's logits), value and gradients from one entry point;
//   * the dense head of the VGG-style discriminators: x.view(B, -1), Linear(C S S -> H), LeakyReLU, Linear(H -> 1), reading the NHWC
//     features and the NCHW-flattened weight as they are;
//   * the perceptual extractor's input normalisation (x - mean[c]) / std[c] and its backward.
// Everything here is exact fp32 / fp64 arithmetic that does not look at the conv math mode, uses no atomics and sums in a fixed
// order: bit-identical from run to run.  The file is compiled with -ffp-contract=off: every fused multiply-add below is an fmaf.
#include "common.h"

namespace srhip {

constexpr long GAN_MAX_COUNT = 1L << 22;     // one 256-thread block walks the logits: a patch discriminator's B h w, not an image

// sum of the 256 threads' values, combined as a binary tree over the thread index (strides 128, 64, .., 1): a fixed order
__device__ inline double block_tree_sum_f64(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__device__ inline float block_tree_sum_f32(float v, float* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

// BCEWithLogits in the stable form max(x, 0) - x y + log1p(exp(-|x|)).  `x < 0 ? 0 : x` keeps a NaN logit (fmax would drop it), and
// exp(-|x|) <= 1 never overflows: logits of +-100 give finite values.
__device__ __forceinline__ double bce_logits(double x, double y) { return (x < 0.0 ? 0.0 : x) - x * y + log1p(exp(-fabs(x))); }
// its derivative sigmoid(x) - y, each branch with an argument <= 0 of exp; a NaN fails `x >= 0` and comes back out of exp
__device__ __forceinline__ double bce_logits_grad(double x, double y) {
  if (x >= 0.0) return 1.0 / (1.0 + exp(-x)) - y;
  const double e = exp(x);
  return e / (1.0 + e) - y;
}

// One block.  m = relativistic ? mean(b) : 0 (float64, thread t adds b[t], b[t + 256], .. in order, then the tree);
// x_i = a_i - m (float64); out = mean_i f(x_i, label); with gout: da_i = gout f'(x_i) / count and, through the mean,
// db_j = -gout sum_i f'(x_i) / (count count_b).
template <int MODE>
__global__ __launch_bounds__(256) void gan_loss_kernel(const float* __restrict__ a, long count, const float* __restrict__ b, long count_b,
                                                       float label, int relativistic, const float* __restrict__ gout,
                                                       float* __restrict__ out, float* __restrict__ da, float* __restrict__ db) {
  __shared__ double red[256];
  double m = 0.0;
  if (relativistic) {
    double s = 0.0;
    for (long i = threadIdx.x; i < count_b; i += 256) s += (double)b[i];
    m = block_tree_sum_f64(s, red) / (double)count_b;
  }
  const double y = (double)label;
  const double g0 = gout ? (double)gout[0] / (double)count : 0.0;
  double ls = 0.0, gs = 0.0;
  for (long i = threadIdx.x; i < count; i += 256) {
    const double x = (double)a[i] - m;
    if (out) ls += MODE == SRHIP_GAN_VANILLA ? bce_logits(x, y) : (x - y) * (x - y);
    if (gout) {
      const double d = MODE == SRHIP_GAN_VANILLA ? bce_logits_grad(x, y) : 2.0 * (x - y);
      if (da) da[i] = (float)(g0 * d);
      gs += d;
    }
  }
  if (out) {
    ls = block_tree_sum_f64(ls, red);
    if (threadIdx.x == 0) out[0] = (float)(ls / (double)count);
  }
  if (db) {
    gs = block_tree_sum_f64(gs, red);
    const float v = (float)(-(g0 * gs) / (double)count_b);
    for (long j = threadIdx.x; j < count_b; j += 256) db[j] = v;
  }
}

// ---- the discriminators' dense head ------------------------------------------------------------------------------------------ //
// x: [B, S, S, C] (NHWC), w0: [H, K], K = C S S, flattened as the reference's NCHW view does: k = c S S + p, p = row S + column.
// Element k of a weight row meets x[b, p, c] = xb[p C + c]: the flatten order lives in this index, nothing is transposed.

// hidden[b, j] = lrelu(b0[j] + sum_k w0[j, k] x[b, k]).  Block (j, b).  Order: thread t owns the float4 groups g = t, t + 256, .. of the
// weight row (k = 4 g .. 4 g + 3) and runs ONE fmaf chain over them in ascending k; the 256 chains are added as a binary tree over t
// (strides 128 .. 1); the bias is added last.
__global__ __launch_bounds__(256) void dhead_hidden_kernel(const float* __restrict__ x, const float* __restrict__ w0,
                                                           const float* __restrict__ b0, float* __restrict__ hidden, int C, int S2,
                                                           int K, int H, float slope) {
  __shared__ float red[256];
  const int j = blockIdx.x, b = blockIdx.y;
  const float* __restrict__ wr = w0 + (long)j * K;
  const float* __restrict__ xb = x + (long)b * K;
  float acc = 0.f;
  for (int k = threadIdx.x * 4; k < K; k += 1024) {
    const float4 wv = *reinterpret_cast<const float4*>(wr + k);
    const float wk[4] = {wv.x, wv.y, wv.z, wv.w};
    int c = k / S2, p = k - c * S2;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      acc = fmaf(wk[l], xb[p * C + c], acc);
      if (++p == S2) {
        p = 0;
        ++c;
      }
    }
  }
  acc = block_tree_sum_f32(acc, red);
  if (threadIdx.x == 0) {
    const float z = acc + b0[j];
    hidden[(long)b * H + j] = z > 0.f ? z : z * slope;          // a NaN fails the comparison and stays a NaN
  }
}

// y[b] = b1 + sum_j w1[j] hidden[b, j].  Block b; thread t chains j = t, t + 256, .. ascending, then the tree, then the bias.
__global__ __launch_bounds__(256) void dhead_out_kernel(const float* __restrict__ hidden, const float* __restrict__ w1,
                                                        const float* __restrict__ b1, float* __restrict__ y, int H) {
  __shared__ float red[256];
  const int b = blockIdx.x;
  float acc = 0.f;
  for (int j = threadIdx.x; j < H; j += 256) acc = fmaf(w1[j], hidden[(long)b * H + j], acc);
  acc = block_tree_sum_f32(acc, red);
  if (threadIdx.x == 0) y[b] = acc + b1[0];
}

// dz[b, j] = dy[b] w1[j] * (hidden[b, j] > 0 ? 1 : slope): the gradient at the first linear's output, the LeakyReLU mask taken from
// the stored activation (slope > 0: hidden > 0 exactly where the pre-activation was)
__global__ __launch_bounds__(256) void dhead_dz_kernel(const float* __restrict__ dy, const float* __restrict__ hidden,
                                                       const float* __restrict__ w1, float* __restrict__ dz, int B, int H, float slope) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * H) return;
  const int b = i / H, j = i - b * H;
  const float g = dy[b] * w1[j];
  dz[i] = hidden[i] > 0.f ? g : g * slope;
}

// thread j < H: dw1[j] = sum_b dy[b] hidden[b, j], db0[j] = sum_b dz[b, j]; thread H: db1 = sum_b dy[b].  Chains over ascending b.
__global__ __launch_bounds__(256) void dhead_small_grads_kernel(const float* __restrict__ dy, const float* __restrict__ hidden,
                                                                const float* __restrict__ dz, float* __restrict__ db0,
                                                                float* __restrict__ dw1, float* __restrict__ db1, int B, int H) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < H) {
    float sw = 0.f, sb = 0.f;
    for (int b = 0; b < B; ++b) {
      sw = fmaf(dy[b], hidden[(long)b * H + j], sw);
      sb += dz[(long)b * H + j];
    }
    dw1[j] = sw;
    db0[j] = sb;
  } else if (j == H) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += dy[b];
    db1[0] = s;
  }
}

// dw0[j, k .. k + 3] = sum_b dz[b, j] x[b, k ..]: one thread per float4 of the weight gradient, one fmaf chain per element over
// ascending b
__global__ __launch_bounds__(256) void dhead_dw0_kernel(const float* __restrict__ dz, const float* __restrict__ x, float* __restrict__ dw0,
                                                        int B, int C, int S2, int K, int H) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const int k4 = K >> 2;
  if (idx >= (long)H * k4) return;
  const int j = (int)(idx / k4), k = (int)(idx - (long)j * k4) * 4;
  int off[4];
  int c = k / S2, p = k - c * S2;
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    off[l] = p * C + c;
    if (++p == S2) {
      p = 0;
      ++c;
    }
  }
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int b = 0; b < B; ++b) {
    const float z = dz[(long)b * H + j];
    const float* __restrict__ xb = x + (long)b * K;
#pragma unroll
    for (int l = 0; l < 4; ++l) acc[l] = fmaf(z, xb[off[l]], acc[l]);
  }
  *reinterpret_cast<float4*>(dw0 + (long)j * K + k) = make_float4(acc[0], acc[1], acc[2], acc[3]);
}

// dx[b, p, c] = sum_j dz[b, j] w0[j, c S2 + p]: one thread per element of the NHWC gradient, one fmaf chain over ascending j
__global__ __launch_bounds__(256) void dhead_dx_kernel(const float* __restrict__ dz, const float* __restrict__ w0, float* __restrict__ dx,
                                                       int B, int C, int S2, int K, int H) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)B * K) return;
  const int b = (int)(idx / K), r = (int)(idx - (long)b * K);
  const int p = r / C, c = r - p * C;
  const float* __restrict__ wk = w0 + (c * S2 + p);
  float acc = 0.f;
  for (int j = 0; j < H; ++j) acc = fmaf(dz[(long)b * H + j], wk[(long)j * K], acc);
  dx[idx] = acc;
}

// ---- input normalisation of the perceptual extractor ------------------------------------------------------------------------- //
// NHWC, element e belongs to channel e % C.  BWD = false: y = (x - mean[c]) / std[c]; BWD = true: y = x / std[c] (x the gradient).
// IEEE subtraction and division, as torch evaluates (x - mean) / std.
template <bool BWD>
__global__ __launch_bounds__(256) void input_norm_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                         const float* __restrict__ stdv, float* __restrict__ y, long count, int C) {
  float mu[4], sd[4];
  for (int c = 0; c < 4; ++c) {
    mu[c] = (!BWD && c < C) ? mean[c] : 0.f;
    sd[c] = c < C ? stdv[c] : 1.f;
  }
  const long n4 = count >> 2;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    const float in[4] = {v.x, v.y, v.z, v.w};
    float o[4];
    int c = (int)((i * 4) % C);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      o[l] = (in[l] - mu[c]) / sd[c];
      if (++c == C) c = 0;
    }
    reinterpret_cast<float4*>(y)[i] = make_float4(o[0], o[1], o[2], o[3]);
  }
  if (blockIdx.x == 0)
    for (long e = (n4 << 2) + threadIdx.x; e < count; e += 256) {
      const int c = (int)(e % C);
      y[e] = (x[e] - mu[c]) / sd[c];
    }
}

}  // namespace srhip

using namespace srhip;

extern "C" {

int srhip_gan_loss_fwd_bwd(const float* a, long count, const float* b, long count_b, int mode, float label, int relativistic,
                           const float* gout, float* out, float* da, float* db, void* stream) {
  SRHIP_REQUIRE(a != nullptr && count >= 1 && count <= GAN_MAX_COUNT, "gan_loss: needs 1 <= count <= %ld logits, got %ld", GAN_MAX_COUNT,
                count);
  SRHIP_REQUIRE(mode == SRHIP_GAN_VANILLA || mode == SRHIP_GAN_LS, "gan_loss: unknown mode %d (0 vanilla, 1 LS)", mode);
  SRHIP_REQUIRE(!relativistic || (b != nullptr && count_b >= 1 && count_b <= GAN_MAX_COUNT),
                "gan_loss: the relativistic form needs b with 1 <= count_b <= %ld, got %ld", GAN_MAX_COUNT, count_b);
  SRHIP_REQUIRE(db == nullptr || relativistic, "gan_loss: db is the gradient through mean(b): relativistic form only");
  SRHIP_REQUIRE((da == nullptr && db == nullptr) || gout != nullptr, "gan_loss: gradients need gout");
  SRHIP_REQUIRE(out != nullptr || gout != nullptr, "gan_loss: nothing to compute (out and gout are both null)");
  if (mode == SRHIP_GAN_VANILLA)
    hipLaunchKernelGGL(gan_loss_kernel<SRHIP_GAN_VANILLA>, dim3(1), dim3(256), 0, as_stream(stream), a, count, b, count_b, label,
                       relativistic, gout, out, da, db);
  else
    hipLaunchKernelGGL(gan_loss_kernel<SRHIP_GAN_LS>, dim3(1), dim3(256), 0, as_stream(stream), a, count, b, count_b, label, relativistic,
                       gout, out, da, db);
  return check_launch("gan_loss_fwd_bwd");
}

static int dhead_dims_ok(const char* what, int B, int C, int S, int H) {
  if (B < 1 || B > 65535 || C < 4 || C % 4 || S < 1 || H < 1 || (long)C * S * S > (1L << 24)) {
    set_error("%s: needs 1 <= B <= 65535, C %% 4 == 0, S >= 1, H >= 1, C S S <= 2^24, got B %d C %d S %d H %d", what, B, C, S, H);
    return 0;
  }
  return 1;
}

int srhip_dhead_fwd(const float* x, const float* w0, const float* b0, const float* w1, const float* b1, float* hidden, float* y, int B,
                    int C, int S, int H, float slope, void* stream) {
  if (!dhead_dims_ok("dhead_fwd", B, C, S, H)) return SRHIP_ERR_ARG;
  SRHIP_REQUIRE(x && w0 && b0 && w1 && b1 && hidden && y, "dhead_fwd: null tensor");
  SRHIP_REQUIRE(((uintptr_t)w0 & 15) == 0, "dhead_fwd: the weight must be 16-byte aligned");
  SRHIP_REQUIRE(slope > 0.f, "dhead_fwd: the backward reads the mask from the activation: slope > 0");
  const int K = C * S * S;
  hipLaunchKernelGGL(dhead_hidden_kernel, dim3(H, B), dim3(256), 0, as_stream(stream), x, w0, b0, hidden, C, S * S, K, H, slope);
  hipLaunchKernelGGL(dhead_out_kernel, dim3(B), dim3(256), 0, as_stream(stream), hidden, w1, b1, y, H);
  return check_launch("dhead_fwd");
}

int srhip_dhead_bwd(const float* dy, const float* x, const float* hidden, const float* w0, const float* w1, float* dz, float* dx,
                    float* dw0, float* db0, float* dw1, float* db1, int B, int C, int S, int H, float slope, void* stream) {
  if (!dhead_dims_ok("dhead_bwd", B, C, S, H)) return SRHIP_ERR_ARG;
  SRHIP_REQUIRE(dy && x && hidden && w0 && w1 && dz, "dhead_bwd: null tensor");
  const bool params = dw0 != nullptr;
  SRHIP_REQUIRE(params == (db0 != nullptr) && params == (dw1 != nullptr) && params == (db1 != nullptr),
                "dhead_bwd: the four parameter gradients come together or not at all");
  SRHIP_REQUIRE(params || dx, "dhead_bwd: nothing to compute");
  SRHIP_REQUIRE(((uintptr_t)dw0 & 15) == 0, "dhead_bwd: the weight gradient must be 16-byte aligned");
  const int K = C * S * S;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(dhead_dz_kernel, dim3(cdiv((long)B * H, 256)), dim3(256), 0, st, dy, hidden, w1, dz, B, H, slope);
  if (params) {
    hipLaunchKernelGGL(dhead_small_grads_kernel, dim3(cdiv(H + 1, 256)), dim3(256), 0, st, dy, hidden, dz, db0, dw1, db1, B, H);
    hipLaunchKernelGGL(dhead_dw0_kernel, dim3(cdiv((long)H * (K / 4), 256)), dim3(256), 0, st, dz, x, dw0, B, C, S * S, K, H);
  }
  if (dx) hipLaunchKernelGGL(dhead_dx_kernel, dim3(cdiv((long)B * K, 256)), dim3(256), 0, st, dz, w0, dx, B, C, S * S, K, H);
  return check_launch("dhead_bwd");
}

static int input_norm_launch(const char* what, bool bwd, const float* x, const float* mean, const float* stdv, float* y, long count,
                             int c, void* stream) {
  if (!x || !y || !stdv || (!bwd && !mean) || count < 1 || c < 1 || c > 4 || count % c) {
    set_error("%s: needs tensors, 1 <= C <= 4 (image channels) and count a multiple of C, got count %ld, C %d", what, count, c);
    return SRHIP_ERR_ARG;
  }
  if ((((uintptr_t)x | (uintptr_t)y) & 15) != 0) {
    set_error("%s: input and output must be 16-byte aligned", what);
    return SRHIP_ERR_ARG;
  }
  long nb = (count / 4 + 255) / 256;
  nb = nb < 1 ? 1 : (nb > 4096 ? 4096 : nb);
  if (bwd)
    hipLaunchKernelGGL(input_norm_kernel<true>, dim3((int)nb), dim3(256), 0, as_stream(stream), x, mean, stdv, y, count, c);
  else
    hipLaunchKernelGGL(input_norm_kernel<false>, dim3((int)nb), dim3(256), 0, as_stream(stream), x, mean, stdv, y, count, c);
  return check_launch(what);
}

int srhip_input_norm_fwd(const float* x, const float* mean, const float* stdv, float* y, long count, int c, void* stream) {
  return input_norm_launch("input_norm_fwd", false, x, mean, stdv, y, count, c, stream);
}

int srhip_input_norm_bwd(const float* dy, const float* stdv, float* dx, long count, int c, void* stream) {
  return input_norm_launch("input_norm_bwd", true, dy, nullptr, stdv, dx, count, c, stream);
}

}  // extern "C"
