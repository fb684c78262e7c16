// Spectral normalisation of the patch discriminator's conv weights (reference base_networks.py:73-131), batched over the layers of one
// discriminator pass.  Per layer, Wb = weight_bar viewed as [cout][k] (k = cin kh kw, OIHW order), one power iteration per forward:
//   t = Wb^T u,  v <- t / (|t| + 1e-12);   s = Wb v,  u <- s / (|s| + 1e-12);   sigma = <u, s>;   W = Wb / sigma
// u and v are updated IN PLACE (they are parameters of the module) and a snapshot of (u, v, sigma) of THIS pass is left in the pass
// buffer for the pass's backward, which projects a gradient G with respect to W onto weight_bar:
//   Gb += G / sigma - (<G, Wb> / sigma^2) u v^T
//
// One device table of SnEntry serves every pass: it holds the parameters' addresses and, for everything a pass writes, OFFSETS into a
// buffer the caller allocates per pass (sigma, W, the snapshots, scratch) -- the table never changes, so no pass copies a table to the
// device.  The per-call addresses of the backward (the gradients autograd hands over, the slots they are accumulated into) travel as
// kernel arguments (SnGradPtrs, at most SN_MAXL layers per launch).
//
// Launches per call, whatever the number of layers (blockIdx.y = layer): forward 4 (column partials per slab of SN_SLAB rows | t, |t|,
// v | rows | |s|, u, sigma recomputed by every block + the scaling of its chunk), backward 2 (partial dots per chunk of SN_CHUNK elements |
// the dot + the projection of a chunk).  Every reduction is two-stage in a fixed order without atomics, and the work items of a layer
// (slabs, column chunks, row quads, element chunks) are functions of (cout, k) alone: blocks walk them with a grid stride, so a layer's
// results depend neither on the other layers of the table nor on the grid.  fp32 operands, sums carried in fp64 and rounded once,
// divisions in fp32 as the reference writes them; nothing here looks at the conv arithmetic mode.  Any cout >= 1, k >= 1: no vector
// width is assumed (k = 27 in the first layer).
#include "common.h"

namespace srhip {

constexpr int SN_SLAB = 32;       // rows of a column-partial slab
constexpr int SN_COLS = 256;      // columns of a column-partial block
constexpr int SN_CHUNK = 4096;    // elements of an element-wise chunk (16 per thread)
constexpr int SN_T = 256;
constexpr int SN_TV = 1024;       // threads of the per-layer block that finishes v
constexpr int SN_MAXL = 32;       // layers per backward launch (addresses in the kernel arguments)
constexpr int SN_MAXGRID = 4096;

struct SnEntry {
  const float* wbar;
  float* u;
  float* v;
  long off_sigma, off_weff, off_u, off_v;   // floats from the pass buffer: sigma [1], W [cout k], snapshots of u [cout] and v [k]
  long off_tpart, off_s;                    // scratch in the pass buffer: column partials (DOUBLES, srhip_sn_tpart_elems floats; even offset), s [cout]
  long off_dpart;                           // doubles from the backward's workspace: srhip_sn_dot_parts partial dots
  int cout, k;
};

struct SnGradPtrs {
  const float* g[SN_MAXL];
  float* gbar[SN_MAXL];
};

static inline int sn_slabs(int cout) { return (cout + SN_SLAB - 1) / SN_SLAB; }
static inline long sn_chunks(long cout, long k) { return (cout * k + SN_CHUNK - 1) / SN_CHUNK; }

// block-wide sum in a fixed tree; every thread gets the result; `red` is free again on return
template <int T>
__device__ inline double sn_block_sum(double* red, double v) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int o = T / 2; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// ---- forward 1: tpart[slab][k] = sum over the slab's rows of Wb[r][k] u[r]
__global__ __launch_bounds__(SN_T) void sn_colpart(const SnEntry* __restrict__ ents, float* __restrict__ out) {
  const SnEntry e = ents[blockIdx.y];
  const int slabs = (e.cout + SN_SLAB - 1) / SN_SLAB, cchunks = (e.k + SN_COLS - 1) / SN_COLS;
  const long items = (long)slabs * cchunks;
  double* tpart = reinterpret_cast<double*>(out + e.off_tpart);
  for (long it = blockIdx.x; it < items; it += gridDim.x) {
    const int slab = (int)(it / cchunks), cc = (int)(it % cchunks);
    const int k = cc * SN_COLS + threadIdx.x;
    if (k >= e.k) continue;
    const int r0 = slab * SN_SLAB, r1 = r0 + SN_SLAB < e.cout ? r0 + SN_SLAB : e.cout;
    double a = 0.0;
    for (int r = r0; r < r1; ++r) a += (double)e.wbar[(size_t)r * e.k + k] * (double)e.u[r];
    tpart[(size_t)slab * e.k + k] = a;
  }
}

// ---- forward 2 (one block per layer): t[k] = the slabs in order, |t|, v = t / (|t| + eps) -> the parameter and the snapshot
__global__ __launch_bounds__(SN_TV) void sn_finish_v(const SnEntry* __restrict__ ents, float* __restrict__ out) {
  __shared__ double red[SN_TV];
  const SnEntry e = ents[blockIdx.x];
  const int slabs = (e.cout + SN_SLAB - 1) / SN_SLAB;
  const double* tpart = reinterpret_cast<const double*>(out + e.off_tpart);
  float* vs = out + e.off_v;
  double ss = 0.0;
  for (int k = threadIdx.x; k < e.k; k += SN_TV) {
    double t = 0.0;
    for (int s = 0; s < slabs; ++s) t += tpart[(size_t)s * e.k + k];
    const float tf = (float)t;
    vs[k] = tf;                                     // (read back below by the thread that wrote it)
    ss += (double)tf * (double)tf;
  }
  const float den = (float)sqrt(sn_block_sum<SN_TV>(red, ss)) + 1e-12f;
  for (int k = threadIdx.x; k < e.k; k += SN_TV) {
    const float val = vs[k] / den;
    vs[k] = val;
    e.v[k] = val;
  }
}

// ---- forward 3: s[r] = <Wb[r], v>, one wave per row: 64 strided lane sums, then the butterfly
__global__ __launch_bounds__(SN_T) void sn_rows(const SnEntry* __restrict__ ents, float* __restrict__ out) {
  const SnEntry e = ents[blockIdx.y];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float* vs = out + e.off_v;
  float* s = out + e.off_s;
  const int quads = (e.cout + 3) / 4;
  for (int q = blockIdx.x; q < quads; q += gridDim.x) {
    const int r = q * 4 + wv;
    if (r >= e.cout) continue;                      // (wave-uniform)
    const float* row = e.wbar + (size_t)r * e.k;
    double a = 0.0;
    for (int k = lane; k < e.k; k += 64) a += (double)row[k] * (double)vs[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if (lane == 0) s[r] = (float)a;
  }
}

// ---- forward 4: every block recomputes |s|, u and sigma = <u, s> in the same order (cout values); block 0 of a layer stores u
// (parameter + snapshot) and sigma; then W = Wb / sigma over the layer's chunks
__global__ __launch_bounds__(SN_T) void sn_scale(const SnEntry* __restrict__ ents, float* __restrict__ out) {
  __shared__ double red[SN_T];
  const SnEntry e = ents[blockIdx.y];
  const long total = (long)e.cout * e.k, chunks = (total + SN_CHUNK - 1) / SN_CHUNK;
  if ((long)blockIdx.x >= chunks) return;           // (the whole block)
  const int tid = threadIdx.x;
  const float* s = out + e.off_s;
  double ss = 0.0;
  for (int i = tid; i < e.cout; i += SN_T) ss += (double)s[i] * (double)s[i];
  const float den = (float)sqrt(sn_block_sum<SN_T>(red, ss)) + 1e-12f;
  double sg = 0.0;
  for (int i = tid; i < e.cout; i += SN_T) sg += (double)(s[i] / den) * (double)s[i];
  const float sigma = (float)sn_block_sum<SN_T>(red, sg);
  if (blockIdx.x == 0) {
    float* us = out + e.off_u;
    for (int i = tid; i < e.cout; i += SN_T) {
      const float ui = s[i] / den;
      us[i] = ui;
      e.u[i] = ui;
    }
    if (tid == 0) out[e.off_sigma] = sigma;
  }
  float* weff = out + e.off_weff;
  for (long c = blockIdx.x; c < chunks; c += gridDim.x)
#pragma unroll 4
    for (int j = 0; j < SN_CHUNK / SN_T; ++j) {
      const long idx = c * SN_CHUNK + (long)j * SN_T + tid;
      if (idx < total) weff[idx] = e.wbar[idx] / sigma;
    }
}

// ---- backward 1: dpart[chunk] = sum over the chunk of G Wb
__global__ __launch_bounds__(SN_T) void sn_dot_part(const SnEntry* __restrict__ ents, SnGradPtrs p, double* __restrict__ ws) {
  __shared__ double red[SN_T];
  const float* g = p.g[blockIdx.y];
  if (!g) return;
  const SnEntry e = ents[blockIdx.y];
  const long total = (long)e.cout * e.k, chunks = (total + SN_CHUNK - 1) / SN_CHUNK;
  double* dpart = ws + e.off_dpart;
  for (long c = blockIdx.x; c < chunks; c += gridDim.x) {   // (block-uniform trip count: the barriers inside are safe)
    double a = 0.0;
    for (int j = 0; j < SN_CHUNK / SN_T; ++j) {
      const long idx = c * SN_CHUNK + (long)j * SN_T + threadIdx.x;
      if (idx < total) a += (double)g[idx] * (double)e.wbar[idx];
    }
    const double tot = sn_block_sum<SN_T>(red, a);
    if (threadIdx.x == 0) dpart[c] = tot;
  }
}

// ---- backward 2: <G, Wb> = the partial dots in order (every block, the same order), Gb += G / sigma - (dot / sigma^2) u v^T
__global__ __launch_bounds__(SN_T) void sn_project(const SnEntry* __restrict__ ents, SnGradPtrs p, const float* __restrict__ out,
                                                  const double* __restrict__ ws) {
  __shared__ double red[SN_T];
  const float* g = p.g[blockIdx.y];
  if (!g) return;
  float* gbar = p.gbar[blockIdx.y];
  const SnEntry e = ents[blockIdx.y];
  const long total = (long)e.cout * e.k, chunks = (total + SN_CHUNK - 1) / SN_CHUNK;
  if ((long)blockIdx.x >= chunks) return;
  const double* dpart = ws + e.off_dpart;
  double a = 0.0;
  for (long c = threadIdx.x; c < chunks; c += SN_T) a += dpart[c];
  const float dot = (float)sn_block_sum<SN_T>(red, a);
  const float sigma = out[e.off_sigma];
  const float coef = dot / (sigma * sigma);
  const float* us = out + e.off_u;
  const float* vs = out + e.off_v;
  for (long c = blockIdx.x; c < chunks; c += gridDim.x)
#pragma unroll 4
    for (int j = 0; j < SN_CHUNK / SN_T; ++j) {
      const long idx = c * SN_CHUNK + (long)j * SN_T + threadIdx.x;
      if (idx < total) {
        const long r = idx / e.k;
        const int kk = (int)(idx - r * e.k);
        gbar[idx] += g[idx] / sigma - coef * us[r] * vs[kk];
      }
    }
}

static int sn_grid(long items) { return (int)(items < 1 ? 1 : (items > SN_MAXGRID ? SN_MAXGRID : items)); }

}  // namespace srhip

using namespace srhip;

int srhip_sn_entry_bytes(void) { return (int)sizeof(SnEntry); }

long srhip_sn_tpart_elems(int cout, int k) {
  if (cout < 1 || k < 1) return 0;
  return 2L * sn_slabs(cout) * k;
}

long srhip_sn_dot_parts(int cout, int k) {
  if (cout < 1 || k < 1) return 0;
  return sn_chunks(cout, k);
}

int srhip_sn_forward_batched(const void* entries_dev, int count, float* out, int max_cout, int max_k, void* stream) {
  SRHIP_REQUIRE(entries_dev && out && count >= 0 && count <= 65535 && max_cout >= 1 && max_k >= 1, "sn_forward_batched: bad argument");
  SRHIP_REQUIRE((reinterpret_cast<size_t>(out) & 7) == 0, "sn_forward_batched: the pass buffer must be 8-byte aligned");
  if (count == 0) return SRHIP_OK;
  const SnEntry* ents = static_cast<const SnEntry*>(entries_dev);
  hipStream_t st = as_stream(stream);
  const long cols = (long)sn_slabs(max_cout) * ((max_k + SN_COLS - 1) / SN_COLS);
  hipLaunchKernelGGL(sn_colpart, dim3(sn_grid(cols), count), dim3(SN_T), 0, st, ents, out);
  hipLaunchKernelGGL(sn_finish_v, dim3(count), dim3(SN_TV), 0, st, ents, out);
  hipLaunchKernelGGL(sn_rows, dim3(sn_grid((max_cout + 3) / 4), count), dim3(SN_T), 0, st, ents, out);
  hipLaunchKernelGGL(sn_scale, dim3(sn_grid(sn_chunks(max_cout, max_k)), count), dim3(SN_T), 0, st, ents, out);
  return check_launch("sn_forward_batched");
}

int srhip_sn_backward_batched(const void* entries_dev, int count, const float* out, const void* const* grads, void* const* gbars,
                              void* workspace, int max_cout, int max_k, void* stream) {
  SRHIP_REQUIRE(entries_dev && out && grads && gbars && workspace && count >= 0 && max_cout >= 1 && max_k >= 1,
                "sn_backward_batched: bad argument");
  SRHIP_REQUIRE((reinterpret_cast<size_t>(workspace) & 7) == 0, "sn_backward_batched: the workspace must be 8-byte aligned");
  for (int i = 0; i < count; ++i) SRHIP_REQUIRE(!grads[i] || gbars[i], "sn_backward_batched: layer %d has a gradient but no slot", i);
  const SnEntry* ents = static_cast<const SnEntry*>(entries_dev);
  hipStream_t st = as_stream(stream);
  const int gx = sn_grid(sn_chunks(max_cout, max_k));
  for (int first = 0; first < count; first += SN_MAXL) {      // (more than SN_MAXL layers: one pair of launches per SN_MAXL)
    const int n = count - first < SN_MAXL ? count - first : SN_MAXL;
    SnGradPtrs p;
    bool any = false;
    for (int i = 0; i < SN_MAXL; ++i) {
      p.g[i] = i < n ? static_cast<const float*>(grads[first + i]) : nullptr;
      p.gbar[i] = i < n ? static_cast<float*>(gbars[first + i]) : nullptr;
      any = any || p.g[i];
    }
    if (!any) continue;
    hipLaunchKernelGGL(sn_dot_part, dim3(gx, n), dim3(SN_T), 0, st, ents + first, p, static_cast<double*>(workspace));
    hipLaunchKernelGGL(sn_project, dim3(gx, n), dim3(SN_T), 0, st, ents + first, p, out, static_cast<const double*>(workspace));
  }
  return check_launch("sn_backward_batched");
}
