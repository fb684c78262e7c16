/* sradsgan_hip.h -- C ABI of libsradsgan_hip.so (MI355X / gfx950 only).
 *
 * The reference (Meng-333/SRADSGAN) is pure Python on stock PyTorch: it has no FFI layer of its
 * own.  Every entry point below therefore replaces an ATen/cuDNN call that the reference makes
 * implicitly through torch.nn in SRADSGAN/model/sradsgan.py (cited per function as file:line).
 *
 * Conventions
 *   - all tensors are fp32, device memory, caller-allocated; activations are NHWC
 *     ("channels_last": element (n,h,w,c) at ((n*H+h)*W+w)*ld + c, ld >= C);
 *     parameters and parameter gradients keep the framework layout (OIHW) so state_dicts stay
 *     interchangeable with the reference's `.pkl` files;
 *   - `stream` is a hipStream_t passed as void*; calls are asynchronous on that stream and
 *     re-entrant across streams; nothing allocates, frees or synchronises;
 *   - return value 0 = success; otherwise a negative code and srhip_last_error() (thread local)
 *     describes it.  No exceptions cross the boundary.
 */
#ifndef SRADSGAN_HIP_H
#define SRADSGAN_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRHIP_OK 0
#define SRHIP_ERR_ARG (-1)
#define SRHIP_ERR_LAUNCH (-2)
#define SRHIP_ERR_WORKSPACE (-3)

/* epilogue flags of srhip_conv2d_fwd */
#define SRHIP_EPI_BIAS 1      /* y += bias[co]                                             */
#define SRHIP_EPI_LRELU 2     /* y = y > 0 ? y : slope*y   (slope 0 => ReLU)               */
#define SRHIP_EPI_RESIDUAL 4  /* y += residual (after the activation): `out += x`          */
#define SRHIP_EPI_ROWSCALE 8  /* y = rowscale[pixel] * (W.x) (+bias...) : SLAM mask folded */
#define SRHIP_EPI_ACTMASK 32  /* (dgrad) y = actmask > 0 ? y : slope*y : backward of the producer's LeakyReLU */
#define SRHIP_EPI_CHANSCALE 16 /* x[n,h,w,c] is read as x*chanscale[n][c] : CLAM scale folded (Cin%16==0) */
#define SRHIP_EPI_GRADDATA 64 /* (fwd) x holds gradients (second-order passes): SRHIP_MATH_HALF then multiplies in bf16, not fp16 */

const char* srhip_last_error(void);
int srhip_abi_version(void);
/* `to_stream` waits for everything enqueued on `from_stream` so far (event record + stream wait, events from an internal
 * ring shared by all callers: slot counter atomic, ONE device per process; legal under stream capture: it forks `to_stream` into
 * the capture).  Host-side helper, no kernel.  */
int srhip_stream_fork(void* from_stream, void* to_stream);
/* ABI 2: fast packed weights carry a second, pre-split bf16 section (srhip_packed_elems doubled for them);
 * srhip_set_conv_math / srhip_get_conv_math added.
 * ABI 3: srhip_cgam_*, srhip_sgam_flash_*, loss reductions (srhip_l1_mean_*, srhip_mean_*, srhip_gp_norm_penalty_*),
 * srhip_dp_* (RCCL gradient exchange), srhip_cbam_* / srhip_sigmoid_* (discriminator attention primitives) added;
 *        fast packed weights carry a third (fp16) section, SRHIP_MATH_HALF.
 * ABI 4: srhip_conv2d_wgrad_act / srhip_conv2d_wgrad_act_ok added (no existing entry point changed).
 * ABI 5: srhip_bn_eval_fwd, srhip_attn_tail_bwd (+ _fused_workspace), srhip_stream_fork, srhip_conv2d_wgrad_multi (+ _ok)
 *        added (no existing entry point changed).
 * ABI 6-9: see the notes at the entry points they added.
 * ABI 10: srhip_attn_tail_bwd_g REMOVED (nothing else changed).
 * ABI 11: srhip_cat_channels / srhip_split_channels added.
 * ABI 12: DSSR's average-pool channel attention (srhip_ca_*), the upsampler fold passes (srhip_add_bcast_scaled,
 *         srhip_batch_sum_scaled) and srhip_mse_mean_* added (no existing entry point changed).
 * ABI 13: NDSRGAN's passes (srhip_scaled_res_fwd / _bwd, srhip_lrelu_bwd_strided, srhip_upsample_nearest_fwd / _bwd) and
 *         srhip_smooth_l1_mean_* added (no existing entry point changed).
 * ABI 14: AMSSRN's passes: dilated 3x3 convolutions (srhip_conv2d_*_dil, srhip_conv2d_dil_workspace), PReLU with a
 *         device-resident slope (srhip_prelu_*), quadrant non-local attention (srhip_nl_quad_*) and the gamma residual
 *         (srhip_gamma_*) added (no existing entry point changed).
 *         Later in ABI 14, additive only: the channel attention with biases (srhip_ca_mlp_fwd_bias, srhip_ca_mlp_bwd_bias) for
 *         RCAN; HAT's window-transformer passes (srhip_hat_*: LayerNorm, GELU, window attention, channel attention at any
 *         C <= 128 and the block combine).  The version number stays 14: no existing entry point or layout changed, and the Python binding resolves every
 *         declared symbol by name when it loads the library, so a library without them fails at load time.
 *         The LPIPS metric's passes (srhip_lpips_*, srhip_maxpool3x3s2_fwd) joined the same way: additive, version 14; so did the
 *         backward passes that make it a loss (srhip_lpips_head_bwd, srhip_maxpool3x3s2_bwd, srhip_lpips_stem_bwd), and the passes of
 *         the contrastive VGG19 losses (srhip_contrast_*, srhip_maxpool2x2_floor_*). */
/* Experiment knobs for kernel tuning and for tests that must reach a specific kernel at a small size:
 *   key 0  fprop/dgrad kernel choice: 0 heuristic, -1 force the LDS-DMA kernels, -2 force the patch kernel,
 *          20 / 21 register-staged (exact fp32) kernels only, 23 every launch the patch kernel would take goes to the LDS-DMA kernel,
 *          24 the patch kernel with 64-wide N tiles for every Cout (experiment: twice the blocks, -8 %),
 *          1..8 fixed tile shapes of the register-staged kernel
 *   key 1  wgrad: 0 heuristic, 1/2 N tile 64/128, 5 256-wide tiles, 7 no row-tap kernel, 9 row-tap kernel without paired row tails, >= 10 register-staged
 *          kernel, >= 100 split-K block target of the row-tap kernel
 *   key 3  ablation bits (0x100 / 0x200: timing only, wrong results;
 *          0x400: plain instead of non-temporal epilogue stores, correct results)
 *   key 4  1: the exact-fp32 SGAM kernels in every arithmetic mode (default: split-bf16 products outside SRHIP_MATH_FP32)
 *   key 5  grid of the persistent patch kernel: 0 = three blocks per CU when the conv has more tiles than that (default),
 *          n > 0 = exactly min(n, tiles) blocks whatever the tile count (tests: several tiles per block on small images),
 *          -1 = never (one tile per block: the round-1..3 kernel)
 * The live keys are 0, 1, 3, 4, 5, 7, 10, 11, 12, 14, 17, 18 and 19 (csrc/conv_dev.h names the knob behind each).  Keys 2, 6, 8, 9,
 * 13, 15 and 16 drove rejected experiments whose code is gone: like any unknown key they return SRHIP_ERR_ARG, and their
 * numbers are not reused. */
int srhip_debug_set(int key, int value);

/* ---- in-step kernel timing probe (ABI 6; bench.py: roofline.in_step_avg_launch_ms / in_step_frac) ------------------------------ *
 * No counterpart in the reference (it has no kernels of its own): measurement infrastructure for SURVEY §8(d).
 * srhip_probe_config(kind, n, h, w, cin, cout, max_pairs) arms the probe: every later srhip_conv2d_fwd (kind 1),
 * srhip_conv2d_dgrad (kind 2) or srhip_conv2d_wgrad / srhip_conv2d_wgrad_multi (kind 3) call with exactly this geometry
 * (n, h, w = batch and INPUT image of the convolution) records a HIP event before and after its launches on its own launch
 * stream, for the first max_pairs (<= 1024) such calls; kind 0 disarms.  srhip_probe_read(ms, units, cap) waits for the recorded
 * events and writes the elapsed milliseconds of each call (<= cap) and, when units != NULL, the number of convolutions it
 * processed (nprob of srhip_conv2d_wgrad_multi, else 1), returning the count (-1 on error): the time the kernel took while the
 * step's other streams shared the chip.  Not legal under stream capture; one driving thread.                                  */
int srhip_probe_config(int kind, int n, int h, int w, int cin, int cout, int max_pairs);
int srhip_probe_read(float* ms, int* units, int cap);

/* ---- which kernels the last conv call launched (added within ABI 14; nothing existing changed) -------------------------------- *
 * No counterpart in the reference: test infrastructure.  The route heuristics (csrc/conv_fast_fprop.hip: choose_fprop_route,
 * csrc/conv_wgrad_fast.hip: choose_wgrad_route) decide which kernel a geometry runs, and performance work edits exactly those;
 * a test of a kernel's tile edges must therefore be able to say that its case still reaches that kernel
 * (tests/test_conv_geometry_gpu.py).  srhip_conv2d_last_route(buf, cap) writes one line per kernel launch of the most recent
 * srhip_conv2d_* compute call ON THE CALLING THREAD (the record is thread_local: a step launches from two host threads) into buf
 * (at most cap bytes, always terminated; buf NULL or cap 0: nothing is written) and returns the number of launches; the first 16
 * are kept.  An entry point that calls another (the _dil forms, _dual, _pool, _res3) shows its own launches beside the inner
 * call's.  A line reads
 *     <family> tile=<a>x<b> bn=<n> math=<m> epi=<e> nsplit=<s> cps=<c> phases=<p> grid=<blocks>
 * family  narrow | dot | reg | patch | patch-ks | patch-pers | patch-pers-pp | dma | legacy | headconv (forward / data gradient),
 *         rowtap | wdma | wreg | tail1x1 | wflat | wlegacy | wsmallcin | wnarrow (weight gradient), reduce | reduce-scalar |
 *         wlegacy-reduce | colsum (split-K reduces, bias column sum), dil-gather | dil-scatter
 * tile    BM x BN of the GEMM tile; PH x PW output pixels for the patch family; sub-sums x problems for the reduces; rows x
 *         columns of a sub-image for the dilated passes
 * bn      patch family: destination channels per tile; reg: source channels per K chunk (16 / 32); wdma / wreg: pixels per K
 *         chunk; rowtap: the paired-tail remainder (0: no paired tails); narrow / wnarrow: destination channels compiled for;
 *         dil-*: the dilation
 * math    0 fp32 products, 1 split-bf16, 2 one bf16 product, 3 one fp16 product
 * epi     the SRHIP_EPI_* set compiled into the kernel, -1: flags read at run time; 0 where a kernel has no epilogue
 * nsplit, cps   weight gradients: split-K splits per problem and chunks per split as the kernel walks them
 * phases  dma: phases of a strided data gradient batched into this launch (0: a plain launch); rowtap / wflat: problems of a
 *         grouped launch (0: one)
 * The record is plain integers stored beside each launch; the text is formatted in this call.  Nothing in the library reads it,
 * and it has no effect on routing. */
int srhip_conv2d_last_route(char* buf, int cap);

/* ---- arithmetic of the conv fprop/dgrad contraction ------------------------------------------ *
 * Replaces the implicit choice torch makes for nn.Conv2d (torch.backends.cudnn.allow_tf32, which the
 * reference leaves at its default).  Inputs, outputs and accumulation are fp32 in both modes.
 *   SRHIP_MATH_FP32    every product on v_mfma_f32_32x32x2_f32 (an exact fmaf chain)
 *   SRHIP_MATH_BF16X3  split-bf16: a*b ~= ah*bh + ah*bl + al*bh on v_mfma_f32_32x32x16_bf16, with
 *                      ah = bf16(a), al = bf16(a - ah); per-product error <= ~2^-16, measured max error
 *                      of a 3x3x256 conv vs fp64: 4.5e-6 of max|y| (fp32 chain: 2e-6, TF32: ~5e-4)
 * Process-wide.  Applies to every conv with source channels % 16 == 0 that is large enough for the LDS-DMA / patch /
 * row-tap kernels and to the narrow-N (Cdst <= 32) kernel; the generic small-channel kernels and very small grids
 * always compute in fp32.                                                                        */
#define SRHIP_MATH_FP32 0
#define SRHIP_MATH_BF16X3 1
/*   SRHIP_MATH_HALF    one 16-bit product per multiply, fp32 accumulate, fp32 tensors (BASELINE configs[4]: "fp16 MFMA"):
 *                      forward convolutions of activations round both operands to fp16 (v_mfma_f32_32x32x16_f16, ~2^-11
 *                      per operand); everything that multiplies GRADIENTS (dgrad, wgrad, forward calls flagged
 *                      SRHIP_EPI_GRADDATA) rounds to bf16 instead (v_mfma_f32_32x32x16_bf16): gradients of a mean-reduced
 *                      loss sit far below fp16's range and bf16 needs no loss scaling.  Does NOT meet the 1e-3 parity
 *                      contract of configs[1..3]; judged on PSNR (<= 0.05 dB) and loss drift instead.       */
#define SRHIP_MATH_HALF 2
int srhip_set_conv_math(int mode);
int srhip_get_conv_math(void);

/* ---- weight packing ------------------------------------------------------------------------ *
 * OIHW parameter -> the GEMM "B" operand the conv kernels read.  mode 0 = fprop operand,
 * mode 1 = dgrad operand.  The internal layout depends only on (cout,cin,kh,kw,mode); the buffer
 * must hold srhip_packed_elems() floats (for Cin % 16 == 0 shapes: an fp32 copy, a pre-split
 * bf16 hi/lo copy for SRHIP_MATH_BF16X3 and an fp16 copy for SRHIP_MATH_HALF).  Runs once per optimiser step per conv. */
size_t srhip_packed_elems(int cout, int cin, int kh, int kw, int mode);
int srhip_pack_weight(const float* w_oihw, float* packed, int cout, int cin, int kh, int kw, int mode,
                      void* stream);
/* Batched form: one launch re-packs `count` weights.  entries_dev: device array of
 * struct { const float* w; float* packed; int cout, cin, kh, kw, mode, fast; } (srhip_pack_entry_bytes()
 * bytes each; fast = srhip_packed_is_fast(cout, cin, kh, kw, mode)).                                */
int srhip_pack_entry_bytes(void);
int srhip_packed_is_fast(int cout, int cin, int kh, int kw, int mode);
int srhip_pack_weights_batched(const void* entries_dev, int count, void* stream);

/* ---- nn.Conv2d forward (sradsgan.py:222-223,233,297,332-336,375,381,384,427,448,476,503;
 *      vgg19.features convs :92-95) with the elementwise tail of its call site fused:
 *      bias, LeakyReLU (:242,:337,:383,:428,:479) and the residual add (:274,:323).
 * x: [N,H,W,ldx>=Cin]  packed: srhip_pack_weight(mode 0)  y: [N,Ho,Wo,ldy>=Cout]
 * residual: [N,Ho,Wo,ldr] or NULL; rowscale: [N*Ho*Wo] or NULL; chanscale: [N][Cin] or NULL.   */
int srhip_conv2d_fwd(const float* x, const float* packed, const float* bias, const float* residual,
                     const float* rowscale, const float* chanscale, float* y, int n, int h, int w, int cin, int cout, int kh,
                     int kw, int stride, int pad, int ldx, int ldy, int ldr, float slope, int flags,
                     void* stream);

/* ---- conv backward-data (autograd of the same call sites; second-order use in
 *      SRADSGAN.gradient_penalty :621,:639).  dy: [N,Ho,Wo,ldy] packed: mode 1  dx: [N,H,W,ldx].
 * Optional fused tail (Cout % 16 == 0): actmask [N,H,W,ldx] = the OUTPUT of the LeakyReLU(slope) that
 * produced this conv's input -- dx is multiplied by its derivative (backward of :242,:252 without a
 * separate pass); residual [N,H,W,ldr] is added afterwards (gradient of the skip path, :274).
 * accumulate != 0 adds into dx (gradient fan-in of the dense bus :459).                        */
int srhip_conv2d_dgrad(const float* dy, const float* packed, float* dx, const float* residual, const float* actmask,
                       float slope, int n, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad,
                       int ldy, int ldx, int ldr, int accumulate, void* stream);

/* ---- conv backward-weight: dw (OIHW) = sum over pixels of dy (x) window(x), and (db != NULL) the
 *      bias gradient db[co] = sum over pixels of dy.  Deterministic two-pass split-K (no atomics);
 *      `workspace` must hold srhip_conv2d_wgrad_workspace() bytes.  Optional xrowscale [N*H*W] /
 *      xchanscale [N][Cin]: x is read as x * xrowscale[pixel] * xchanscale[n][c] (the un-materialised
 *      input of the attention tail's 1x1 conv, sradsgan.py:262).  accumulate != 0 (only where
 *      srhip_conv2d_wgrad_can_accumulate): dw += ..., db += ... -- lets the caller point dw/db at the
 *      parameter's .grad slice of the gradient arena instead of paying one add launch per parameter. */
size_t srhip_conv2d_wgrad_workspace(int n, int h, int w, int cin, int cout, int kh, int kw, int stride,
                                    int pad);
int srhip_conv2d_wgrad_can_accumulate(int cin, int cout, int kh, int kw);
int srhip_conv2d_wgrad(const float* x, const float* dy, float* dw_oihw, float* db, const float* xrowscale,
                       const float* xchanscale, int accumulate, void* workspace,
                       size_t workspace_bytes, int n, int h, int w, int cin, int cout, int kh, int kw,
                       int stride, int pad, int ldx, int ldy, void* stream);

/* GROUPED weight gradient (round 3): nprob = 2..4 convolutions of the SAME shape (stride-1 pad-1 3x3, Cin % 64 == 0, split-bf16 or
 * half arithmetic, enough pixels: srhip_conv2d_wgrad_multi_ok returns the largest group size) in ONE main launch.  The chip wants one full wave of blocks whatever the number
 * of convolutions behind it, so each problem runs with 1 / nprob of the splits: split-K partial traffic, the write burst at the
 * end of the kernel and the reduce shrink by nprob.  x / dy / dw / db are HOST arrays of nprob device pointers (db or db[i] NULL:
 * no bias gradient); workspace as for srhip_conv2d_wgrad of one problem.  The dw[i], and the non-NULL db[i], of one call must be
 * DISTINCT (each problem's reduce reads, adds and writes its own destination without atomics): a repeated pointer is refused.  The step pairs the weight gradients of consecutive
 * RABs (model/sradsgan.py:222-223 of blocks i and i+1): nothing reads them before the optimiser.                     */
int srhip_conv2d_wgrad_multi_ok(int n, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad);   /* largest nprob (2..4), 0: not served */
int srhip_conv2d_wgrad_multi(int nprob, const float* const* x, const float* const* dy, float* const* dw, float* const* db,
                             int accumulate, void* workspace, size_t workspace_bytes, int n, int h, int w, int cin, int cout,
                             int kh, int kw, int stride, int pad, int ldx, int ldy, void* stream);
/* ---- ABI 9: padded split-bf16 planes ("pp") and the weight gradient as a flat GEMM over them (csrc/conv_wgrad_flat.hip) -------- *
 * Replaces nothing new in the reference: it is the autograd of the RAB convs (sradsgan.py:222-223, 250-252) like
 * srhip_conv2d_wgrad; what changes is the FORMAT the two 256-channel tensors inside a RAB (t = LeakyReLU(conv1 x) and its
 * gradient) are kept in between the block's own kernels.
 * pp of an NHWC tensor [N,H,W,C] (C % 8 == 0): srhip_pp_plane_pixels(n,h,w) pixel rows of C * 4 bytes; a row holds, for every
 * 8 channels, the 8 hi halves (hi = bf16(v)) followed by the 8 lo halves (lo = bf16(v - hi)) -- 32 bytes, the split the bf16x3
 * kernels form anyway.  srhip_pp_guard(w) zero rows come first, then pixel (n,y,x) at row (n*(H+1) + y)*(W+1) + x -- one zero
 * pixel behind every image row, one zero row behind every image --, then a zero tail.
 * The PAD / GUARD / TAIL ROWS MUST BE ZERO and no entry point ever writes them: allocate the buffer zeroed once and reuse it.
 * srhip_pp_from_f32 / srhip_pp_to_f32 convert (valid pixels only; to_f32 returns hi + lo).
 * srhip_conv2d_wgrad_pp: nprob (1..4) weight gradients of ONE 3x3 stride-1 pad-1 shape in one launch, split-bf16 arithmetic.
 * x_pp / dy_pp say which operands are pp (the other is fp32 NHWC with row stride ldf); srhip_conv2d_wgrad_pp_ok returns the served
 * combinations as a bit mask: 1 = x fp32 + dy pp (Cin % 64 == 0, Cout >= 128), 2 = x pp + dy fp32 (Cout == 64, Cin % 128 == 0),
 * 4 = both pp (Cin % 64 == 0 and Cout >= 256, or Cout == 64 and Cin % 256 == 0: the 8-wave kernel, one block per CU).
 * dw[i] (OIHW) and db[i] (optional) written or accumulated into; deterministic two-pass split-K as srhip_conv2d_wgrad. */
int srhip_pp_guard(int w);
/* 3x3 stride-1 pad-1 conv forward / data gradient with padded-plane operands (split-bf16 arithmetic; the persistent patch kernel,
 * csrc/conv_patch_pers.hip): x_pp / y_pp (dy_pp / dx_pp) say which side is pp, the other is DENSE fp32 NHWC (row stride = channels).
 * A pp source skips the kernel's in-place split; a pp destination gets the epilogue's rows as hi | lo stores.  Replaces the same
 * nn.Conv2d call sites as srhip_conv2d_fwd / _dgrad inside the RAB (sradsgan.py:222-223, 250-252).
 * fwd: flags = SRHIP_EPI_BIAS | SRHIP_EPI_LRELU subset; pool != NULL (fp32 destination of 64 channels): also the CLAM pooling
 * partials as srhip_conv2d_fwd_pool.  dgrad: residual (fp32 destination only) is added; actmask (pp destination only) = the PP of
 * the LeakyReLU output that fed the forward conv: dx is multiplied by the activation's derivative. */
int srhip_conv2d_pp_ok(int n, int h, int w, int cin, int cout);
/* srhip_conv2d_fwd whose fp32 output also leaves as padded planes (the attention tail's 1x1 conv, sradsgan.py:262-274: the next RAB's
 * input in both forms); *served = 0 when the kernel that took the launch has no second destination (the caller converts y). */
int srhip_conv2d_fwd_dual(const float* x, const float* packed, const float* bias, const float* residual, const float* rowscale,
                          const float* chanscale, float* y, void* y_pp, int* served, int n, int h, int w, int cin, int cout, int kh,
                          int kw, int stride, int pad, int ldx, int ldy, int ldr, float slope, int flags, void* stream);
int srhip_conv2d_fwd_pp(const void* x, int x_pp, const float* packed, const float* bias, void* y, int y_pp, float* pool, size_t pool_sec_bytes,
                        int* nseg_out, int n, int h, int w, int cin, int cout, float slope, int flags, void* stream);
int srhip_conv2d_dgrad_pp(const void* dy, int dy_pp, const float* packed, void* dx, int dx_pp, const float* residual, const void* actmask,
                          float slope, int n, int h, int w, int cin, int cout, void* stream);
/* The data gradient of a 3x3 stride-1 (any fast-path) conv with up to THREE residuals of dx's geometry, contiguous rows (ld = cin):
 * dx = conv_transpose(dy, w) + residual + residual2 + residual3, added in this order (residual2 or residual3 may be NULL).  Stands
 * where autograd sums the gradients a block input receives from its consumers -- the first RAB of a ResGroup, the group's skip
 * connection (sradsgan.py:286-324) and the trunk's dense-sampling bus (:455-460) --: the data gradient that is computed last takes
 * the other two in its epilogue instead of two element-wise add passes over 24 MB tensors per group.  Where the launch is served by a
 * kernel without the extra operands (other arithmetic modes, small shapes) the library adds them with one srhip_sum_n pass, same order. */
int srhip_conv2d_dgrad_res3(const float* dy, const float* packed, float* dx, const float* residual, const float* residual2,
                            const float* residual3, int n, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad,
                            void* stream);
int srhip_conv2d_dgrad_pp_res3(const void* dy, int dy_pp, const float* packed, float* dx, const float* residual, const float* residual2,
                               const float* residual3, int n, int h, int w, int cin, int cout, void* stream);
/* The LeakyReLU mask between a plane-writing forward and the masked data gradient behind it as sign words: 1 bit per element, in the
 * order the persistent patch kernel's lanes convert them (opaque; srhip_conv2d_pp_sign_bytes(n, h, w, channels) bytes, 0 = shape not
 * served), written by _fwd_pp_signs (bias + LeakyReLU onto planes) and read by _dgrad_pp_signs INSTEAD of the hi plane of the
 * producer's output (autograd of the RAB's conv1 -> LeakyReLU -> conv2, sradsgan.py:222-223: the data gradient reads 3 MB of mask
 * instead of 48 at B = 32).  channels % 128 == 0; both calls must name the same [n, h, w, channels] tensor geometry. */
size_t srhip_conv2d_pp_sign_bytes(int n, int h, int w, int channels);
int srhip_conv2d_fwd_pp_signs(const void* x, int x_pp, const float* packed, const float* bias, void* y_planes, void* signs, size_t sign_bytes,
                              int n, int h, int w, int cin, int cout, float slope, void* stream);
int srhip_conv2d_dgrad_pp_signs(const void* dy, int dy_pp, const float* packed, void* dx_planes, const void* signs, size_t sign_bytes, float slope,
                                int n, int h, int w, int cin, int cout, void* stream);
long srhip_pp_plane_pixels(int n, int h, int w);
int srhip_pp_from_f32(const float* x_nhwc, void* pp, int n, int h, int w, int c, int ldx, void* stream);
int srhip_pp_to_f32(const void* pp, float* x_nhwc, int n, int h, int w, int c, int ldx, void* stream);
int srhip_conv2d_wgrad_pp_ok(int n, int h, int w, int cin, int cout);
size_t srhip_conv2d_wgrad_pp_workspace(int nprob, int x_pp, int dy_pp, int n, int h, int w, int cin, int cout);
int srhip_conv2d_wgrad_pp(int nprob, const void* const* x, const void* const* dy, int x_pp, int dy_pp, float* const* dw, float* const* db,
                          int accumulate, void* workspace, size_t workspace_bytes, int n, int h, int w, int cin, int cout, int ldf,
                          void* stream);

/* The same for a conv with a fused LeakyReLU (sradsgan.py:476: D's 3 -> 64 head conv), from the gradient at the ACTIVATED
 * output: dy * (y > 0 ? 1 : slope) is formed while dy is read, so no lrelu-backward pass is needed when only the weight and
 * bias gradients of the layer are wanted.  srhip_conv2d_wgrad_act_ok says whether the shape is served (3-channel 3x3
 * stride-1 convs at >= 65536 pixels); workspace as srhip_conv2d_wgrad_workspace. */
int srhip_conv2d_wgrad_act_ok(int n, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad);
int srhip_conv2d_wgrad_act(const float* x, const float* dy, const float* y, float slope, float* dw_oihw, float* db,
                           void* workspace, size_t workspace_bytes, int n, int h, int w, int cin, int cout, int kh, int kw,
                           int stride, int pad, int ldx, int ldy, void* stream);

/* Additive in ABI 14 -- the same head conv with an ACTIVATION RECORD: one 64-bit word per output pixel, bit c = (y[pixel][c] > 0)
 * for the 64 output channels (NaN, +0 and -0 give 0; srhip_conv2d_head_mask_bytes = n * h * w * 8, 8-byte aligned).  The forward
 * leaves the record behind and the three passes that apply the LeakyReLU's backward read it while they stage the gradient, so
 * no pass of its own multiplies the 382 MB gradient by the mask and nothing re-reads y:
 *   srhip_conv2d_fwd_head_mask   mask_out: y = lrelu(conv(x, w) + bias) AND its record (flags = BIAS | LRELU);
 *                                mask_in:  y = mask * conv(x, w), mask = bit ? 1 : slope (flags = 0): the gradient penalty's second-
 *                                order pass d_dy = mask * conv(ddx, w).  Exactly one of the two pointers.
 *   srhip_conv2d_dgrad_head_mask dx = conv_transpose(mask * dy, w)   (packed = the mode-1 packed weight, dense dy)
 *   srhip_conv2d_wgrad_head_mask dw = wgrad(x, mask * dy), db = column sums of mask * dy (db may be NULL); workspace as
 *                                srhip_conv2d_wgrad_workspace.
 * Every result equals, bit for bit, the one of srhip_lrelu_bwd followed by (or following) the plain entry point.
 * srhip_conv2d_head_mask_ok: 3x3 stride-1 pad-1, cin <= 3, cout == 64, >= 65536 pixels, 3 * (w + 2) * cin * 4 <= 32 KB. */
int srhip_conv2d_head_mask_ok(int n, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad);
size_t srhip_conv2d_head_mask_bytes(int n, int h, int w, int cout);
int srhip_conv2d_fwd_head_mask(const float* x, const float* packed, const float* bias, float* y, void* mask_out, const void* mask_in,
                               size_t mask_bytes, int n, int h, int w, int cin, int cout, int ldx, int ldy, float slope, int flags,
                               void* stream);
int srhip_conv2d_dgrad_head_mask(const float* dy, const float* packed, float* dx, const void* mask, size_t mask_bytes, float slope, int n,
                                 int h, int w, int cin, int cout, int ldy, int ldx, void* stream);
int srhip_conv2d_wgrad_head_mask(const float* x, const float* dy, const void* mask, size_t mask_bytes, float slope, float* dw_oihw,
                                 float* db, void* workspace, size_t workspace_bytes, int n, int h, int w, int cin, int cout, int ldx,
                                 int ldy, void* stream);

/* ---- bias gradient: db[c] = sum_rows dy[row][c]; workspace >= srhip_colsum_workspace() bytes -- */
size_t srhip_colsum_workspace(long rows, int c);
int srhip_colsum(const float* dy, float* db, void* workspace, size_t workspace_bytes, long rows, int c,
                 int ld, void* stream);

/* ---- elementwise / permutation pieces of the same call sites --------------------------------- */
/* dx = dy * (y > 0 ? 1 : slope): backward of the in-place LeakyReLU (:242,:479) from its OUTPUT  */
int srhip_lrelu_bwd(const float* dy, const float* y, float* dx, long count, float slope, void* stream);
/* ABI 9: the same with the SIGN of y as a bit mask (one bit per element): y != NULL reads y and also WRITES the mask, y == NULL reads the
 * mask INSTEAD of y.  The gradient penalty (sradsgan.py:621, 639) applies the backward of the discriminator's first LeakyReLU twice to
 * the same 382 MB activation -- first order, then its double backward --: the second application reads 12 MB. */
size_t srhip_lrelu_mask_bytes(long count);
int srhip_lrelu_bwd_bits(const float* dy, const float* y, void* mask, float* dx, long count, float slope, void* stream);
/* ABI 7: out = ((srcs[0] + srcs[1]) + srcs[2]) + ... (n = 2..16 dense tensors of `count` floats, count % 4 == 0, 16-byte aligned):
 * the stratified dense-sampling bus of GeneratorResNet.forward (sradsgan.py:455-460: `bus = bus + out` after every residual
 * group) in one pass, same summation order as the chained torch adds it replaces.                                            */
int srhip_sum_n(const float* const* srcs, int n, float* out, long count, void* stream);
/* ABI 12 -- DSSR's wide-activation block tail (model/dssr.py:69-104): out = s * u + x with s[n,c] = sigmoid(fc2 relu(fc1 mean_hw u)),
 * the average-pool-only channel attention (bias-free 64 -> hidden -> 64 MLP, hidden <= 16) followed by the block's `out += x`.
 * u, x, g, du, out: NHWC with C == 64 dense channels, 16-byte aligned; avg, s, dmean: [n][64]; hid: [n][hidden].
 *   srhip_ca_pool_sum    : psum[n][srhip_ca_segments()][64] = per-segment channel sums of u (when no conv epilogue left them:
 *                          the sum section of srhip_conv2d_fwd_pool's partials has the same layout, with its own nseg)
 *   srhip_ca_mlp_fwd     : avg = sum of the nseg partials / hw, hid = relu(fc1 avg), s = sigmoid(fc2 hid), one block per image
 *   srhip_ca_scale_res   : out = s * u + x (s * u is never written on its own)
 *   srhip_ca_bwd_partial : part[n][srhip_ca_segments()][64] = per-segment sums of g * u (fixed order, no atomics)
 *   srhip_ca_mlp_bwd     : the MLP and sigmoid backward (one block per image, then one pass for the weights): dfc1 [hidden][64],
 *                          dfc2 [64][hidden] (written, summed over the images in order) and dmean = d(loss)/d(mean_hw u) / hw;
 *                          workspace >= srhip_ca_mlp_bwd_workspace(n, hidden)
 *   srhip_ca_bwd_du      : du = s * g + dmean (dx = g is the caller's)
 * All results are bit-identical from run to run.
 * The upsampler fold (model/dssr.py:170-177: sum_i UP(x_i) = UP(sum_i x_i) + G UP(0), UP affine):
 *   srhip_add_bcast_scaled : out[b][i] = a[b][i] + scale * bcast[i], per_image % 4 == 0
 *   srhip_batch_sum_scaled : out[i] = scale * sum_b g[b][i], images in order (its backward)                                    */
int srhip_ca_segments(void);
int srhip_ca_pool_sum(const float* u, float* psum, int n, int hw, int c, void* stream);
int srhip_ca_mlp_fwd(const float* psum, int nseg, const float* fc1, const float* fc2, float* avg, float* hid, float* s, int n, int hw,
                     int c, int hidden, void* stream);
int srhip_ca_scale_res(const float* u, const float* s, const float* x, float* out, int n, int hw, int c, void* stream);
int srhip_ca_bwd_partial(const float* g, const float* u, float* part, int n, int hw, int c, void* stream);
size_t srhip_ca_mlp_bwd_workspace(int n, int hidden);
int srhip_ca_mlp_bwd(const float* part, const float* avg, const float* hid, const float* s, const float* fc1, const float* fc2,
                     float* dmean, float* dfc1, float* dfc2, void* workspace, size_t workspace_bytes, int n, int hw, int c, int hidden,
                     void* stream);
int srhip_ca_bwd_du(const float* g, const float* s, const float* dmean, float* du, int n, int hw, int c, void* stream);
/* ABI 14, additive -- RCAN's channel attention (model/drcan.py:94-111: CALayer.conv_du = 1x1 (+b1), ReLU, 1x1 (+b2), sigmoid) on the
 * same kernels as the bias-free entries above; b1 [hidden], b2 [64], db1 [hidden], db2 [64]:
 *   srhip_ca_mlp_fwd_bias : hid = relu(fc1 avg + b1), s = sigmoid(fc2 hid + b2)
 *   srhip_ca_mlp_bwd_bias : srhip_ca_mlp_bwd plus db2[c] = sum_b dl[b,c] and db1[j] = sum_b dh[b,j] (dl = d(loss)/d(fc2 hid + b2),
 *                           dh = d(loss)/d(fc1 avg + b1)), images summed in order in the weight-gradient pass
 * Any bias pointer may be NULL: that bias is absent (forward) or its gradient is not written (backward).  With all of them NULL the
 * results are bit-identical to srhip_ca_mlp_fwd / srhip_ca_mlp_bwd.  hidden = 4 and 16 are RCAN's reduction 16 and 4.           */
int srhip_ca_mlp_fwd_bias(const float* psum, int nseg, const float* fc1, const float* b1, const float* fc2, const float* b2, float* avg,
                          float* hid, float* s, int n, int hw, int c, int hidden, void* stream);
int srhip_ca_mlp_bwd_bias(const float* part, const float* avg, const float* hid, const float* s, const float* fc1, const float* fc2,
                          float* dmean, float* dfc1, float* db1, float* dfc2, float* db2, void* workspace, size_t workspace_bytes, int n,
                          int hw, int c, int hidden, void* stream);
int srhip_add_bcast_scaled(const float* a, const float* b, float scale, float* out, int n, long per_image, void* stream);
int srhip_batch_sum_scaled(const float* g, float scale, float* out, int n, long per_image, void* stream);
/* ABI 14, additive -- HAT's window transformer (model/hat.py; csrc/hat.hip).  Tokens are NHWC rows of C = 96 floats (6 heads of 16).
 * Every reduction is a fixed-order sum: the results are bit-identical from run to run.
 *   srhip_hat_ln_fwd   : nn.LayerNorm(96) (eps 1e-5) per token: y, mean [tokens], rstd [tokens]
 *   srhip_hat_ln_bwd   : dx (+ dadd when not NULL), dgamma / dbeta written (NULL: not written); part: float workspace
 *                        [srhip_hat_ln_parts(tokens)][192]
 *   srhip_hat_gelu_fwd / _bwd : nn.GELU() (erf) and its backward, count % 4 == 0, 16-byte aligned
 *   srhip_hat_attn_fwd : window attention on qkv [n*h*w][288] (channel part * 96 + head * 16 + d, the qkv Linear's output):
 *                        kind 0 = HAB's W-MSA (shift 0) / SW-MSA (shift ws/2: roll, and the shift mask's -100), kind 1 = OCAB's
 *                        overlapping cross-attention (queries: ws x ws windows; keys / values: the (ws + ws/2)^2 unfold of the
 *                        qkv output with zero padding).  table [(2L-1)^2][6] is the relative-position bias table, indexed
 *                        modulo its size.  out [n*h*w][96] at the original pixel positions, lse [n*h*w][6] the rows' log-sum-exp.
 *                        ws 8 or 9, h and w multiples of ws.
 *   srhip_hat_attn_bwd : dqkv [n*h*w][288] (written) and dtable (written) from out, dout and lse; workspace >=
 *                        srhip_hat_attn_bwd_workspace(kind, n, h, w, ws)
 *   srhip_hat_ca_fwd   : CAB's channel attention, C <= 128, 1 <= hidden <= 16: s[n][C] = sigmoid(w2 relu(w1 mean_hw u + b1) + b2);
 *                        mz [n][C + hidden] keeps the mean and the hidden units for the backward (b1 / b2 may be NULL)
 *   srhip_hat_combine_fwd : HAB's out = (x + kb[b] a) + cs (s[b,c] u); kb NULL: 1; u NULL: no third term (the MLP branch)
 *   srhip_hat_combine_bwd : da = kb[b] g; with u: du = cs s g + d(mean)/hw through the channel attention and its parameter
 *                        gradients dw1 [hidden][C], db1, dw2 [C][hidden], db2 (written, images summed in order; NULL: not written);
 *                        workspace >= srhip_hat_combine_bwd_workspace(n, C, hidden).  dx = g is the caller's.
 * Argument errors return SRHIP_ERR_ARG, a NULL or too small workspace SRHIP_ERR_WORKSPACE, both before any launch and with a
 * message that names the entry point.                                                                                          */
int srhip_hat_ln_parts(long tokens);
int srhip_hat_ln_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, long tokens,
                     void* stream);
int srhip_hat_ln_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, const float* dadd,
                     float* dx, float* part, float* dgamma, float* dbeta, long tokens, void* stream);
int srhip_hat_gelu_fwd(const float* x, float* y, long count, void* stream);
int srhip_hat_gelu_bwd(const float* dy, const float* x, float* dx, long count, void* stream);
int srhip_hat_attn_fwd(const float* qkv, const float* table, float* out, float* lse, int kind, int n, int h, int w, int ws, int shift,
                       void* stream);
size_t srhip_hat_attn_bwd_workspace(int kind, int n, int h, int w, int ws);
int srhip_hat_attn_bwd(const float* qkv, const float* table, const float* out, const float* dout, const float* lse, float* dqkv,
                       float* dtable, void* workspace, size_t workspace_bytes, int kind, int n, int h, int w, int ws, int shift,
                       void* stream);
int srhip_hat_ca_fwd(const float* u, const float* w1, const float* b1, const float* w2, const float* b2, float* s, float* mz, int n,
                     long hw, int c, int hidden, void* stream);
int srhip_hat_combine_fwd(const float* x, const float* a, const float* kb, const float* u, const float* s, float* out, float cs, int n,
                          long hw, int c, void* stream);
size_t srhip_hat_combine_bwd_workspace(int n, int c, int hidden);
int srhip_hat_combine_bwd(const float* g, const float* kb, const float* u, const float* s, const float* mz, const float* w1,
                          const float* w2, float* da, float* du, float* dw1, float* db1, float* dw2, float* db2, void* workspace,
                          size_t workspace_bytes, float cs, int n, long hw, int c, int hidden, void* stream);
/* ABI 14, additive -- HAT at its published widths (csrc/hat_wide.hip; the channel attention in csrc/hat.hip): embed_dim C = 144 or
 * 180, heads of 24 or 30 channels, window 16 with overlap 0.5 (key window 24 x 24, padding 4).  The contracts are those of the
 * srhip_hat_* entries above with the width, the head count and the window as arguments; srhip_hat_gelu_* and srhip_hat_combine_fwd
 * take any width and serve both families.  Exact fp32 whatever the conv arithmetic mode, no atomics, fixed-order reductions.
 *   srhip_hatw_ln_fwd / _bwd : nn.LayerNorm(C) (eps 1e-5), 128 < C <= 192, C % 4 == 0; part: [srhip_hatw_ln_parts(tokens)][2C]
 *   srhip_hatw_attn_fwd : qkv [n*h*w][3C] (part * C + head * D + d), D = C / heads = 24 or 30, 1 to 6 heads, ws = 16, h and w multiples of 16,
 *                        shift 0 or 8 (kind 0 only); table [961 (kind 0) or 1521 (kind 1)][heads]; out [n*h*w][C], lse [n*h*w][heads].
 *                        qkv, out, dout, dqkv and the workspace are 16-byte aligned.
 *   srhip_hatw_attn_bwd : dqkv and dtable (written); workspace >= srhip_hatw_attn_bwd_workspace(kind, n, h, w, C, heads, ws) holds
 *                        the table-gradient partials by table row, delta = rowsum(dO o O) and, for kind 1, the per-window dk / dv
 *                        slabs -- never an element per (query, key) pair.
 *   srhip_hatw_ca_fwd / srhip_hatw_combine_bwd : srhip_hat_ca_fwd / srhip_hat_combine_bwd at 128 < C <= 192 (workspace:
 *                        srhip_hat_combine_bwd_workspace).
 * Anything else returns SRHIP_ERR_ARG (SRHIP_ERR_WORKSPACE for a NULL or too small workspace) before any launch. */
int srhip_hatw_ln_parts(long tokens);
int srhip_hatw_ln_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, long tokens, int c,
                      void* stream);
int srhip_hatw_ln_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, const float* dadd,
                      float* dx, float* part, float* dgamma, float* dbeta, long tokens, int c, void* stream);
int srhip_hatw_attn_fwd(const float* qkv, const float* table, float* out, float* lse, int kind, int n, int h, int w, int c, int heads,
                        int ws, int shift, void* stream);
size_t srhip_hatw_attn_bwd_workspace(int kind, int n, int h, int w, int c, int heads, int ws);
int srhip_hatw_attn_bwd(const float* qkv, const float* table, const float* out, const float* dout, const float* lse, float* dqkv,
                        float* dtable, void* workspace, size_t workspace_bytes, int kind, int n, int h, int w, int c, int heads, int ws,
                        int shift, void* stream);
int srhip_hatw_ca_fwd(const float* u, const float* w1, const float* b1, const float* w2, const float* b2, float* s, float* mz, int n,
                      long hw, int c, int hidden, void* stream);
int srhip_hatw_combine_bwd(const float* g, const float* kb, const float* u, const float* s, const float* mz, const float* w1,
                           const float* w2, float* da, float* du, float* dw1, float* db1, float* dw2, float* db2, void* workspace,
                           size_t workspace_bytes, float cs, int n, long hw, int c, int hidden, void* stream);
/* ABI 13 -- NDSRGAN (model/ndsrgan.py:57-211).  Rows are pixels; every operand has its own row stride (floats, multiple of 4, >= ch),
 * all pointers 16-byte aligned, ch % 4 == 0.  A dense block keeps its input and the four CL outputs in ONE [n, h, w, 192] buffer:
 * CL j reads channels 0 : 64+32j (srhip_conv2d_fwd ldx = 192) and writes 64+32j : 96+32j (ldy = 192), and the passes below write a
 * block's result straight into channels 0:64 of the next block's buffer -- no torch.cat, no copy.
 *   srhip_scaled_res_fwd   : y = r + alpha * c (c NULL: y = r), z = s + beta * y; y or z NULL: not written.  DenseBlock / DCRDB end
 *                            in `r + conv * 0.2` (:75, :92) and the trunk forms running sums `s + 0.2 * y` (:89-91, :121-146), in
 *                            the reference's fp32 operation order.
 *   srhip_scaled_res_bwd   : dc = ka * dz (dc non-NULL); dr[0:ch] = kb * dz + kc * e (e optional), dr[ch:width] = 0 (dr non-NULL):
 *                            the gradient at the conv and the initial gradient of a dense-block buffer in one pass.
 *   srhip_lrelu_bwd_strided: dx = dy * (y > 0 ? 1 : slope) over ch channels (in place when dx == dy): the CL's LeakyReLU(0.2)
 *                            backward, the mask from the post-activation values in the buffer.  dy and dx have one row stride
 *                            (ldx == ldg), in place or not; anything else is SRHIP_ERR_ARG.
 *   srhip_upsample_nearest_fwd / _bwd: nn.UpsamplingNearest2d(r), r in {2, 3}, NHWC [n, h, w, c] <-> [n, r h, r w, c]; the backward
 *                            sums each r x r block in a fixed order (no atomics).                                                  */
int srhip_scaled_res_fwd(const float* r, int ldr, const float* c, int ldc, const float* s, int lds, float alpha, float beta, float* y,
                         int ldy, float* z, int ldz, long rows, int ch, void* stream);
int srhip_scaled_res_bwd(const float* dz, int ldz, const float* e, int lde, float ka, float kb, float kc, float* dc, int ldc, float* dr,
                         int ldr, int width, long rows, int ch, void* stream);
int srhip_lrelu_bwd_strided(const float* dy, int ldg, const float* y, int ldy, float* dx, int ldx, float slope, long rows, int ch,
                            void* stream);
int srhip_upsample_nearest_fwd(const float* x, float* y, int n, int h, int w, int c, int r, void* stream);
int srhip_upsample_nearest_bwd(const float* dy, float* dx, int n, int h, int w, int c, int r, void* stream);
/* ABI 14 -- dilated 3x3 convolutions, stride 1, pad = dilation, dilation 1..3 (AMSSRN's ASPP, amssrn.py:200-217).  Same packed weight
 * as a plain 3x3 conv of that shape (srhip_pack_weight), same arithmetic modes.  Channels and row strides % 4 == 0, 16-byte aligned
 * tensors; x / dx / dy / y rows have their own strides (ASPP writes its three outputs straight into one [n, h, w, 768] buffer).
 * Dilation 1 is the plain 3x3 call.  Dilation d > 1 runs as the plain 3x3 conv of the d^2 polyphase sub-images (pixels with equal
 * (h mod d, w mod d)) stacked as a batch of n d^2 images of ceil(h/d) x ceil(w/d) pixels: exact, and every kernel and knob of the plain
 * path applies.  The workspace holds the gathered sub-images (srhip_conv2d_dil_workspace: kind 1 forward, 2 data gradient, 3 weight
 * gradient; 0 bytes for dilation 1 except kind 3).
 *   srhip_conv2d_fwd_dil  : y = act(conv(x [* chanscale[n][c]]) + bias); flags: SRHIP_EPI_BIAS | SRHIP_EPI_LRELU | SRHIP_EPI_CHANSCALE.
 *   srhip_conv2d_dgrad_dil: dx (=|+=, accumulate) conv_transpose(dy, w).
 *   srhip_conv2d_wgrad_dil: dw (OIHW) and db (optional) (=|+=, accumulate), from x and dy; accumulate only where
 *                           srhip_conv2d_wgrad_can_accumulate(cin, cout, 3, 3) holds (the plain call's rule).                      */
size_t srhip_conv2d_dil_workspace(int kind, int n, int h, int w, int cin, int cout, int dilation);
int srhip_conv2d_fwd_dil(const float* x, const float* packed, const float* bias, const float* chanscale, float* y, void* workspace,
                         size_t workspace_bytes, int n, int h, int w, int cin, int cout, int dilation, int ldx, int ldy, float slope,
                         int flags, void* stream);
int srhip_conv2d_dgrad_dil(const float* dy, const float* packed, float* dx, void* workspace, size_t workspace_bytes, int n, int h, int w,
                           int cin, int cout, int dilation, int ldy, int ldx, int accumulate, void* stream);
int srhip_conv2d_wgrad_dil(const float* x, const float* dy, float* dw, float* db, int accumulate, void* workspace, size_t workspace_bytes,
                           int n, int h, int w, int cin, int cout, int dilation, int ldx, int ldy, void* stream);
/* ABI 14 -- nn.PReLU() with one slope `a` that stays on the device (amssrn.py:176, 189, 212).  Rows are pixels with their own strides
 * (multiples of 4, >= ch), ch % 4 == 0, 16-byte aligned; in place when the two tensors and their strides coincide (the
 * backward: dz may alias g or z only with the same row stride).
 *   srhip_prelu_fwd         : y = z > 0 ? z : a z.
 *   srhip_prelu_bwd         : dz = z > 0 ? g : a g (from the pre-activation z, right for any sign of a), and the slope gradient
 *                             sum (z > 0 ? 0 : z g) as srhip_prelu_parts() fixed-order partials.
 *   srhip_prelu_slope_reduce: da (=|+=) the sum of nparts partials in a fixed order: one call over the partials of every application
 *                             of a shared slope.  No atomics: reruns are bit-identical.                                           */
int srhip_prelu_parts(void);
int srhip_prelu_fwd(const float* z, int ldz, float* y, int ldy, const float* slope, long rows, int ch, void* stream);
int srhip_prelu_bwd(const float* g, int ldg, const float* z, int ldz, float* dz, int lddz, const float* slope, float* partials, long rows,
                    int ch, void* stream);
int srhip_prelu_slope_reduce(const float* partials, int nparts, float* da, int accumulate, void* stream);
/* ABI 14 -- AMSSRN's non-local attention on image quadrants (Nonlocal_CA, amssrn.py:93-165) and the gamma residual (:326-328).
 *   srhip_nl_quad_fwd : per quadrant of the split at h / 2, w / 2, y = softmax(theta^T phi) g; theta, phi, g, y dense NHWC tensors of
 *                       8 channels, [n, h, w, 8]; ml [n h w, 2] receives the row maximum and row sum of every query (for the backward).
 *                       A NaN logit makes the row's y and row sum NaN, as torch's softmax; the saved maximum alone is not torch's
 *                       amax there: it is the maximum of the row's logits that are not NaN (-inf when all are), and is only ever
 *                       read together with the row sum.
 *   srhip_nl_quad_bwd : dtheta, dphi, dg from dy (same layout); dd [n h w] is scratch (dy . y per query).  Exact fp32, no atomics.
 *   srhip_gamma_res_fwd: out = a + gamma * b (gamma: one device float), dense, count % 4 == 0.
 *   srhip_gamma_res_bwd: db = gamma * g (db may be NULL) and srhip_gamma_parts() fixed-order partials of sum(g * b) (reduce with
 *                        srhip_prelu_slope_reduce).                                                                           */
int srhip_nl_quad_fwd(const float* theta, const float* phi, const float* g, float* y, float* ml, int n, int h, int w, void* stream);
int srhip_nl_quad_bwd(const float* theta, const float* phi, const float* g, const float* y, const float* ml, const float* dy, float* dd,
                      float* dtheta, float* dphi, float* dg, int n, int h, int w, void* stream);
int srhip_gamma_parts(void);
int srhip_gamma_res_fwd(const float* a, const float* b, const float* gamma, float* out, long count, void* stream);
int srhip_gamma_res_bwd(const float* g, const float* b, const float* gamma, float* db, float* partials, long count, void* stream);
/* ABI 11: torch.cat(dim = 1) of n = 2..8 NHWC tensors with `rows` pixel rows each and chans[k] channels (multiples of 4, 16-byte aligned
 * tensors) -- the multi-scale block's three branches, sradsgan.py:340-344 -- and its backward: the wide tensor split back into n dense ones. */
int srhip_cat_channels(const float* const* srcs, const int* chans, int n, float* out, long rows, void* stream);
int srhip_split_channels(const float* in, const int* chans, int n, float* const* dsts, long rows, void* stream);
/* nn.MaxPool2d(2,2) of vgg19.features[4] / [9] (sradsgan.py:92-95) on NHWC, even H and W, C % 4 == 0.
 * bwd recomputes the argmax from x (first maximum in window scan order, like ATen); relu_input != 0
 * also applies the backward of the ReLU that produced x (dx = 0 where the window maximum is 0).   */
int srhip_maxpool2x2_fwd(const float* x, float* y, int n, int h, int w, int c, void* stream);
int srhip_maxpool2x2_bwd(const float* dy, const float* x, float* dx, int n, int h, int w, int c, int relu_input,
                         void* stream);
/* ABI 9: the forward that also leaves a 2-byte record per 4 output elements (per channel: the arg-max position of the window, first
 * maximum in scan order, and whether the maximum is > 0) -- n (h/2) (w/2) (c/4) records --, and the backward that reads the records
 * INSTEAD of x (1 / 32 of its bytes): same dx as srhip_maxpool2x2_bwd. */
int srhip_maxpool2x2_fwd_idx(const float* x, float* y, void* rec, int n, int h, int w, int c, void* stream);
int srhip_maxpool2x2_bwd_idx(const float* dy, const void* rec, float* dx, int n, int h, int w, int c, int relu_input, void* stream);
/* nn.PixelShuffle(r) (:382,:385) on NHWC, fused with the LeakyReLU(slope) that follows it (:383):
 * out[n,h*r+i,w*r+j,c] = act(in[n,h,w,c*r*r+i*r+j]);  backward = inverse permutation * mask(out) */
int srhip_pixel_shuffle_fwd(const float* in, float* out, int n, int h, int w, int cout, int r,
                            float slope, int apply_act, void* stream);
int srhip_pixel_shuffle_bwd(const float* dout, const float* out, float* din, int n, int h, int w,
                            int cout, int r, float slope, int apply_act, void* stream);

/* ---- fused local-attention tail of RAB / ResGroup (sradsgan.py:254-274, 303-323; CLAM :117-127,
 *      SLAM :141-151), C == 64.  u: [N,H,W,64] (conv2 output).  Forward produces the two scales
 *      s[N][64] (CLAM) and m[N*H*W] (SLAM) plus what backward needs: avg/mx [N][64], argmax_hw [N][64]
 *      (first max pixel per channel), pooled [N*H*W][2] (mean_c, max_c of s*u), argc [N*H*W] (first
 *      max channel).  The caller then runs srhip_conv2d_fwd(u, ..., rowscale=m, chanscale=s,
 *      residual=skip): y and z of the reference are never written to HBM.                         */
size_t srhip_attn_tail_workspace(int n);
int srhip_attn_tail_fwd(const float* u, const float* fc1, const float* fc2, const float* w7, float* avg, float* mx,
                        int* argmax_hw, float* s, float* pooled, int* argc, float* m, void* workspace,
                        size_t workspace_bytes, int n, int h, int w, int c, int hidden, void* stream);

/* Inference form of the tail (ABI 6): out = conv1x1(SLAM(CLAM(u))) + bc + skip in TWO launches (pooling partials, one fused
 * kernel: MLP, pooled map with its 3-pixel halo, 7x7 conv, 1x1 conv on the MFMA, gate + bias + skip epilogue) and nothing saved
 * for a backward.  wc_packed = srhip_pack_weight(mode 0) image of the 1x1 conv (its split-bf16 section is read), bc may be NULL,
 * workspace >= srhip_attn_tail_workspace(n).  Split-bf16 arithmetic only (SRHIP_ERR_ARG otherwise); bit-identical to
 * srhip_attn_tail_fwd + srhip_conv2d_fwd(EPI bias|residual|rowscale|chanscale) in that mode.
 * Replaces: the eval-mode forward of model/sradsgan.py:254-274 and :303-323 (mfeNew_validate's generator pass).          */
int srhip_attn_tail_eval(const float* u, const float* skip, const float* fc1, const float* fc2, const float* w7,
                         const float* wc_packed, const float* bc, float* out, void* workspace, size_t workspace_bytes, int n, int h,
                         int w, int c, int hidden, void* stream);
/* ABI 8 -- the CLAM pooling partials (sradsgan.py:108-121: adaptive avg / max pool of the RAB conv2 output) as an object of their
 * own, so that the conv that PRODUCES u can leave them behind from its epilogue instead of a separate pass over u.
 * pool = three sections [sum | NaN-propagating max | first arg-max pixel (int32)] of pool_sec_bytes each, [image][segment][64]
 * inside a section; pool_sec_bytes >= n * srhip_clam_pool_max_segments() * 64 * 4, a multiple of 16.
 *   srhip_conv2d_fwd_pool   : stride-1 pad-1 3x3 conv to 64 dense channels (flags 0 or SRHIP_EPI_BIAS) + the partials of its output;
 *                             *nseg_out = segments per image written (epilogue of the persistent patch kernel: 2 x tiles per image;
 *                             any other kernel: srhip_clam_pool_partial on y, srhip_clam_pool_segments() segments)
 *   srhip_clam_pool_partial : the stand-alone pooling pass (what srhip_attn_tail_fwd / _eval run internally)
 *   srhip_attn_tail_fwd_pooled / srhip_attn_tail_eval_pooled: srhip_attn_tail_fwd / _eval without their pooling pass.          */
int srhip_clam_pool_segments(void);
int srhip_clam_pool_max_segments(void);
int srhip_clam_pool_partial(const float* u, float* pool, size_t pool_sec_bytes, int n, int h, int w, int c, void* stream);
int srhip_conv2d_fwd_pool(const float* x, const float* packed, const float* bias, float* y, float* pool, size_t pool_sec_bytes,
                          int* nseg_out, int n, int h, int w, int cin, int cout, int ldx, int ldy, int flags, void* stream);
int srhip_attn_tail_fwd_pooled(const float* u, const float* pool, size_t pool_sec_bytes, int nseg, const float* fc1, const float* fc2,
                               const float* w7, float* avg, float* mx, int* argmax_hw, float* s, float* pooled, int* argc, float* m,
                               int n, int h, int w, int c, int hidden, void* stream);
int srhip_attn_tail_eval_pooled(const float* u, const float* skip, const float* pool, size_t pool_sec_bytes, int nseg, const float* fc1,
                                const float* fc2, const float* w7, const float* wc_packed, const float* bc, float* out, int n, int h,
                                int w, int c, int hidden, void* stream);

/* backward, spatial half: dz = gradient at z (dgrad of the 1x1 conv).  Outputs du (partial: s * dy),
 * ds [N][64] (gradient at s), dw7 [2*7*7].  The caller back-propagates ds through sigmoid + MLP
 * (tiny, [N,64]) to davg/dmax and finishes with srhip_attn_tail_bwd_channel (in place on du).      */
size_t srhip_attn_tail_bwd_workspace(int n, int h, int w);
int srhip_attn_tail_bwd_spatial(const float* dz, const float* u, const float* s, const float* m, const float* pooled,
                                const int* argc, const float* w7, float* du, float* ds, float* dw7, int accumulate_dw7,
                                void* workspace, size_t workspace_bytes, int n, int h, int w, int c, void* stream);
/* backward, channel half: ds -> sigmoid -> shared MLP (sradsgan.py:110-112,124-126): davg/dmax [N][64],
 * dfc1 [hidden][64], dfc2 [64][hidden].                                                             */
size_t srhip_attn_tail_mlp_workspace(int n, int hidden);
int srhip_attn_tail_bwd_mlp(const float* ds, const float* avg, const float* mx, const float* s, const float* fc1,
                            const float* fc2, float* davg, float* dmax, float* dfc1, float* dfc2, int accumulate_dfc,
                            void* workspace, size_t workspace_bytes, int n, int c, int hidden, void* stream);
/* The three calls above as ONE (7 launches instead of 10 in the serial chain of every RAB / ResGroup backward; identical
 * arithmetic and summation orders): dz = gradient at z (from srhip_conv2d_dgrad of the 1x1 conv), everything else as saved
 * by srhip_attn_tail_fwd.  dw7 / dfc1 / dfc2 are written, or accumulated into when the flag is set.        */
size_t srhip_attn_tail_bwd_fused_workspace(int n, int h, int w, int hidden);
int srhip_attn_tail_bwd(const float* dz, const float* u, const float* s, const float* m, const float* pooled, const int* argc,
                        const float* avg, const float* mx, const int* argmax_hw, const float* w7, const float* fc1,
                        const float* fc2, float* du, float* dw7, int accumulate_dw7, float* dfc1, float* dfc2,
                        int accumulate_dfc, void* workspace, size_t workspace_bytes, int n, int h, int w, int c, int hidden,
                        void* stream);
/* ABI 9: the same with the FINAL du as padded split-bf16 planes (du_pp) instead of the fp32 tensor: the RAB's conv2 data and weight
 * gradient read the planes without a conversion pass.  `du` is then scratch (it holds the main pass's partial result, without the
 * channel-pooling terms); du_pp NULL: exactly srhip_attn_tail_bwd. */
int srhip_attn_tail_bwd_pp(const float* dz, const float* u, const float* s, const float* m, const float* pooled, const int* argc,
                        const float* avg, const float* mx, const int* argmax_hw, const float* w7, const float* fc1,
                        const float* fc2, float* du, void* du_pp, float* dw7, int accumulate_dw7, float* dfc1, float* dfc2,
                        int accumulate_dfc, void* workspace, size_t workspace_bytes, int n, int h, int w, int c, int hidden,
                        void* stream);
/* (ABI 10 removed srhip_attn_tail_bwd_g -- ABI 9's form that rebuilt dz = conv_transpose(g, wc) inside the passes: it was slower in the
 * training step, off by default, and carried a sporadic wrong result that was never explained) */
int srhip_attn_tail_bwd_channel(float* du, const float* davg, const float* dmax, const int* argmax_hw, int n, int h,
                                int w, int c, void* stream);

/* ---- the attention tail's ablations (sradsgan.py:101-151, 215-324: la_mode x pool_mode); csrc/attn_variants.hip ---------------- *
 * `order` is the la_mode, `pools` the pool set of both gates (bit 0 Avg, bit 1 Max).  With Chan(a) = sigmoid(sum over the pools
 * of fc2 relu(fc1 pool_pixels a)) and Spat(a) = sigmoid(conv7x7(the pooled channel maps of a, Avg first, pad 3)):
 *   CA_SA  s = Chan(u), m = Spat(s u)      SA_CA  m = Spat(u), s = Chan(m u)      CA  s = Chan(u)      SA  m = Spat(u)
 *   CA_PAR_SA ('CA|SA')  s = Chan(u), m = Spat(u)
 * u [n][hw][64] NHWC, C == 64, hidden 1..16, w7 [1][|pools|][7][7].  Outputs: avg, mx, s [n][64], arg [n][64] (first pixel attaining
 * the maximum of the tensor the channel gate pooled), pooled [n][hw][|pools|], argc [n][hw] (first channel), m [n][hw]; those a
 * variant does not have (no such gate, or a statistic outside the pool set) may be NULL and are not written.  Exact fp32 in every
 * conv arithmetic, no atomics, fixed reduction order.  The workspace (srhip_attn_var_workspace(n) bytes) is needed by the variants
 * with a channel gate.  Argument errors return SRHIP_ERR_ARG before any launch.  (Additive: the ABI version does not move.) */
#define SRHIP_ATTN_CA_SA 0
#define SRHIP_ATTN_SA_CA 1
#define SRHIP_ATTN_CA 2
#define SRHIP_ATTN_SA 3
#define SRHIP_ATTN_CA_PAR_SA 4
size_t srhip_attn_var_workspace(int n);
int srhip_attn_var_fwd(const float* u, const float* fc1, const float* fc2, const float* w7, float* avg, float* mx, int* arg, float* s,
                       float* pooled, int* argc, float* m, float* ws, size_t ws_bytes, int n, int h, int w, int c, int hidden,
                       int order, int pools, void* stream);
/* The closing pass of the variants that do not end in a 64 -> 64 1x1 conv (those hand m and s to srhip_conv2d_fwd as row and channel
 * scales).  cat == 0: out [n][hw][64] = z + skip with z = m (s u) for CA_SA, s (m u) for SA_CA, s u for CA, m u for SA, each product
 * and the add rounded once in fp32.  cat != 0 (CA_PAR_SA only): out [n][hw][128] = [s u, m u], the x operand of the 128 -> 64 conv;
 * skip is not read. */
int srhip_attn_var_close(const float* u, const float* s, const float* m, const float* skip, float* out, int n, int hw, int c, int order,
                         int cat, void* stream);
/* Backward of the same variants: the gradient dz at z ([n][hw][64]; CA_PAR_SA: [n][hw][128], channel half first) and the tensors
 * srhip_attn_var_fwd saved give du [n][hw][64], dw7 [1][|pools|][7][7], dfc1 [hidden][64], dfc2 [64][hidden]; the parameter gradients
 * are written, or accumulated into when their flag is set.  Max pools are differentiated at the saved first arg-max indices.  At most
 * three passes over (dz, u) for the two-gate sequential orders, two for the others; nothing tensor-sized is written but du.  No
 * atomics, fixed reduction order.  Tensors a variant does not have may be NULL.  Workspace: srhip_attn_var_bwd_workspace() bytes. */
size_t srhip_attn_var_bwd_workspace(int n, int h, int w, int hidden);
int srhip_attn_var_bwd(const float* dz, const float* u, const float* s, const float* m, const float* avg, const float* mx, const int* arg,
                       const float* pooled, const int* argc, const float* w7, const float* fc1, const float* fc2, float* du, float* dw7,
                       int accumulate_dw7, float* dfc1, float* dfc2, int accumulate_dfc, float* ws, size_t ws_bytes, int n, int h, int w,
                       int c, int hidden, int order, int pools, void* stream);

/* ---- global attention of GAB_UP (sradsgan.py:365-418), C == 64, NHWC [n][hw][64] ---------------- *
 * CGAM (channel self-attention, sradsgan.py:178-213, light=False; call site :395): E = X^T X per image,
 * A = softmax(rowmax(E) - E), y = gamma * (X A^T) + x.  Exact fp32 on the matrix pipe.  fwd saves A
 * (att [n][64][64]); bwd returns dx (incl. the residual path) and dgamma (accumulate_dgamma != 0: +=).
 * Both need srhip_cgam_workspace() bytes of 16-byte aligned scratch.  Every tensor but dgamma is required:
 * a NULL one is SRHIP_ERR_ARG, a NULL or too small workspace SRHIP_ERR_WORKSPACE, before any launch.  */
size_t srhip_cgam_workspace(int n, int hw);
int srhip_cgam_fwd(const float* x, const float* gamma, float* y, float* att, void* workspace, size_t workspace_bytes,
                   int n, int hw, int c, void* stream);
int srhip_cgam_bwd(const float* dy, const float* x, const float* att, const float* gamma, float* dx, float* dgamma,
                   int accumulate_dgamma, void* workspace, size_t workspace_bytes, int n, int hw, int c, void* stream);
/* SGAM (position self-attention, sradsgan.py:153-176; call site :397) on already projected q, k [n][hw][8] and
 * v [n][hw][64] (the 1x1 convs :157-159 are srhip_conv2d_fwd calls): y = gamma * softmax_j(q_i . k_j) v + x,
 * no 1/sqrt(d) scaling.  Flash-style: the hw x hw energy / attention matrices (torch.bmm + Softmax, :167-172) are
 * never written to memory; fwd saves o = softmax(.) v [n][hw][64] and the per-query log-sum-exp lse [n][hw];
 * bwd recomputes the probabilities (deterministic two-pass, no atomics) and returns dq, dk, dv and dgamma; the
 * gradient of the residual path is dy itself.  bwd needs srhip_sgam_flash_bwd_workspace() bytes.  Every
 * tensor but dgamma is required (NULL: SRHIP_ERR_ARG; workspace NULL or too small: SRHIP_ERR_WORKSPACE).  */
int srhip_sgam_flash_fwd(const float* q, const float* k, const float* v, const float* x, const float* gamma, float* y,
                         float* o, float* lse, int n, int hw, int dk, int c, void* stream);
size_t srhip_sgam_flash_bwd_workspace(int n, int hw);
int srhip_sgam_flash_bwd(const float* dy, const float* q, const float* k, const float* v, const float* o, const float* lse,
                         const float* gamma, float* dq, float* dk_out, float* dv, float* dgamma, int accumulate_dgamma,
                         void* workspace, size_t workspace_bytes, int n, int hw, int dk, int c, void* stream);

/* ---- channel / spatial attention primitives (ChannelAttention base_networks.py:366-403 and SpatialAttention :424-457 of
 *      the discriminator, sradsgan.py:495-496; the stand-alone CLAM / SLAM of sradsgan.py:101-151), NHWC [n][hw][c],
 *      c % 4 == 0.  The set is closed under differentiation -- pool <-> unpool (at the saved arg-max), scale <-> dot,
 *      sigmoid_bwd -> sigmoid_bwd_bwd -- so the WGAN-GP double backward (:621, :639) is composed of these launches only.
 * pool_hw:   t[n][2][c] = (mean, max over pixels); fixed_arg == 0 also writes arg[n][c] = first arg-max pixel,
 *            fixed_arg != 0 reads it instead (max row = x at that pixel).   unpool_hw: out[n][p][c] = t0/hw + (p==arg)*t1.
 * pool_c / unpool_c: the same over channels, t[n][hw][2], argc[n][hw].
 * scale:     out = x * s; mode 0: s[n][c], mode 1: s[n][hw].   dot: mode 0: out[n][c] = sum_hw a*b, mode 1: out[n][hw] = sum_c a*b.
 * sigmoid_*: y = sigmoid(x) (pair == 0, count elements) or y[n][c] = sigmoid(x[n][0][c] + x[n][1][c]) (pair != 0, the sum of
 *            the two MLP branches, base_networks.py:401); bwd: dx = g y (1-y) (both rows when pair); bwd_bwd: for a
 *            cotangent gg on dx: dg = gg y (1-y), dy = gg g (1-2y) (either output may be NULL).                   */
int srhip_cbam_pool_hw(const float* x, float* t, int* arg, int fixed_arg, int n, int hw, int c, void* stream);
int srhip_cbam_unpool_hw(const float* t, const int* arg, float* out, int n, int hw, int c, void* stream);
int srhip_cbam_pool_c(const float* x, float* t, int* argc, int fixed_arg, int n, int hw, int c, void* stream);
int srhip_cbam_unpool_c(const float* t, const int* argc, float* out, int n, int hw, int c, void* stream);
int srhip_cbam_scale(const float* x, const float* s, float* out, int n, int hw, int c, int mode, void* stream);
int srhip_cbam_dot(const float* a, const float* b, float* out, int n, int hw, int c, int mode, void* stream);
int srhip_sigmoid_fwd(const float* x, float* y, long count, int c, int pair, void* stream);
int srhip_sigmoid_bwd(const float* g, const float* y, float* dx, long count, int c, int pair, void* stream);
int srhip_sigmoid_bwd_bwd(const float* gg, const float* g, const float* y, float* dg, float* dy, long count, int c, int pair,
                          void* stream);

/* ---- loss reductions (deterministic two-stage sums; scalars stay on the device; every fwd needs
 *      srhip_reduce_workspace() bytes of scratch; bwd kernels read the incoming scalar gradient from `gout`) --
 * l1_mean:  nn.L1Loss() (sradsgan.py:686; pixel loss :834, content loss :838): out = mean |a - b|;
 *           bwd: da = sign(a - b) * gout / count, db = -da when db != NULL.
 * mean:     the WGAN critic means of GANLoss (sradsgan.py:61-66; :847, :876-878).
 * gp_norm_penalty: sradsgan.py:630-637 with 'L2' / 'LS': per-pixel L2 norm over the C (<= 4) channels of
 *           grads [npix][C], (norm - 1)^2, mean over pixels; bwd: d/dgrads (0 where the norm is 0, like torch). */
size_t srhip_reduce_workspace(void);
int srhip_l1_mean_fwd(const float* a, const float* b, float* out, void* workspace, size_t workspace_bytes, long count,
                      void* stream);
int srhip_l1_mean_bwd(const float* a, const float* b, const float* gout, float* da, float* db, long count, void* stream);
/* ABI 12 -- mse_mean: nn.MSELoss() (DSSR, model/dssr.py:266-269 with loss_Lp_norm='L2'): out = mean (a - b)^2;
 *           bwd: da = 2 (a - b) * gout / count, db = -da when db != NULL.  Any count (the tail that is not a multiple of 4 is
 *           read with scalar loads). */
int srhip_mse_mean_fwd(const float* a, const float* b, float* out, void* workspace, size_t workspace_bytes, long count,
                       void* stream);
int srhip_mse_mean_bwd(const float* a, const float* b, const float* gout, float* da, float* db, long count, void* stream);
/* ABI 13 -- smooth_l1_mean: nn.SmoothL1Loss() (beta = 1, mean; NDSRGAN, model/ndsrgan.py:325-351): out = mean sl1(a - t) with
 *           t = b[i], or the scalar `target` when b == NULL (D's valid / fake targets, no ones tensor); sl1(d) = |d| < 1 ? d^2 / 2 :
 *           |d| - 1/2.  bwd: da = clamp(a - t, -1, 1) * gout / count, db = -da when db != NULL (needs b). */
int srhip_smooth_l1_mean_fwd(const float* a, const float* b, float target, float* out, void* workspace, size_t workspace_bytes,
                             long count, void* stream);
int srhip_smooth_l1_mean_bwd(const float* a, const float* b, float target, const float* gout, float* da, float* db, long count,
                             void* stream);
int srhip_mean_fwd(const float* x, float* out, void* workspace, size_t workspace_bytes, long count, void* stream);
int srhip_mean_bwd(const float* gout, float* dx, long count, void* stream);
int srhip_gp_norm_penalty_fwd(const float* grads, float* out, void* workspace, size_t workspace_bytes, long npix, int c,
                              void* stream);
int srhip_gp_norm_penalty_bwd(const float* grads, const float* gout, float* dgrads, long npix, int c, void* stream);
/* ABI 14 (additive) -- gp_penalty: the gradient penalty under every option of sradsgan.py:624-637 (--grad_penalty_Lp_norm,
 *           --penalty_type), kinds by value.  norm over the C (<= 4) channels of a pixel: L2 sqrt(sum g^2) (gradient 0 where the
 *           norm is 0), L1 sum |g| (gradient sign(g), sign(0) = 0), Linf max |g| (the whole gradient, times sign(g), at the FIRST
 *           channel that attains the maximum, as torch.max(dim); an all-zero pixel gets 0).  penalty: LS (norm - 1)^2, factor
 *           2 (norm - 1); hinge relu(norm - 1), factor 1 where norm - 1 > 0 in fp32, else 0 (0 at exactly 1).  out = mean over
 *           npix; bwd: dgrads = gout / npix * factor * d norm / d grads.  Same two-stage fixed-tree sum as gp_norm_penalty, no
 *           atomics; (L2, LS) here is the arithmetic of gp_norm_penalty, which stays the default path.  Unknown kinds and
 *           C > 4 are refused. */
#define SRHIP_GP_NORM_L2 0
#define SRHIP_GP_NORM_L1 1
#define SRHIP_GP_NORM_LINF 2
#define SRHIP_GP_PENALTY_LS 0
#define SRHIP_GP_PENALTY_HINGE 1
int srhip_gp_penalty_fwd(const float* grads, float* out, void* workspace, size_t workspace_bytes, long npix, int c, int norm_kind,
                         int penalty_kind, void* stream);
int srhip_gp_penalty_bwd(const float* grads, const float* gout, float* dgrads, long npix, int c, int norm_kind, int penalty_kind,
                         void* stream);

/* ---- data-parallel gradient exchange over RCCL / xGMI (the reference is single-GPU, README.md:91).
 * One communicator per process = per GPU.  Rank 0 calls srhip_dp_unique_id and hands the srhip_dp_id_bytes() bytes
 * to every rank (any side channel: the host code uses torch.distributed's store); every rank then calls
 * srhip_dp_init with the current HIP device set.  srhip_dp_allreduce_bucket sums `count` floats in place over the
 * ranks, asynchronously on `stream` (the caller orders it against compute with events and folds 1/world into
 * srhip_adam_step's grad_scale); srhip_dp_broadcast makes replicas identical.  RCCL is bound with dlopen at the
 * first call.                                                                                            */
int srhip_dp_id_bytes(void);
int srhip_dp_unique_id(void* id_out);
int srhip_dp_init(const void* id_in, int rank, int world);
int srhip_dp_world(void);
int srhip_dp_rank(void);
int srhip_dp_allreduce_bucket(float* buf, size_t count, void* stream);
int srhip_dp_broadcast(float* buf, size_t count, int root, void* stream);
int srhip_dp_finalize(void);

/* ---- train-mode nn.BatchNorm2d + LeakyReLU (discriminator, sradsgan.py:478-479), NHWC [rows][C].
 * fwd: batch mean / biased variance -> y = act((x-mean)*invstd*gamma + beta); updates
 * running_mean/var in place (momentum, unbiased variance) unless NULL; saves mean and invstd.
 * bwd: dy is the gradient at y; the activation mask comes from y; produces dx, dgamma, dbeta.
 * bwd_bwd: the second-order pass of the gradient penalty (:621,:639): for a cotangent ddx on dx it
 * returns the gradients at dy (g_dy), at x (g_x) and at gamma (g_gamma); cotangents on dgamma/dbeta are
 * not supported here (the host composes that rare case from primitive ops).                          */
size_t srhip_bn_workspace(long rows, int c);
int srhip_bn_train_fwd(const float* x, const float* gamma, const float* beta, float* running_mean,
                       float* running_var, float* y, float* save_mean, float* save_invstd, void* workspace,
                       size_t workspace_bytes, long rows, int c, float eps, float momentum, float slope, int apply_act,
                       void* stream);
int srhip_bn_train_bwd(const float* dy, const float* x, const float* y, const float* gamma, const float* save_mean,
                       const float* save_invstd, float* dx, float* dgamma, float* dbeta, void* workspace,
                       size_t workspace_bytes, long rows, int c, float slope, int apply_act, void* stream);
/* ABI 7: the same pass, and acc_gamma[c] += dgamma[c], acc_beta[c] += dbeta[c] when the pointers are not NULL (the parameters'
 * .grad buffers: what optimizer-side accumulation of sradsgan.py:858/887 sees; one writer per channel, deterministic).      */
int srhip_bn_train_bwd_acc(const float* dy, const float* x, const float* y, const float* gamma, const float* save_mean,
                           const float* save_invstd, float* dx, float* dgamma, float* dbeta, float* acc_gamma,
                           float* acc_beta, void* workspace, size_t workspace_bytes, long rows, int c, float slope,
                           int apply_act, void* stream);
/* ABI 9: the same WITHOUT y: the LeakyReLU mask is the sign of the pre-activation recomputed from x with the forward's own expression
 * ((x - mean) * invstd * gamma + beta: bit-identical, so the same sign as y's) -- one tensor read less in each of the two passes */
int srhip_bn_train_bwd_acc_x(const float* dy, const float* x, const float* gamma, const float* beta, const float* save_mean,
                             const float* save_invstd, float* dx, float* dgamma, float* dbeta, float* acc_gamma,
                             float* acc_beta, void* workspace, size_t workspace_bytes, long rows, int c, float slope,
                             int apply_act, void* stream);
/* ... and with dx = (that backward) + addend formed in the apply pass (addend may be dx): a BatchNorm input's second gradient -- the one
 * the gradient penalty's double backward sends through the first-order backward's node, sradsgan.py:621-639 -- without autograd's
 * separate accumulation pass. */
int srhip_bn_train_bwd_acc_xa(const float* dy, const float* x, const float* gamma, const float* beta, const float* save_mean,
                              const float* save_invstd, const float* addend, float* dx, float* dgamma, float* dbeta, float* acc_gamma,
                              float* acc_beta, void* workspace, size_t workspace_bytes, long rows, int c, float slope,
                              int apply_act, void* stream);
/* eval()-mode nn.BatchNorm2d (+ activation): the per-channel affine of the running statistics (SRGAN's generator at
 * validation time, model/srgan.py; the SRADSGAN discriminator is never put in eval()).  Inference only.   */
int srhip_bn_eval_fwd(const float* x, const float* gamma, const float* beta, const float* running_mean,
                      const float* running_var, float* y, long rows, int c, float eps, float slope, int apply_act,
                      void* stream);
size_t srhip_bn_bwd2_workspace(long rows, int c);
int srhip_bn_train_bwd_bwd(const float* ddx, const float* dy, const float* x, const float* y, const float* gamma,
                           const float* save_mean, const float* save_invstd, float* g_dy, float* g_x, float* g_gamma,
                           void* workspace, size_t workspace_bytes, long rows, int c, float slope, int apply_act,
                           void* stream);
int srhip_bn_train_bwd_bwd_acc(const float* ddx, const float* dy, const float* x, const float* y, const float* gamma,
                               const float* save_mean, const float* save_invstd, float* g_dy, float* g_x, float* g_gamma,
                               float* acc_gamma, void* workspace, size_t workspace_bytes, long rows, int c, float slope,
                               int apply_act, void* stream);   /* ABI 7: + acc_gamma[c] += g_gamma[c] unless NULL */
/* ABI 9: the second-order pass without y (mask from the recomputed pre-activation, like srhip_bn_train_bwd_acc_x) */
int srhip_bn_train_bwd_bwd_acc_x(const float* ddx, const float* dy, const float* x, const float* gamma, const float* beta,
                                 const float* save_mean, const float* save_invstd, float* g_dy, float* g_x, float* g_gamma,
                                 float* acc_gamma, void* workspace, size_t workspace_bytes, long rows, int c, float slope,
                                 int apply_act, void* stream);

/* ---- per-sample normalisations + LeakyReLU of the patch discriminator (base_networks.py:1759-1767), NHWC x[n][p][c], p = H * W:
 * `groups` groups of C / groups adjacent channels, one statistic per (sample, group) over m = p * C / groups elements.  Instance norm
 * (nn.InstanceNorm2d(C)) is groups = C, unbiased = 0, gamma = beta = NULL; the reference's GroupNorm (base_networks.py:12-31) is
 * groups = 32, unbiased = 1 (x.var(-1)) with per-channel gamma / beta.  gamma and beta are given or NULL together.  Additive to ABI 14.
 * fwd: y = act((x - mean) * invstd * gamma + beta); saves mean and invstd, [n * groups] each.
 * bwd: dx (+ addend when not NULL; addend may be dx), dgamma, dbeta; acc_gamma / acc_beta += them when not NULL.  The LeakyReLU mask
 * is the sign of the pre-activation recomputed from x (no pass reads y).
 * bwd_bwd: for a cotangent u on dx, the gradients at dy, x and gamma (cotangents on dgamma / dbeta: the host composes that case).
 * Two-stage reductions without atomics whose order depends on (p, C, groups) only: y, dx, g_dy and g_x of a sample are bit-identical
 * whatever else is in the batch.  C % 4 == 0, C <= 1024, C % groups == 0, m >= 2, n <= 65535; anything else returns SRHIP_ERR_ARG and
 * writes nothing.  One workspace size (16-byte aligned) serves the three passes. */
size_t srhip_gn_workspace(long n, long p, int c);
int srhip_gn_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* invstd, void* workspace,
                 size_t workspace_bytes, long n, long p, int c, int groups, int unbiased, float eps, float slope, int apply_act,
                 void* stream);
int srhip_gn_bwd(const float* dy, const float* x, const float* gamma, const float* beta, const float* mean, const float* invstd,
                 const float* addend, float* dx, float* dgamma, float* dbeta, float* acc_gamma, float* acc_beta, void* workspace,
                 size_t workspace_bytes, long n, long p, int c, int groups, int unbiased, float slope, int apply_act, void* stream);
int srhip_gn_bwd_bwd(const float* u, const float* dy, const float* x, const float* gamma, const float* beta, const float* mean,
                     const float* invstd, float* g_dy, float* g_x, float* g_gamma, float* acc_gamma, void* workspace,
                     size_t workspace_bytes, long n, long p, int c, int groups, int unbiased, float slope, int apply_act, void* stream);

/* ---- validation metrics (mfeNew_validate / validate, sradsgan.py:1314-1325; utils/utils.py:923-962):
 *      images quantised like ToPILImage (mul(255).byte(): truncate + wrap, no clamp), NHWC floats in.
 * A byte cannot carry a NaN: a NaN element is quantised to byte 0.
 * quant_sse: partial uint64 [n][srhip_metric_blocks()][2] = {sum (a_u8-b_u8)^2, sum b_u8} (exact);
 * ssim_u8 (scikit-image 0.15 compare_ssim, multichannel, 7x7 uniform window): partial double
 * [n][srhip_metric_blocks()] = sums of the SSIM index over interior pixels and channels (a = test, b = truth). */
int srhip_metric_blocks(void);
int srhip_quant_sse(const float* a, const float* b, unsigned long long* partial, int n, long per_image, void* stream);
int srhip_ssim_u8(const float* a, const float* b, double* partial, int n, int h, int w, int c, void* stream);
/* ABI 9: the scalar tail of the two metric passes for all images in one launch: out = double [4][n], rows mse, psnr (inf where mse = 0),
 * ssim, ergas (utils.py:923-962) */
int srhip_metric_finish(const unsigned long long* sse_partial, const double* ssim_partial, double* out, int n, int h, int w, int c,
                        double scale, void* stream);

/* ---- evaluation by the papers' protocol (EDSR, RCAN, ESRGAN, SwinIR, HAT, BasicSR; calculate_psnr / calculate_ssim of
 *      GDP_x0/core/metrics.py:109-160 with BasicSR's crop_border / test_y_channel switches).  Additive, ABI 14.
 * a (test) and b (ground truth): [n][h][w][c] NHWC, c in {1, 3}; is_float = 0: uint8 bytes, 1: float32 in nominal [0, 1].
 * Quantisation (is_float = 1 only): q = (uint8) rintf(fminf(fmaxf(x, 0), 1) * 255.f) -- the float32 product rounded half to even,
 *   tensor2img with min_max = (0, 1), byte for byte what srhip_diff_quant_u8(lo 0, hi 1) writes.  A byte cannot carry a NaN: a NaN
 *   element is quantised to byte 0; +inf -> 255, -inf -> 0.
 * Crop: `crop` >= 0 rows and columns are removed on every side; the remaining h' x w' must be at least 11 x 11.
 * Channels: luma = 0: the c channels as they are.  luma = 1 (needs c = 3): one channel, num = 65481 r + 128553 g + 24966 b as an exact
 *   int32 and Y = 16.0 + num / 255000.0 in fp64, not rounded (BT.601 studio range, bgr2ycbcr(y_only=True); BasicSR passes Y through a
 *   float32 intermediate, this library does not).
 * MSE: mean over cropped pixels and channels of (a - b)^2 from an EXACT integer sum -- of squared byte differences, or in luma mode of
 *   squared differences of num, divided by 255000^2; psnr = 10 log10(255^2 / mse), +inf where mse = 0.
 * SSIM: g_i = exp(-(i - 5)^2 / 4.5) / sum, i = 0..10, in fp64; window g g^T.  At each of the (h' - 10)(w' - 10) positions whose window
 *   lies inside the cropped image, per channel: mu_a, mu_b, E[a^2], E[b^2], E[ab] as window-weighted sums, s_a^2 = E[a^2] - mu_a^2,
 *   s_b^2 likewise, s_ab = E[ab] - mu_a mu_b (population covariance), and
 *   ((2 mu_a mu_b + C1)(2 s_ab + C2)) / ((mu_a^2 + mu_b^2 + C1)(s_a^2 + s_b^2 + C2)), C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2; the result
 *   is the mean over positions and channels.  All fp64, products and sums separate (no contraction).
 * Determinism: *partials partials per image, reduced in a fixed order, no atomics; an image's results have the same bits alone or in any
 *   batch.
 * pub_config: *partials = partials per image of the two passes, *tile = side of the SSIM kernel's tile of valid positions.
 * pub_sse:  partial uint64 [n][*partials][2] = {sum of the low 32 bits, sum of the remaining high bits} of the squared differences.
 * pub_ssim: partial double [n][*partials] = sums of the SSIM value over positions and channels.
 * pub_finish: out = double [3][n], rows mse, psnr, ssim, from the two partial arrays in one launch. */
int srhip_pub_config(int* partials, int* tile);
int srhip_pub_sse(const void* a, const void* b, unsigned long long* partial, int n, int h, int w, int c, int crop, int luma, int is_float,
                  void* stream);
int srhip_pub_ssim(const void* a, const void* b, double* partial, int n, int h, int w, int c, int crop, int luma, int is_float,
                   void* stream);
int srhip_pub_finish(const unsigned long long* sse_partial, const double* ssim_partial, double* out, int n, int h, int w, int c, int crop,
                     int luma, void* stream);

/* ---- LPIPS, the fourth validation metric (sradsgan.py:561 `PerceptualLoss('net-lin', 'alex')`, called per image at :1125-1132 and
 *      :1326-1332; utils/PerceptualSimilarity/__init__.py:26-44, networks_basic.py:64-105, pretrained_networks.py:57-96).  The forward passes:
 * lpips_stem: the scaling layer and AlexNet features[0:2] in one pass.  x [m][h][w][3] in [0,1] (normalize != 0: x = 2x - 1 first,
 *   __init__.py:36-38) -> (x - shift) / scale per channel (networks_basic.py:101-105) on in-image taps only -- the conv pads with zeros
 *   in the scaled space -- then conv 3->64 k11 s4 p2 + bias + ReLU in exact fp32 in every conv-math mode.
 *   w_hwio: the weight as [11][11][3][64] (ky, kx, ci, co); y [m][ho][wo][64], ho = (h + 4 - 11) / 4 + 1.  Needs h, w >= 7.
 * maxpool3x3s2_fwd: nn.MaxPool2d(3, 2) of features[2] / [5]: floor mode, no padding, ho = (h - 3) / 2 + 1; C % 4 == 0, h, w >= 3.
 * lpips_head: one tap.  f [m][h][w][c] holds the features of all images; pairs = int32 [npairs][2] on the device, indices into m
 *   (the caller checks them); w [c] = the tap's lin weights.  Per pixel: f / (sqrt(sum_c f^2) + 1e-10) for both images, then
 *   sum_c w[c] * (difference)^2 (networks_basic.py:70-78, __init__.py:42-44).  partial: double [npairs][srhip_lpips_blocks()] pixel
 *   sums, fixed reduction order, no atomics.  C % 4 == 0.
 * lpips_finish: partial = double [ntaps][npairs][srhip_lpips_blocks()], tap_pixels = host array of h * w per tap (read during the
 *   call) -> out[npairs] = sum over taps of (pixel sum / pixels): spatial_average and the sum of the layers (:83-87).               */
int srhip_lpips_stem(const float* x, const float* w_hwio, const float* bias, float* y, int m, int h, int w, int normalize, void* stream);
int srhip_maxpool3x3s2_fwd(const float* x, float* y, int n, int h, int w, int c, void* stream);
int srhip_lpips_blocks(void);
int srhip_lpips_head(const float* f, const int* pairs, const float* w, double* partial, int m, int npairs, int h, int wd, int c,
                     void* stream);
int srhip_lpips_finish(const double* partial, const long* tap_pixels, int ntaps, int npairs, double* out, void* stream);
/* Additive, ABI stays 14 -- LPIPS as a loss (lpips.LPIPS.loss): the three backward passes that the conv kernels do not cover.  Exact
 * fp32 in every conv-math mode, no atomics, one fixed summation order per value, nothing that crosses images.  (The version number
 * does not move, as for the forward passes: the binding resolves every declared symbol when it loads the library.)
 * lpips_head_bwd: one tap's gradient with respect to the PRED features -- pairs[p] = (target index, pred index) into m -- already
 *   passed back through that tap's ReLU; df [npairs][h][w][c].  Per pixel, f = pred, t = target, n = sqrt(sum f^2), D = n + 1e-10,
 *   e_c = f_c / D - t_c / D_t, q_c = 2 w_c e_c s, S = sum_c q_c f_c, df_c = q_c / D - f_c S / (D^2 n); s = upstream[0] * inv_count
 *   with upstream a device scalar (no host sync) and inv_count = 1 / (N h w).  f_c <= 0 writes 0, so a NaN feature passes its NaN on
 *   like ATen's threshold_backward.  A pixel with n == 0 writes zeros and never forms 0 / 0: every channel is masked there anyway;
 *   torch autograd yields NaN at such a pixel, and the departure is deliberate.  C % 4 == 0.
 * maxpool3x3s2_bwd: backward of nn.MaxPool2d(3, 2) in gather form, fused with what follows it: dx = gather(dy) * [x > 0] + residual.
 *   x [n][h][w][c] is the pool's input; each input pixel recomputes the arg-max of the at most 2 x 2 windows that hold it in the
 *   forward's scan order (the first maximum wins) and adds their dy in ascending (oy, ox) order.  relu != 0 applies the mask of x (a
 *   ReLU output; x <= 0 writes 0); residual may be NULL.
 * lpips_stem_bwd: the stem's data gradient to the image, scaling layer included: g [m][ho][wo][64] is the gradient at the stem conv's
 *   output (ReLU mask applied), dx [m][h][w][3] = (normalize ? 2 : 1) / scale[ch] * conv_transpose(g, w).  Gather form: at most 3 x 3
 *   output positions x 64 channels, one fmaf chain per value with (oy, ox, co) ascending.                                          */
int srhip_lpips_head_bwd(const float* f, const int* pairs, const float* w, const float* upstream, float inv_count, float* df, int m,
                         int npairs, int h, int wd, int c, void* stream);
int srhip_maxpool3x3s2_bwd(const float* x, const float* dy, const float* residual, float* dx, int n, int h, int w, int c, int relu,
                           void* stream);
int srhip_lpips_stem_bwd(const float* g, const float* w_hwio, float* dx, int m, int h, int w, int normalize, void* stream);

/* Additive, ABI stays 14 -- the contrastive VGG19 losses (contrast.py; reference model/loss.py:121-298).  All tensors channels-last
 * fp32; exact fp32 elementwise work, float64 reductions in one fixed order per value, no atomics, nothing that crosses samples in the
 * cosine passes.  A tap `f` holds the features of the stacked batch [a; p; n_1 .. n_N]: (1 + kops) * b images of [h][w][c], kops =
 * 1 + N <= 9 operands; operand k of sample s is image (k + 1) * b + s.  C % 4 == 0.
 * maxpool2x2_floor_fwd / _bwd: nn.MaxPool2d(2) for any h, w >= 2: ho = h / 2, wo = w / 2, an odd last row or column belongs to no window
 *   and gets no gradient; the first maximum of a window wins.  bwd, gather form: dx = gather(dy) [* (x > 0) when relu != 0] [+ residual],
 *   x [n][h][w][c] the pool's input, residual may be NULL (the contract of srhip_maxpool3x3s2_bwd).
 * contrast_l1_fwd: partial = double [kops][srhip_contrast_l1_parts()], the sums of |a - x_k| over the tap, every entry written.
 * contrast_l1_bwd: da [b][h][w][c] = upstream[0] * (coef[0] * sign(a - x_0) - sum_{k >= 1} coef[k] * sign(a - x_k)), sign(0) = 0, 0 where
 *   a <= 0 (the tap's ReLU).  coef = double [kops] and upstream = float [1], both on the device.
 * contrast_l1_finish: partial = double [5][kops][parts] of the five taps, tap_counts = host array of the 5 element counts b * h * w * c
 *   (read during the call), kops >= 2 -> loss[0] = sum_t weight_t * d_ap / (d_an + 1e-7) (ablation != 0: weight_t * d_ap), d_an summed
 *   over the negatives, weights 1/32 1/16 1/8 1/4 1, and coef = double [5][kops], the (alpha, beta ..) of each tap's backward.
 * contrast_cos_fwd: per pixel cos_k = (a . x_k) / (max(|a|, 1e-8) max(|x_k|, 1e-8)); partial = double [b][kops][srhip_contrast_cos_parts()],
 *   the pixel sums of cos_k per sample.
 * contrast_cos_bwd: da = upstream[0] / (h w) * sum_k gamma[s][k] * d cos_k / d a, 0 where a <= 0; gamma = double [b][kops] on the device.
 *   d cos / d a_c = x_c / (mx ma) - [|a| > 1e-8] cos a_c / (ma |a|): a zero-norm pixel forms no 0 / 0.
 * contrast_cos_finish: partial = double [5][b][kops][parts], tap_counts = host array of the 5 h * w.  With E_k = exp(mean cos_k / 0.07):
 *   form 0 (kops == 2): term = -log(E_0 / (E_1 + 1e-7)), ablation != 0: -log(E_0); form 1: term = -log(E_0 / (sum_{k>=1} E_k + E_0)).
 *   loss[0] = mean_s sum_t weight_t term; gamma = double [5][b][kops] = weight_t / b * d term / d mean_k; terms = double [5 * b] scratch. */
int srhip_maxpool2x2_floor_fwd(const float* x, float* y, int n, int h, int w, int c, void* stream);
int srhip_maxpool2x2_floor_bwd(const float* x, const float* dy, const float* residual, float* dx, int n, int h, int w, int c, int relu,
                               void* stream);
int srhip_contrast_l1_parts(void);
int srhip_contrast_cos_parts(void);
int srhip_contrast_l1_fwd(const float* f, double* partial, int b, int kops, int h, int w, int c, void* stream);
int srhip_contrast_l1_bwd(const float* f, const double* coef, const float* upstream, float* da, int b, int kops, int h, int w, int c,
                          void* stream);
int srhip_contrast_l1_finish(const double* partial, const long* tap_counts, int kops, int ablation, float* loss, double* coef,
                             void* stream);
int srhip_contrast_cos_fwd(const float* f, double* partial, int b, int kops, int h, int w, int c, void* stream);
int srhip_contrast_cos_bwd(const float* f, const double* gamma, const float* upstream, float* da, int b, int kops, int h, int w, int c,
                           void* stream);
int srhip_contrast_cos_finish(const double* partial, const long* tap_counts, int b, int kops, int form, int ablation, float* loss,
                              double* gamma, double* terms, void* stream);

/* ---- torch.optim.Adam (sradsgan.py:724-725, step at :858 and :887) over a flat fp32 arena, fused
 *      with the discriminator's weight clip `p.data.clamp_(-c, c)` (:891-892; clip <= 0: none).
 * p,g,m,v: [n] arenas (n % 4 == 0, 16-byte aligned); g is multiplied by grad_scale first (1/world
 * for the data-parallel mean).  state: float[4] on the device {step, lr/(1-b1^step),
 * sqrt(1-b2^step), -}; the call advances it on the device, so it is hipGraph-capturable.
 * Arithmetic order follows torch.optim.Adam (eps added after sqrt(v)/sqrt(bias_correction2)).
 * The clip is torch's clamp_, which keeps a NaN: a NaN gradient leaves m, v and p of that element
 * NaN; a +inf gradient leaves m = v = +inf and p = NaN (inf / inf), the next finite gradient turns
 * m NaN too and v stays +inf; a NaN weight stays NaN.  All with or without the clip, as
 * torch.optim.Adam + clamp_ does; the float4 lane-mates of such an element are unaffected.        */
int srhip_adam_step(float* p, const float* g, float* m, float* v, float* state, long n, float lr, float b1,
                    float b2, float eps, float grad_scale, float clip, void* stream);

/* ---- input pipeline ------------------------------------------------------ *
 * Pillow-compatible resampling of uint8 NHWC tiles, replacing the per-sample PIL calls of
 * RGB_TrainDatasetFromFolder.__getitem__ (data/dataset.py:428 lr = resize(img, BICUBIC), :435 bc = resize(lr, BICUBIC))
 * and the test-time Resize (data/data.py:331, BILINEAR).  Bit-exact with Image.resize for 8-bit images
 * (Pillow Resample.c arithmetic: 22-bit fixed-point weights, clip after each pass, horizontal pass first).
 * srhip_resample_ksize / srhip_resample_coeffs are host-only (weights per output coordinate, computed in double);
 * srhip_resample_pass_u8 runs one pass (axis 1: width, axis 0: height) with device copies of bounds/coeffs;
 * srhip_u8_to_float is torchvision's to_tensor scaling (value / 255 in fp32).                    */
#define SRHIP_FILTER_BILINEAR 2
#define SRHIP_FILTER_BICUBIC 3
int srhip_resample_ksize(int in_size, int out_size, int filter);
int srhip_resample_coeffs(int in_size, int out_size, int filter, int* bounds, int* coeffs);
int srhip_resample_pass_u8(const unsigned char* src, unsigned char* dst, const int* bounds_dev, const int* coeffs_dev,
                           int ksize, int n, int h, int w, int c, int axis, int out_size, void* stream);
int srhip_u8_to_float(const unsigned char* src, float* dst, long count, void* stream);

/* ---- whole-scene super-resolution in overlapping tiles (sradsgan_amd/scene.py; additive, ABI stays 14) ---------- *
 * srhip_scene_tiles_u8: scene = uint8 [h][w][3] on the device, origins_dev = int [n][2] (y, x) on the device, every tile
 *   th x tw inside the scene (an origin outside it yields a zero tile, never an out-of-bounds read).  dst = float
 *   [n][th][tw][3], value / 255: tile k holds the bits srhip_u8_to_float gives for scene[y:y+th, x:x+tw].
 * srhip_scene_blend_u8: feathered blend of float SR tiles into HR rows [row0, row1) of the scene, gather form.
 *   Tiles form an ny x nx grid; tile (j, i) covers HR rows ay[j] .. ay[j]+th-1 and columns ax[i] .. ax[i]+tw-1 (th, tw in
 *   HR pixels here) and is read at tiles_dev[(j % depth) * nx + i] + c*sc + qy*sy + qx*sx (element strides, any memory
 *   format; a null entry is skipped).  ycover_dev [hr_h][2] / xcover_dev [hr_w][2] hold, per HR row / column, the first
 *   and one-past-last tile row / column covering it; wy_dev [ny][th], wx_dev [nx][tw] are the 1-D feather tables.  Per
 *   pixel, in fp32 and in row-major tile order (no atomics, so the result is deterministic):
 *       w = wy * wx;  acc += w * v;  wsum += w;  out = acc / wsum
 *   (a pixel one tile covers alone has w = 1 and returns the tile's value, -0 as +0).  out_f32 (float [hr_h][hr_w][3],
 *   may be null) receives out; out_u8 (uint8 [hr_h][hr_w][3], 4-byte aligned, may be null) receives save_img1's
 *   quantisation (utils/utils.py:169-187) trunc(clamp(255 out, 0, 255)), NaN written as 0.  Whole dwords are stored
 *   (4 pixels = 12 bytes per thread) with scalar row heads and tails.                                            */
int srhip_scene_tiles_u8(const unsigned char* scene, int h, int w, const int* origins_dev, int n, int th, int tw, float* dst,
                         void* stream);
int srhip_scene_blend_u8(const float* const* tiles_dev, int depth, long sc, long sy, long sx, const int* ycover_dev,
                         const int* xcover_dev, const int* ay_dev, const int* ax_dev, const float* wy_dev, const float* wx_dev,
                         int ny, int nx, int th, int tw, int hr_h, int hr_w, int row0, int row1, unsigned char* out_u8,
                         float* out_f32, void* stream);

/* ---- spectral normalisation of the patch discriminator's conv weights (base_networks.py:73-131; additive, ABI 14) ---- *
 * All spectral layers of ONE discriminator pass per call.  Per layer, Wb = weight_bar as [cout][k] (k = cin kh kw, OIHW):
 *     t = Wb^T u, v <- t / (|t| + 1e-12);  s = Wb v, u <- s / (|s| + 1e-12);  sigma = <u, s>;  W = Wb / sigma
 * u and v are overwritten in place; (u, v, sigma) of the pass are also left in the pass buffer for its backward:
 *     Gb += G / sigma - (<G, Wb> / sigma^2) u v^T          (G: gradient with respect to W, Gb: weight_bar's gradient slot)
 * entries_dev: device array of
 *     struct { const float* wbar; float* u; float* v; long off_sigma, off_weff, off_u, off_v, off_tpart, off_s, off_dpart;
 *              int cout, k; }                               (srhip_sn_entry_bytes() bytes each)
 * The table holds the parameters' addresses and OFFSETS for what a pass writes, so one table serves every pass: off_sigma [1],
 * off_weff [cout k], off_u [cout], off_v [k], off_s [cout] (scratch) and off_tpart (scratch, srhip_sn_tpart_elems(cout, k) floats, an
 * EVEN offset) count floats from `out`, the pass buffer (8-byte aligned, fresh per pass: it lives until the pass's backward);
 * off_dpart counts doubles from the backward's `workspace` (srhip_sn_dot_parts(cout, k) doubles per layer).  Regions must not overlap.
 * grads / gbars: HOST arrays of `count` device addresses (they change per call and travel as kernel arguments): a null grads[i]
 * skips layer i.  max_cout / max_k: the largest cout and k of the table (they size the grid only).
 * fp32 operands, sums carried in fp64 and rounded once, whatever the conv arithmetic mode; two-stage reductions in a fixed order,
 * no atomics; a layer's results depend neither on the other layers of the table nor on the grid.  Any cout >= 1, k >= 1.
 * Forward: 4 launches, backward: 2 per 32 layers, whatever `count` (<= 65535).                                              */
int srhip_sn_entry_bytes(void);
long srhip_sn_tpart_elems(int cout, int k);
long srhip_sn_dot_parts(int cout, int k);
int srhip_sn_forward_batched(const void* entries_dev, int count, float* out, int max_cout, int max_k, void* stream);
int srhip_sn_backward_batched(const void* entries_dev, int count, const float* out, const void* const* grads, void* const* gbars,
                              void* workspace, int max_cout, int max_k, void* stream);

/* ---- scene-classification evaluation of SR outputs (sradsgan_amd/classify.py, Scene_classification_mfe.py; additive, ABI 14) ---- *
 * srhip_cls_channel_sums: img = uint8 [n][h][w][c] (c <= 4) -> sums = int64 [n][c], the per-image per-channel sums of the raw
 *   bytes.  Integer arithmetic in two stages (workspace: srhip_cls_channel_sums_workspace bytes, 8-byte aligned): exact.
 * srhip_cls_preprocess: out[i] = ((float)img[i] - means_dev[i % c]) * (float)(1 / 255.), fp32, one rounding per operation.
 * The dense layer y[m][n] = x[m][k] w[k][n] + bias[n], 1 <= m <= 64 rows per call, row-major operands, exact fp32 whatever
 *   srhip_set_conv_math says, no atomics, reproducible bit for bit:
 *   srhip_cls_dense_fwd: k % 8 == 0, x 16-byte aligned.  Split-K: srhip_cls_dense_chunks(k) slabs of [m][n] partial sums in
 *     `partials` (a second launch adds them in chunk order), then + bias (may be null), ReLU when relu != 0, dropout when
 *     dropout != 0: keep(seed, step, e = row * n + col) = first word of Philox4x32-10 with counter {e lo, e hi, step lo, step hi}
 *     and key {seed lo, seed hi} < 2^31; kept values are doubled, dropped ones are 0.
 *   srhip_cls_dense_wgrad: dw[k][n] = sum over rows of x[r][k] dy[r][n] in row order; db[n] = sum over rows of dy (db may be null).
 *   srhip_cls_dense_dgrad: dx[m][k] = dy[m][n] w[k][n]^T in column order, then the backward of the layer that produced the [m][k]
 *     activation `act`: x2 / 0 by the recomputed dropout mask (dropout != 0), 0 where act <= 0 (relu != 0).
 * srhip_cls_softmax_ce_fwd_bwd: logits [m][c], c <= 64, labels int32 [m] -> row_loss[r] = -log_softmax(logits[r])[label] in fp32
 *   (max-subtracted, no clipping; 0 for a label outside [0, c)), loss_sum[0] = their sum in fp64 in a fixed order, and, unless
 *   dlogits is null, dlogits = (softmax - onehot) * scale.
 * srhip_cls_confusion: arg[r] = the first index of the row's maximum -> pred[r] (may be null) and ++table[labels[r]][arg[r]]
 *   (int32 [c][c], may be null; the caller zeroes it, so several calls accumulate; labels outside [0, c) are not counted).
 *   A NaN logit counts as the row's maximum (the first one wins), as in torch.argmax; srhip_cls_softmax_ce_fwd_bwd gives such a
 *   row a NaN loss, NaN dlogits and a NaN loss_sum.                                                                             */
size_t srhip_cls_channel_sums_workspace(int n, int h, int w);
int srhip_cls_channel_sums(const unsigned char* img, long long* sums, void* workspace, size_t workspace_bytes, int n, int h, int w,
                           int c, void* stream);
int srhip_cls_preprocess(const unsigned char* img, const float* means_dev, float* out, long count, int c, void* stream);
int srhip_cls_dense_chunks(int k);
int srhip_cls_dense_fwd(const float* x, const float* w, const float* bias, float* y, float* partials, size_t partial_bytes, int m,
                        int k, int n, int relu, int dropout, unsigned long long seed, unsigned long long step, void* stream);
int srhip_cls_dense_wgrad(const float* x, const float* dy, float* dw, float* db, int m, int k, int n, void* stream);
int srhip_cls_dense_dgrad(const float* dy, const float* w, const float* act, float* dx, int m, int k, int n, int relu, int dropout,
                          unsigned long long seed, unsigned long long step, void* stream);
int srhip_cls_softmax_ce_fwd_bwd(const float* logits, const int* labels, float* row_loss, double* loss_sum, float* dlogits, int m,
                                 int c, float scale, void* stream);
int srhip_cls_confusion(const float* logits, const int* labels, int* pred, int* table, int m, int c, void* stream);

/* ABI 14 (additive) -- forward kernels of the diffusion sampler (csrc/diffusion.hip; model/gdp.py).  Exact fp32 whatever
 * srhip_set_conv_math says, no atomics (re-runs are bit-identical), NHWC rows with a row stride where noted.
 *   srhip_diff_gn_fwd: nn.GroupNorm(32, C) (biased variance, per-channel affine) over x [n][p][C] read with row stride ldx, C % 32 == 0,
 *     C <= 2048; then, if scale / shift (both or neither; [n][C] with row stride ldmod) are given, y = y * (1 + scale) + shift; then SiLU
 *     if silu != 0.  A sample's statistics read that sample only (two fixed-order stages).  Workspace: srhip_diff_gn_workspace(n, p).
 *   srhip_diff_silu_fwd: y = x * sigmoid(x) over `count` elements (the time-embedding rows).
 *   srhip_diff_avgpool2x2_fwd: nn.AvgPool2d(2) on [n][h][w][c] -> [n][h/2][w/2][c], ((a + b) + c + d) * 0.25 in window scan order; odd h
 *     or w is an argument error.
 *   srhip_diff_attn_fwd: QKVAttentionLegacy.  qkv [n][t][heads * 3 * ch] with each head's q | k | v as three adjacent runs of ch
 *     channels; out [n][t][heads * ch] = softmax((q s)(k s)^T) v with s = ch^(-1/4), soft-max in fp32, flash style (no t x t tensor).
 *     ch is 32 or 64, t is arbitrary, tensors 16-byte aligned.
 *   srhip_diff_randn: standard normals from Philox4x32-10, key = seed, counter = {element / 4, step}, element = row * ch + channel,
 *     Box-Muller on the four words; written with row stride ldo.  The bits do not depend on the launch shape.
 *   srhip_diff_sampler_step: out = c1 * clamp(x0, -1, 1) + c2 * xt + (t_nonzero ? exp(0.5 * logvar) * noise : 0) over rows x ch, every
 *     tensor with its own row stride; out may be xt.  noise == NULL draws srhip_diff_randn(seed, step)'s values in the kernel.
 *     The clamp is torch's clamp_: x0 = +-inf counts as +-1, a NaN in x0 (or xt, or noise) stays NaN in out at that element only.
 *   srhip_diff_quant_u8: out[rows][ch] = uint8(rint((clamp(x, lo, hi) - lo) / (hi - lo) * 255)), round half to even.  A byte cannot
 *     carry a NaN: a NaN element is written as byte 0.                                                                                */
size_t srhip_diff_gn_workspace(long n, long p);
int srhip_diff_gn_fwd(const float* x, long ldx, const float* gamma, const float* beta, const float* scale, const float* shift, long ldmod,
                      float* y, long ldy, void* workspace, size_t workspace_bytes, long n, long p, int c, float eps, int silu,
                      void* stream);
int srhip_diff_silu_fwd(const float* x, float* y, long count, void* stream);
int srhip_diff_avgpool2x2_fwd(const float* x, float* y, int n, int h, int w, int c, void* stream);
int srhip_diff_attn_fwd(const float* qkv, float* out, int n, int t, int heads, int ch, void* stream);
int srhip_diff_randn(float* out, long ldo, long rows, int ch, unsigned long long seed, unsigned long long step, void* stream);
int srhip_diff_sampler_step(const float* x0, long ldx0, const float* xt, long ldxt, const float* noise, long ldn, float* out, long ldo,
                            long rows, int ch, float c1, float c2, float logvar, int t_nonzero, unsigned long long seed,
                            unsigned long long step, void* stream);
int srhip_diff_quant_u8(const float* x, long ldx, unsigned char* out, long rows, int ch, float lo, float hi, void* stream);

/* ABI 14 (additive) -- backward kernels of the diffusion U-Net and the forward diffusion (csrc/diffusion.hip; model/gdp_train.py).  Same
 * contract: exact fp32, no atomics, fixed summation orders (re-runs are bit-identical), row strides where noted.
 *   srhip_diff_gn_stats_offset: byte offset, inside the workspace srhip_diff_gn_fwd was given, of the statistics it leaves there:
 *     float [n][32][2] = {mean, 1 / sqrt(var + eps)} per (sample, group).  The backward reads them; it does not recompute them.
 *   srhip_diff_gn_bwd: backward of srhip_diff_gn_fwd from dy [n][p][C] (row stride lddy), x (ldx) and those statistics.  With
 *     xh = (x - mean) rstd, z = (xh gamma + beta)(1 + scale) + shift, dz = dy silu'(z) (dz = dy when silu == 0), g = dz (1 + scale) gamma:
 *     dx = rstd (g - mean_grp(g) - xh mean_grp(g xh)) (row stride lddx), dgamma[C], dbeta[C], and, with scale / shift, dscale / dshift
 *     [n][C] (row stride lddmod; NULL exactly when scale is NULL).  A sample's dx / dscale / dshift read that sample only.  Workspace:
 *     srhip_diff_gn_bwd_workspace(n, p, C).
 *   srhip_diff_silu_bwd: dx = dy * sigmoid(x) (1 + x (1 - sigmoid(x))).
 *   srhip_diff_avgpool2x2_bwd: dx [n][h][w][c] = 0.25 * dy [n][h/2][w/2][c] over each window; odd h or w is an argument error.
 *   srhip_diff_attn_fwd_lse: srhip_diff_attn_fwd (the same kernel body, `out` bit-identical) that also writes
 *     lse [n][heads][t] = running maximum + log(running sum) of each query's soft-max row.
 *   srhip_diff_attn_bwd: dqkv [n][t][heads * 3 * ch] (q | k | v layout of qkv) from dout [n][t][heads * ch], qkv, out and lse, flash
 *     style on v_mfma_f32_32x32x2_f32: one kernel owns 32 queries per wave (dq, and delta = rowsum(dout * out) into the workspace), one
 *     owns 32 keys per wave (dk, dv).  No t x t tensor.  Workspace: srhip_diff_attn_bwd_workspace(n, t, heads).
 *   srhip_diff_q_sample: out = sqrt_ac[t_b] * x0 + sqrt_1mac[t_b] * eps over n samples of rows_per_sample rows x ch, every tensor with its
 *     own row stride; t is int64 [n] ON THE DEVICE, the two schedule arrays are device float [steps] (a t outside [0, steps) is clamped);
 *     eps = noise, or with noise == NULL srhip_diff_randn(seed, step)'s values over the same [n * rows_per_sample][ch] elements.        */
size_t srhip_diff_gn_stats_offset(long n, long p);
size_t srhip_diff_gn_bwd_workspace(long n, long p, int c);
int srhip_diff_gn_bwd(const float* dy, long lddy, const float* x, long ldx, const float* stats, const float* gamma, const float* beta,
                      const float* scale, const float* shift, long ldmod, float* dx, long lddx, float* dgamma, float* dbeta, float* dscale,
                      float* dshift, long lddmod, void* workspace, size_t workspace_bytes, long n, long p, int c, int silu, void* stream);
int srhip_diff_silu_bwd(const float* dy, const float* x, float* dx, long count, void* stream);
int srhip_diff_avgpool2x2_bwd(const float* dy, float* dx, int n, int h, int w, int c, void* stream);
int srhip_diff_attn_fwd_lse(const float* qkv, float* out, float* lse, int n, int t, int heads, int ch, void* stream);
size_t srhip_diff_attn_bwd_workspace(int n, int t, int heads);
int srhip_diff_attn_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, void* workspace,
                        size_t workspace_bytes, int n, int t, int heads, int ch, void* stream);
int srhip_diff_q_sample(const float* x0, long ldx0, const float* noise, long ldn, float* out, long ldo, const long long* t,
                        const float* sqrt_ac, const float* sqrt_1mac, int steps, long n, long rows_per_sample, int ch,
                        unsigned long long seed, unsigned long long step, void* stream);

/* ABI 14 (additive) -- the dihedral group on image batches (csrc/augment.hip; data.Augment, ensemble.py).  Exact permutations, no
 * atomics, re-runs are bit-identical.
 * Op encoding, the same in every call: op in 0..7, bit 0 = transpose (swap H and W), bit 1 = flip top-bottom, bit 2 = flip
 *   left-right, applied in that order: y = fliplr^b2(flipud^b1(transpose^b0(x))).
 *   srhip_augment_u8: in = uint8 [n][h][w][c] (c <= 4), params_dev = DEVICE int [n][4] = {y0, x0, op, 0}, out = uint8 [n][cs][cs][c],
 *     4-byte aligned.  Sample k of out is op_k applied to the cs x cs crop of sample k at (y0_k, x0_k); a crop that leaves the source
 *     or an op outside 0..7 (the device table cannot be checked on the host) yields a zero tile, never an out-of-bounds read.
 *     With sigma > 0, Gaussian noise is added to the crop BEFORE the op, in double: byte' = trunc(clip((double)byte + sigma * z, 0, 255))
 *     (numpy's clip(..).astype(uint8)), z = the fp32 tensor z [n][cs][cs][c] indexed in the un-rotated crop, or, with z == NULL and
 *     drawn != 0, the value srhip_diff_randn(seed, step) writes for element ((k * cs + y) * cs + x) * c + ch.  sigma == 0 launches
 *     the kernel without any noise code.  Whole dwords are stored, with scalar row heads and tails.
 *   srhip_dihedral_f32: y = op(x) for a float tensor, logically x [n][c][h][w] and y [n][c][oh][ow] ((oh, ow) = (w, h) for a
 *     transposing op), each given by four element strides {n, c, h, w} read on the HOST -- NCHW-dense and channels-last alike.
 *     float4 per thread when c % 4 == 0, both channel strides are 1 and both sides are 16-byte aligned; scalar otherwise.
 *   srhip_ensemble_merge_f32: views = HOST array of m <= 8 device pointers, view_strides = HOST long [m][4], ops = HOST int [m];
 *     view k has the shape of op_k(out).  out[n][c][y][x] = (((v_0 + v_1) + v_2) + ... + v_{m-1}) * (1.0f / m) in fp32, in index
 *     order, v_k read where op_k sends (y, x) (i.e. through the inverse of op_k); one pass, no workspace.                        */
int srhip_augment_u8(const unsigned char* in, const int* params_dev, const float* z, unsigned char* out, int n, int h, int w, int c,
                     int cs, double sigma, int drawn, unsigned long long seed, unsigned long long step, void* stream);
int srhip_dihedral_f32(const float* x, const long* x_strides, float* y, const long* y_strides, int n, int c, int h, int w, int op,
                       void* stream);
int srhip_ensemble_merge_f32(const float* const* views, const long* view_strides, const int* ops, int m, float* out,
                             const long* out_strides, int n, int c, int h, int w, void* stream);

/* ABI 14 (additive) -- the blur-and-noise degradation of training batches (csrc/degrade.hip; sradsgan_amd/degrade.py; model/util.py:
 * BatchBlur, b_GaussianNoising).  No atomics, re-runs are bit-identical, and no byte depends on the batch size or on a sample's place
 * in the batch.  Argument errors return SRHIP_ERR_ARG before any launch.
 *   srhip_blur_u8: in / out = uint8 [n][h][w][c] (c <= 4), kernels_dev = DEVICE float [n][l][l], l = 1..21 (even l allowed): sample k
 *     cross-correlated with kernel k, every channel alike, on the image padded like nn.ReflectionPad2d (edge not repeated: i < 0 ->
 *     -i, i >= H -> 2 (H - 1) - i) by lo = l / 2 before and hi = l / 2 (l odd) or l / 2 - 1 (l even) after; lo >= h or lo >= w is an
 *     argument error.  The arithmetic is fixed: x = (float)byte / 255.0f; acc = 0.0f; for i = 0..l-1, inside it j = 0..l-1:
 *     acc = acc + k[i][j] * xpad[y + i][x + j], product and sum each rounded to fp32 (no fma, one chain per output); the byte is
 *     (unsigned char)(int)(acc * 255.0f) -- to_pil_image's mul(255).byte(), a truncation.  Whole dwords are stored, with scalar
 *     heads and tails per row.
 *   srhip_blur_f32: the same sum without the quantisation on a float tensor, logically x / y [n][c][h][w], each given by four
 *     element strides {n, c, h, w} read on the HOST (NCHW-dense and channels-last alike).  per_sample = 0: one shared kernel [l][l]
 *     (BatchBlur's 2-D branch), otherwise [n][l][l].  A NaN input reaches exactly the outputs whose l x l footprint holds it.
 *   srhip_degrade_noise_u8: out = float [n][h][w][c] = min(max(x + z * level[k], 0), 1) with x = (float)byte / 255.0f, product and
 *     sum rounded separately, level = DEVICE float [n]; z = a float tensor of out's shape or, with z == NULL and drawn != 0, the value
 *     srhip_diff_randn(seed, step) writes for element ((k * h + y) * w + x) * c + ch.  level[k] == 0 gives srhip_u8_to_float's bits
 *     for sample k.  A NaN (from a supplied z or a level) stays a NaN, as in torch.clamp.                                          */
int srhip_blur_u8(const unsigned char* in, const float* kernels_dev, unsigned char* out, int n, int h, int w, int c, int l, void* stream);
int srhip_blur_f32(const float* x, const long* x_strides, const float* kernels_dev, int per_sample, float* y, const long* y_strides, int n,
                   int c, int h, int w, int l, void* stream);
int srhip_degrade_noise_u8(const unsigned char* lr, const float* level_dev, const float* z, float* out, int n, int h, int w, int c,
                           int drawn, unsigned long long seed, unsigned long long step, void* stream);

/* ABI 14 (additive) -- ESRGAN (csrc/esrgan.hip; sradsgan_amd/model/esrgan.py; model/architecture.py, model/sradsgan.py:35-67, :840-878).
 * Exact fp32 / fp64 arithmetic that ignores srhip_set_conv_math, no atomics, fixed summation orders: re-runs are bit-identical.
 * Argument errors return SRHIP_ERR_ARG before any launch.
 *   srhip_gan_loss_fwd_bwd: GANLoss('vanilla' | 'lsgan') against a filled label, mean-reduced, plain or relativistic.  With
 *     m = relativistic ? mean(b[0 .. count_b)) : 0 and x_i = a[i] - m it forms mean_i f(x_i, label), f = BCE-with-logits in the stable
 *     form max(x, 0) - x label + log1p(exp(-|x|)) (mode SRHIP_GAN_VANILLA) or (x - label)^2 (SRHIP_GAN_LS).  The mean of b, x_i, f and
 *     every sum are float64, summed by one 256-thread block (thread t takes i = t, t + 256, .. in order, then a binary tree over t).
 *     out != NULL: the value, a 0-d float.  gout != NULL (a device scalar, the upstream gradient): da != NULL receives
 *     gout f'(x_i) / count, db != NULL (relativistic only) the gradient through the mean, -gout sum_i f'(x_i) / (count count_b) in
 *     every element.  One call may ask for the value, the gradients or both.  A NaN logit gives a NaN value (no fmax), logits of
 *     +-100 give finite values and gradients.  1 <= count, count_b <= 2^22 (a patch discriminator's B h w).
 *   srhip_dhead_fwd / _bwd: the dense head of Discriminator_VGG_*: y[b] = b1 + sum_j w1[j] hidden[b][j], hidden = LeakyReLU(b0[j] +
 *     sum_k w0[j][k] xflat[b][k]) where xflat is the reference's x.view(B, -1) of an NCHW tensor, k = c S S + p.  x is the NHWC
 *     activation [B][S][S][C] and w0 the [H][C S S] weight as stored: the kernel's addressing resolves the order (element k meets
 *     x[b][p][c]); no transposed copy and no cached image of either exists.  Summation order of hidden: thread t of 256 runs one fmaf
 *     chain over the float4 groups t, t + 256, .. of the weight row in ascending k, the 256 chains are added as a binary tree over t,
 *     the bias is added last; y likewise over j.  The backward takes the LeakyReLU mask from the stored hidden activation (slope > 0)
 *     and writes dz [B][H] (scratch: the gradient at the first linear's output), dx [B][S][S][C] (NULL: skipped) and dw0, db0, dw1,
 *     db1 (all four or all NULL), each one fmaf chain per element over ascending b (dx: ascending j).  C % 4 == 0, w0 / dw0 16-byte
 *     aligned.
 *   srhip_input_norm_fwd / _bwd: VGGFeatureExtractor's (x - mean[c]) / std[c] on an NHWC image (element e has channel e % c, c <= 4,
 *     mean / std DEVICE floats [c]) with IEEE subtraction and division, and its backward dx = dy / std[c].                          */
#define SRHIP_GAN_VANILLA 0
#define SRHIP_GAN_LS 1
int srhip_gan_loss_fwd_bwd(const float* a, long count, const float* b, long count_b, int mode, float label, int relativistic,
                           const float* gout, float* out, float* da, float* db, void* stream);
int srhip_dhead_fwd(const float* x, const float* w0, const float* b0, const float* w1, const float* b1, float* hidden, float* y, int B,
                    int C, int S, int H, float slope, void* stream);
int srhip_dhead_bwd(const float* dy, const float* x, const float* hidden, const float* w0, const float* w1, float* dz, float* dx,
                    float* dw0, float* db0, float* dw1, float* db1, int B, int C, int S, int H, float slope, void* stream);
int srhip_input_norm_fwd(const float* x, const float* mean, const float* stdv, float* y, long count, int c, void* stream);
int srhip_input_norm_bwd(const float* dy, const float* stdv, float* dx, long count, int c, void* stream);

#ifdef __cplusplus
}
#endif
#endif
