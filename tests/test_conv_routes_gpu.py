"""Every conv kernel route against an operand-rounded fp64 emulation (tests/conv_emulation.py).

Each row names an entry point, an arithmetic mode, the srhip_debug_set knobs that force a route, a shape / epilogue and the
arithmetic the route is expected to run.  The test asserts (a) the result is within tau * |conv|(|x|, |w|) + 2 * 2^-24 * |ref|
of that arithmetic's emulation, element by element, and (b) that every neighbouring arithmetic whose emulation lies well
outside that bound is rejected by the result, i.e. the row proves which arithmetic ran.

Bars: once the operands are rounded the products are exact in fp32, so only fp32 accumulation and the fp32 epilogue remain.
Measured on the MI355X over the whole table (each row prints its own err / bound with -s): the largest error of a 16-bit
arithmetic route is 4.2 * 2^-24 * |conv| (D108-dgrad-bf16x3), of an fp32 route 7.0 * 2^-24 (D54-dgrad-fp32; the fp32 MFMA
rounds after every two products).  TAU keeps 4x above both: 20 * 2^-24 for the 16-bit arithmetics (worst err / bound 0.21),
32 * 2^-24 for fp32 (worst 0.22).

Discrimination: bf16 / fp16 / bf16x3 / fp32 emulations of one conv are thousands of bounds apart, except bf16x3 against
fp32 (the dropped lo*lo term and the rounding of lo are ~2^-17 relative, while fp32 accumulation of a long reduction
reaches a few 2^-24): there the element-wise bound separates the two only on short reductions, so the pair is also
told apart in the 2-norm -- the result must be at least 2x closer to its own emulation than to the other.

The knob state is global to the library: every row resets it in a finally block."""
import zlib

import pytest
import torch

from tests import conv_emulation as E

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
U = E.U24
TAU = {'fp32': 32 * U, 'bf16x3': 20 * U, 'bf16': 20 * U, 'fp16': 20 * U}
KNOB_DEFAULTS = {0: 0, 1: 0, 5: 0, 10: 1, 11: 1, 17: 1}
NEIGHBOURS = {'fp32': ('bf16x3', 'bf16', 'fp16'), 'bf16x3': ('fp32', 'bf16', 'fp16'), 'bf16': ('fp16', 'bf16x3', 'fp32'),
              'fp16': ('bf16', 'bf16x3', 'fp32')}


def R(rid, op, mode, expect, shape, knobs=None, **opt):
    return pytest.param(dict(op=op, mode=mode, expect=expect, shape=shape, knobs=knobs or {}, **opt), id=rid)


# shape: (n, cin, h, w, cout, k, stride, pad)
ROWS = [
    # ---- forward: exact-fp32 VALU kernels ----
    R('narrow3-bf16x3', 'fwd', 'bf16x3', 'fp32', (1, 16, 256, 256, 3, 3, 1, 1), bias=True, slope=0.2),
    R('narrow4-half', 'fwd', 'half', 'fp32', (1, 16, 256, 264, 4, 3, 1, 1), bias=True),
    R('dot-half', 'fwd', 'half', 'fp32', (2, 128, 14, 14, 1, 3, 1, 1), bias=True),
    R('dot-bf16x3-D-out', 'fwd', 'bf16x3', 'fp32', (2, 64, 13, 11, 1, 3, 1, 1)),
    # ---- forward: fast_conv_kernel<128, 32, ...> (Cout <= 32), MATH 0..3 ----
    R('k32-math0-fp32', 'fwd', 'fp32', 'fp32', (2, 32, 20, 18, 32, 3, 1, 1), bias=True, slope=0.2),
    R('k32-math1-bf16x3', 'fwd', 'bf16x3', 'bf16x3', (2, 32, 20, 18, 32, 3, 1, 1), bias=True, slope=0.2),
    R('k32-math3-half', 'fwd', 'half', 'fp16', (2, 32, 20, 18, 32, 3, 1, 1), bias=True, slope=0.2),
    R('k32-math2-half-graddata', 'fwd', 'half', 'bf16', (2, 32, 20, 18, 32, 3, 1, 1), graddata=True),
    R('k32-cfg20-bf16x3', 'fwd', 'bf16x3', 'fp32', (2, 32, 20, 18, 16, 3, 1, 1), knobs={0: 20}),
    R('k32-ld192-half-ndsrgan', 'fwd_ld', 'half', 'fp16', (2, 96, 17, 19, 32, 3, 1, 1), ldx=192, ldy=192, yoff=96, bias=True, slope=0.2),
    R('k32-ld192-bf16x3-ndsrgan', 'fwd_ld', 'bf16x3', 'bf16x3', (2, 160, 17, 19, 32, 3, 1, 1), ldx=192, ldy=192, yoff=160, bias=True),
    R('k32-dgrad-half', 'dgrad', 'half', 'bf16', (2, 32, 20, 18, 32, 3, 1, 1)),
    # ---- forward: register-staged tiles (fp32 MFMA in every mode) ----
    R('reg128x128-fp32', 'fwd', 'fp32', 'fp32', (2, 64, 20, 20, 320, 3, 1, 1), knobs={0: 5}, bias=True, residual=True),
    R('reg128x64-fp32', 'fwd', 'fp32', 'fp32', (2, 64, 20, 20, 96, 3, 1, 1), knobs={0: 8}, bias=True, slope=0.2),
    R('reg64x64-half', 'fwd', 'half', 'fp32', (1, 64, 19, 21, 96, 3, 1, 1), knobs={0: 7}, bias=True),
    R('reg-fallback-bf16x3-s2', 'fwd', 'bf16x3', 'fp32', (2, 64, 16, 16, 64, 3, 2, 1), bias=True),
    R('reg-fallback-half-dgrad-s2', 'dgrad', 'half', 'fp32', (2, 64, 16, 16, 64, 3, 2, 1)),
    R('reg-fallback-bf16x3-rowscale', 'fwd', 'bf16x3', 'fp32', (2, 64, 9, 9, 64, 1, 1, 0), rowscale=True, chanscale=True, bias=True),
    # ---- forward: patch kernels ----
    R('pers-bf16x3-128', 'fwd', 'bf16x3', 'bf16x3', (2, 64, 23, 21, 128, 3, 1, 1), knobs={0: -2}, bias=True, slope=0.2),
    R('pers-bf16x3-64-residual', 'fwd', 'bf16x3', 'bf16x3', (2, 64, 23, 21, 64, 3, 1, 1), knobs={0: -2}, bias=True, residual=True),
    R('pers-half-prod2', 'fwd', 'half', 'fp16', (2, 64, 23, 21, 128, 3, 1, 1), knobs={0: -2}, bias=True, slope=0.2),
    R('pers-half-prod1-dgrad', 'dgrad', 'half', 'bf16', (2, 64, 23, 21, 64, 3, 1, 1), knobs={0: -2}, actmask=True, slope=0.2),
    R('pers-half-prod1-graddata', 'fwd', 'half', 'bf16', (2, 64, 23, 21, 64, 3, 1, 1), knobs={0: -2}, graddata=True),
    R('patch64-epi1-bf16x3', 'fwd', 'bf16x3', 'bf16x3', (2, 64, 23, 21, 64, 3, 1, 1), knobs={0: -2, 5: -1, 10: 0}, bias=True),
    R('patch128-epi3-bf16x3', 'fwd', 'bf16x3', 'bf16x3', (2, 64, 23, 21, 320, 3, 1, 1), knobs={0: -2, 5: -1}, bias=True, slope=0.2),
    R('patch64-epi32-bf16x3-dgrad', 'dgrad', 'bf16x3', 'bf16x3', (2, 64, 23, 21, 64, 3, 1, 1), knobs={0: -2, 5: -1, 10: 0}, actmask=True,
      slope=0.2),
    R('patch-prod2-half', 'fwd', 'half', 'fp16', (2, 64, 23, 21, 128, 3, 1, 1), knobs={0: -2, 5: -1}, bias=True),
    R('patch-prod1-half-dgrad', 'dgrad', 'half', 'bf16', (2, 64, 23, 21, 64, 3, 1, 1), knobs={0: -2, 5: -1}),
    R('patch-ks-bf16x3', 'fwd', 'bf16x3', 'bf16x3', (2, 64, 23, 21, 64, 3, 1, 1), knobs={0: -2, 5: -1}, residual=True),
    # ---- forward / data gradient: LDS-DMA kernel, every epilogue set ----
    R('dma-epi0-fp32', 'fwd', 'fp32', 'fp32', (2, 64, 15, 13, 64, 1, 1, 0), knobs={0: -1}),
    R('dma-epi1-bf16x3', 'fwd', 'bf16x3', 'bf16x3', (2, 64, 15, 13, 576, 1, 1, 0), knobs={0: -1}, bias=True),
    R('dma-epi3-bf16x3-s2', 'fwd', 'bf16x3', 'bf16x3', (2, 64, 17, 15, 128, 3, 2, 1), knobs={0: -1}, bias=True, slope=0.2),
    R('dma-epi4-fp32', 'fwd', 'fp32', 'fp32', (1, 64, 15, 13, 96, 1, 1, 0), knobs={0: -1}, residual=True),
    R('dma-epi29-bf16x3', 'fwd', 'bf16x3', 'bf16x3', (2, 64, 15, 13, 64, 1, 1, 0), knobs={0: -1}, bias=True, residual=True,
      rowscale=True, chanscale=True),
    R('dma-epi29-fp32', 'fwd', 'fp32', 'fp32', (2, 64, 15, 13, 64, 1, 1, 0), knobs={0: -1}, bias=True, residual=True, rowscale=True,
      chanscale=True),
    R('dma-epi32-bf16x3-dgrad', 'dgrad', 'bf16x3', 'bf16x3', (2, 64, 17, 15, 64, 1, 1, 0), knobs={0: -1}, actmask=True, slope=0.2),
    R('dma-accumulate-bf16x3', 'dgrad_ld', 'bf16x3', 'bf16x3', (2, 64, 13, 11, 64, 3, 1, 1), knobs={0: -1}, ldy=64, ldx=192, accumulate=True),
    R('dma-accumulate-fp32', 'dgrad_ld', 'fp32', 'fp32', (2, 64, 13, 11, 96, 3, 1, 1), knobs={0: -1}, ldy=96, ldx=64, accumulate=True),
    R('dma-half-fwd-s2', 'fwd', 'half', 'fp16', (2, 64, 17, 15, 128, 3, 2, 1), knobs={0: -1}, bias=True, slope=0.2),
    R('dma-half-graddata-64', 'fwd', 'half', 'bf16', (2, 64, 17, 15, 64, 1, 1, 0), knobs={0: -1}, graddata=True),
    R('dma-half-dgrad-residual', 'dgrad', 'half', 'bf16', (2, 64, 17, 15, 128, 1, 1, 0), knobs={0: -1}, residual=True),
    # ---- strided data gradient: phase batching on / off, per phase in half ----
    R('dgrad-s2-batched-bf16x3', 'dgrad', 'bf16x3', 'bf16x3', (2, 64, 27, 27, 128, 3, 2, 1), knobs={0: -1}),
    R('dgrad-s2-perphase-bf16x3', 'dgrad', 'bf16x3', 'bf16x3', (2, 64, 27, 27, 128, 3, 2, 1), knobs={0: -1, 17: 0}),
    R('dgrad-s2-batched-fp32-4x4', 'dgrad', 'fp32', 'fp32', (2, 64, 28, 26, 64, 4, 2, 1), knobs={0: -1}),
    R('dgrad-s2-perphase-half', 'dgrad', 'half', 'bf16', (2, 64, 27, 26, 128, 3, 2, 1), knobs={0: -1}),
    R('dgrad-s2-half-4x4-tiny', 'dgrad', 'half', 'bf16', (2, 64, 28, 26, 64, 4, 2, 1), knobs={0: -1}, dyscale=1e-7),
    # ---- legacy generic kernels (fp32 in every mode) ----
    R('legacy-fwd-cin3', 'fwd', 'bf16x3', 'fp32', (3, 3, 17, 19, 64, 3, 1, 1), bias=True, slope=0.2),
    R('legacy-fwd-cin3-7x7-half', 'fwd', 'half', 'fp32', (2, 3, 13, 11, 4, 7, 1, 3), bias=True),
    R('legacy-headconv-cin3', 'fwd', 'bf16x3', 'fp32', (1, 3, 256, 256, 64, 3, 1, 1), bias=True),
    R('legacy-dgrad-cout3', 'dgrad', 'bf16x3', 'fp32', (2, 64, 16, 16, 3, 3, 1, 1)),
    R('legacy-dgrad-cout1-half', 'dgrad', 'half', 'fp32', (2, 64, 14, 14, 1, 3, 1, 1)),
    # ---- padded-plane entry points ----
    R('pp-fwd-bf16x3', 'fwd_pp', 'bf16x3', 'bf16x3', (2, 64, 23, 21, 64, 3, 1, 1), bias=True, slope=0.2),
    R('pp-fwd-wide-bf16x3', 'fwd_pp', 'bf16x3', 'bf16x3', (2, 64, 23, 21, 256, 3, 1, 1), bias=True),
    R('pp-dgrad-bf16x3', 'dgrad_pp', 'bf16x3', 'bf16x3', (2, 256, 23, 21, 64, 3, 1, 1), residual=True),
    # ---- dilated entry points, every mode ----
    # (small launches run the exact-fp32 register kernel in every mode, as any small 3x3 conv does)
    R('dil2-fwd-fp32', 'dil_fwd', 'fp32', 'fp32', (2, 64, 19, 17, 64, 3, 1, 2), d=2, bias=True, slope=0.2),
    R('dil2-fwd-bf16x3-small', 'dil_fwd', 'bf16x3', 'fp32', (2, 64, 19, 17, 64, 3, 1, 2), d=2, bias=True),
    R('dil3-fwd-half-small', 'dil_fwd', 'half', 'fp32', (2, 64, 19, 17, 64, 3, 1, 3), d=3, bias=True),
    R('dil2-fwd-bf16x3', 'dil_fwd', 'bf16x3', 'bf16x3', (8, 64, 48, 46, 64, 3, 1, 2), d=2, bias=True, slope=0.2),
    R('dil3-fwd-half', 'dil_fwd', 'half', 'fp16', (8, 64, 48, 46, 64, 3, 1, 3), d=3, bias=True),
    R('dil2-dgrad-bf16x3-small', 'dil_dgrad', 'bf16x3', 'fp32', (2, 64, 19, 17, 64, 3, 1, 2), d=2),
    R('dil3-dgrad-half-small', 'dil_dgrad', 'half', 'fp32', (2, 64, 19, 17, 64, 3, 1, 3), d=3),
    R('dil2-dgrad-bf16x3', 'dil_dgrad', 'bf16x3', 'bf16x3', (8, 64, 48, 46, 64, 3, 1, 2), d=2),
    R('dil3-dgrad-half', 'dil_dgrad', 'half', 'bf16', (8, 64, 48, 46, 64, 3, 1, 3), d=3),
    R('dil2-dgrad-fp32', 'dil_dgrad', 'fp32', 'fp32', (2, 64, 19, 17, 64, 3, 1, 2), d=2),
    R('dil2-wgrad-bf16x3', 'dil_wgrad', 'bf16x3', 'bf16x3', (2, 64, 19, 17, 64, 3, 1, 2), d=2, bias=True),
    R('dil3-wgrad-half', 'dil_wgrad', 'half', 'bf16', (2, 64, 19, 17, 64, 3, 1, 3), d=3, bias=True),
    R('dil2-wgrad-fp32', 'dil_wgrad', 'fp32', 'fp32', (2, 64, 19, 17, 64, 3, 1, 2), d=2, bias=True),
    # ---- weight gradient: row-tap kernel ----
    R('rowtap128-split', 'wgrad', 'bf16x3', 'bf16x3', (2, 64, 20, 20, 128, 3, 1, 1), bias=True),
    R('rowtap128-nosplit-half', 'wgrad', 'half', 'bf16', (2, 64, 20, 20, 128, 3, 1, 1), bias=True),
    R('rowtap64-split', 'wgrad', 'bf16x3', 'bf16x3', (2, 128, 19, 17, 64, 3, 1, 1), bias=True),
    R('rowtap64-nosplit-half', 'wgrad', 'half', 'bf16', (1, 128, 19, 17, 64, 3, 1, 1), bias=True),
    R('rowtap-tails-off', 'wgrad', 'bf16x3', 'bf16x3', (2, 64, 20, 20, 128, 3, 1, 1), knobs={1: 9}, bias=True),
    R('rowtap-accumulate-cout320', 'wgrad', 'bf16x3', 'bf16x3', (1, 64, 13, 24, 320, 3, 1, 1), accumulate=True, bias=True),
    R('rowtap-ld192-ndsrgan', 'wgrad_ld', 'half', 'bf16', (2, 128, 17, 19, 64, 3, 1, 1), ldx=192, ldy=192),
    R('wgrad-multi-bf16x3', 'wgrad_multi', 'bf16x3', 'bf16x3', (4, 64, 32, 32, 128, 3, 1, 1)),
    R('wgrad-multi-half', 'wgrad_multi', 'half', 'bf16', (4, 64, 32, 32, 128, 3, 1, 1)),
    # ---- weight gradient: LDS-DMA kernel, every tile and arithmetic ----
    R('wdma-256x64-bf16x3', 'wgrad', 'bf16x3', 'bf16x3', (2, 64, 17, 15, 256, 3, 2, 1), bias=True),
    R('wdma-64x256-fp32', 'wgrad', 'fp32', 'fp32', (2, 256, 15, 13, 64, 1, 1, 0), knobs={1: 5}, bias=True),
    R('wdma-128x128-half', 'wgrad', 'half', 'bf16', (2, 128, 17, 15, 128, 3, 2, 1), bias=True),
    R('wdma-128x64-bf16x3', 'wgrad', 'bf16x3', 'bf16x3', (2, 64, 17, 15, 128, 3, 2, 1), bias=True),
    R('wdma-64x128-half', 'wgrad', 'half', 'bf16', (2, 128, 17, 15, 64, 3, 2, 1), bias=True),
    R('wdma-64x64-fp32-bk16', 'wgrad', 'fp32', 'fp32', (2, 64, 17, 15, 64, 3, 2, 1), bias=True),
    R('wdma-64x64-fp32-bk32', 'wgrad', 'fp32', 'fp32', (2, 64, 17, 15, 64, 3, 2, 1), knobs={1: 3}, bias=True),
    R('wdma-4x4-s2-bf16x3', 'wgrad', 'bf16x3', 'bf16x3', (2, 64, 28, 26, 128, 4, 2, 1), bias=True),
    R('wdma-cout576-1x1-bf16x3', 'wgrad', 'bf16x3', 'bf16x3', (1, 64, 15, 13, 576, 1, 1, 0), bias=True),
    R('wdma-tiny-grad-half', 'wgrad', 'half', 'bf16', (2, 64, 17, 15, 64, 3, 2, 1), dyscale=1e-7, bias=True),
    R('wdma-reduce4-off-r4', 'wgrad', 'bf16x3', 'bf16x3', (2, 64, 17, 15, 64, 3, 2, 1), knobs={1: 6}, bias=True),
    R('wdma-reduce4-off-r16', 'wgrad', 'bf16x3', 'bf16x3', (16, 64, 64, 64, 64, 1, 1, 0), knobs={1: 6}, bias=True),   # nsplit 256
    R('wdma-reduce4-r16-ref', 'wgrad', 'bf16x3', 'bf16x3', (16, 64, 64, 64, 64, 1, 1, 0), bias=True),
    # ---- weight gradient: exact-fp32 kernels ----
    R('wreg-xscale-bf16x3', 'wgrad', 'bf16x3', 'fp32', (2, 64, 15, 13, 128, 3, 1, 1), xrow=True, xchan=True, bias=True),
    R('wreg-xchan-half', 'wgrad', 'half', 'fp32', (2, 64, 15, 13, 64, 1, 1, 0), xchan=True),
    R('w1x1-scaled-bf16x3', 'wgrad', 'bf16x3', 'fp32', (2, 64, 15, 13, 64, 1, 1, 0), xrow=True, xchan=True, bias=True),
    R('wlegacy-smallcin', 'wgrad', 'bf16x3', 'fp32', (1, 3, 256, 256, 64, 3, 1, 1), bias=True),
    R('wlegacy-narrow-cout3', 'wgrad', 'half', 'fp32', (1, 64, 256, 256, 3, 3, 1, 1), bias=True),
    R('wlegacy-generic-cout1', 'wgrad', 'bf16x3', 'fp32', (2, 64, 14, 14, 1, 3, 1, 1), bias=True),
    R('wlegacy-generic-7x7', 'wgrad', 'half', 'fp32', (2, 2, 9, 11, 1, 7, 1, 3)),
    # ---- flat padded-plane weight gradient ----
    R('wflat-dy-pp', 'wgrad_pp', 'bf16x3', 'bf16x3', (2, 64, 23, 21, 128, 3, 1, 1), xpp=False, ypp=True),
    R('wflat-x-pp', 'wgrad_pp', 'bf16x3', 'bf16x3', (2, 128, 23, 21, 64, 3, 1, 1), xpp=True, ypp=False),
    R('wflat-both-pp', 'wgrad_pp', 'bf16x3', 'bf16x3', (2, 64, 23, 21, 256, 3, 1, 1), xpp=True, ypp=True),
    # ---- half: fp16 subnormal activations ----
    R('half-subnormal-act', 'fwd', 'half', 'fp16', (2, 32, 20, 18, 32, 3, 1, 1), xscale=2e-5),
    R('half-subnormal-act-dma', 'fwd', 'half', 'fp16', (2, 64, 17, 15, 128, 3, 2, 1), knobs={0: -1}, xscale=2e-5),
]

# D's stride-2 convs at training size (B = 32: 216 -> 108 -> 54 -> 27 -> 14), every op and mode
_D = [(32, 64, 216, 216, 64), (32, 128, 108, 108, 128), (32, 256, 54, 54, 256), (32, 512, 27, 27, 512)]
_EXPECT = {('fwd', 'fp32'): 'fp32', ('fwd', 'bf16x3'): 'bf16x3', ('fwd', 'half'): 'fp16', ('dgrad', 'fp32'): 'fp32',
           ('dgrad', 'bf16x3'): 'bf16x3', ('dgrad', 'half'): 'bf16', ('wgrad', 'fp32'): 'fp32', ('wgrad', 'bf16x3'): 'bf16x3',
           ('wgrad', 'half'): 'bf16'}
D_ROWS = [R('D%d-%s-%s' % (h, op, mode), op, mode, _EXPECT[(op, mode)], (n, c, h, h, co, 3, 2, 1), bias=op != 'dgrad', slope=0.2 if op == 'fwd' else None)
          for (n, c, h, _, co) in _D for op in ('fwd', 'dgrad', 'wgrad') for mode in ('fp32', 'bf16x3', 'half')]


def _lib():
    from sradsgan_amd import _hip
    return _hip.lib()


def _rand(shape, g, scale=1.0):
    t = torch.randn(shape, generator=g, device=DEV) * scale
    return t.contiguous(memory_format=torch.channels_last) if len(shape) == 4 else t


def _nhwc_out(guards, n, c, ld, h, w, prefill=None):
    """An output of c channels in rows of ld floats, as the [n, c, h, w] view the wrappers take.  guards None: a plain buffer.
    guards a list (tests/test_conv_geometry_gpu.py): the rows lie in a pointwise_ref.Guarded allocation -- sentinel bands on both
    sides, body NaN unless prefill (an accumulate destination's previous contents, [n, c, h, w]) -- and the list receives what the
    caller must find afterwards: bands and the ld - c pad columns intact, every body element written."""
    if guards is None:
        buf = torch.full((n, h, w, ld), float('nan'), device=DEV)
    else:
        from tests.pointwise_ref import Guarded
        gd = Guarded((n, h, w, ld), DEV)
        buf = gd.t
    view = buf.permute(0, 3, 1, 2)
    if prefill is not None:
        view[:, :c] = prefill
    if guards is not None:
        guards.append(dict(guard=gd, body=view[:, :c], pad=view[:, c:], accumulate=prefill is not None))
    return view


def _flat_out(guards, shape, prefill=None):
    """A dense output (a weight or bias gradient) of `shape`, in a Guarded allocation when guards is a list (see _nhwc_out)."""
    if guards is None:
        return prefill.clone() if prefill is not None else torch.zeros(shape, device=DEV)
    from tests.pointwise_ref import Guarded
    gd = Guarded(shape, DEV)
    if prefill is not None:
        gd.t.copy_(prefill)
    guards.append(dict(guard=gd, body=gd.t, pad=None, accumulate=prefill is not None))
    return gd.t


def _run(row, g, guards=None):
    """Run the row's entry point; return [(name, got, emulate(arith, with_abs) -> (ref, absref), is_discriminating)].
    guards: a list -- the outputs the row hands to an entry point itself (row stride / out= forms) then lie in Guarded allocations."""
    from sradsgan_amd import ops
    op, (n, cin, h, w, cout, k, s, p) = row['op'], row['shape']
    d = row.get('d', 1)
    ho, wo = (h + 2 * p - d * (k - 1) - 1) // s + 1, (w + 2 * p - d * (k - 1) - 1) // s + 1
    wt = _rand((cout, cin, k, k), g, (cin * k * k) ** -0.5)
    b = _rand((cout,), g) if row.get('bias') else None
    slope = row.get('slope')
    x = _rand((n, cin, h, w), g, row.get('xscale', 1.0))
    dy = _rand((n, cout, ho, wo), g, row.get('dyscale', 1.0))
    out = []
    if op in ('fwd', 'fwd_ld', 'fwd_pp', 'dil_fwd'):
        res = _rand((n, cout, ho, wo), g) if row.get('residual') else None
        rs = _rand((n, 1, ho, wo), g).abs().contiguous(memory_format=torch.channels_last) + 0.5 if row.get('rowscale') else None
        cs = _rand((n, cin), g).abs() + 0.5 if row.get('chanscale') else None
        xs = x * cs.view(n, cin, 1, 1) if cs is not None else x
        # operand scale in fp32 before rounding, as the kernels apply it
        xs = xs.float()
        if op == 'fwd':
            y = ops.conv2d_fwd_raw(x, wt, b, s, p, slope=slope, residual=res, rowscale=rs.reshape(-1) if rs is not None else None,
                                   chanscale=cs, graddata=row.get('graddata', False))
        elif op == 'fwd_ld':
            ldx, ldy, yoff = row['ldx'], row['ldy'], row['yoff']
            xb = torch.zeros(n, ldx, h, w, device=DEV).contiguous(memory_format=torch.channels_last)
            xb[:, :cin] = x
            xb[:, cin:] = float('nan')                        # channels past cin must not be read
            yb = torch.full((n, ldy, h, w), 7.0, device=DEV).contiguous(memory_format=torch.channels_last)
            ops.conv2d_fwd_ld(xb, ldx, wt, b, yb[:, yoff:], ldy, n, h, w, slope)
            keep = torch.cat([yb[:, :yoff], yb[:, yoff + cout:]], 1)
            assert bool((keep == 7.0).all()), 'conv2d_fwd_ld wrote outside its channel slice'
            y = yb[:, yoff:yoff + cout]
        elif op == 'fwd_pp':
            y = ops.conv2d_fwd_pp_raw(ops.pp_from_f32(x), wt, b, slope=slope)
        else:
            ldx, ldy = row.get('ldx', cin), row.get('ldy', cout)
            xb = _nhwc_out(None, n, cin, ldx, h, w, prefill=x)          # (channels past cin are NaN: they must not be read)
            y = _nhwc_out(guards, n, cout, ldy, h, w)[:, :cout]
            ops.conv2d_dil_fwd_raw(xb, ldx, wt, b, y, ldy, n, h, w, d, slope=slope)

        def emu(a, with_abs=True):
            r, ar = E.conv_fwd(xs, wt, s, p, a, d, with_abs=with_abs)
            if ar is None:
                ar = torch.zeros_like(r)
            return E.epilogue(r, ar, rowscale=rs, bias=b, slope=slope, residual=res)
        out.append(('y', y, emu, True))
    elif op in ('dgrad', 'dgrad_ld', 'dgrad_pp', 'dil_dgrad'):
        res = _rand((n, cin, h, w), g) if row.get('residual') else None
        am = _rand((n, cin, h, w), g) if row.get('actmask') else None
        prev = None
        if op == 'dgrad':
            dx = ops.conv2d_dgrad_raw(dy, wt, (n, cin, h, w), s, p, residual=res, actmask=am, slope=slope or 0.0)
        elif op == 'dgrad_ld':
            ldx, ldy = row['ldx'], row['ldy']
            yb = torch.zeros(n, ldy, ho, wo, device=DEV).contiguous(memory_format=torch.channels_last)
            yb[:, :cout] = dy
            xb = _rand((n, ldx, h, w), g)
            prev = xb[:, :cin].clone()
            rest = xb[:, cin:].clone()
            ops.conv2d_dgrad_ld(yb, ldy, wt, xb, ldx, n, h, w, accumulate=row.get('accumulate', False))
            assert torch.equal(xb[:, cin:], rest), 'conv2d_dgrad_ld wrote outside its channel slice'
            dx = xb[:, :cin]
            if not row.get('accumulate'):
                prev = None
        elif op == 'dgrad_pp':
            dx = ops.conv2d_dgrad_pp_raw(ops.pp_from_f32(dy), wt, residual=res)
        else:
            ldx, ldy = row.get('ldx', cin), row.get('ldy', cout)
            yb = _nhwc_out(None, n, cout, ldy, ho, wo, prefill=dy)
            prev = _rand((n, cin, h, w), g) if row.get('accumulate') else None
            dx = _nhwc_out(guards, n, cin, ldx, h, w, prefill=prev)[:, :cin]
            ops.conv2d_dil_dgrad_raw(yb, ldy, wt, dx, ldx, n, h, w, d, accumulate=row.get('accumulate', False))

        def emu(a, with_abs=True):
            r, ar = E.conv_dgrad(dy, wt, (n, cin, h, w), s, p, a, d, with_abs=with_abs)
            if ar is None:
                ar = torch.zeros_like(r)
            return E.epilogue(r, ar, actmask=am, mask_slope=slope, residual=res, prev=prev)
        out.append(('dx', dx, emu, True))
    else:
        xr = _rand((n, 1, h, w), g).abs() + 0.5 if row.get('xrow') else None
        xc = _rand((n, cin), g).abs() + 0.5 if row.get('xchan') else None
        xs = x * (xr if xr is not None else 1.0) * (xc.view(n, cin, 1, 1) if xc is not None else 1.0)
        wshape = (cout, cin, k, k)
        prev_w = prev_b = None
        extra = []
        if op == 'wgrad':
            if row.get('accumulate'):
                prev_w, prev_b = _rand(wshape, g).contiguous(), _rand((cout,), g)
                dw, db = ops.conv2d_wgrad_raw(x, dy, wshape, s, p, True, out=(_flat_out(guards, wshape, prev_w), _flat_out(guards, (cout,), prev_b)))
            else:
                dw, db = ops.conv2d_wgrad_raw(x, dy, wshape, s, p, row.get('bias', False),
                                              xrowscale=xr.reshape(-1).contiguous() if xr is not None else None, xchanscale=xc)
        elif op == 'wgrad_ld':
            ldx, ldy = row['ldx'], row['ldy']
            xb = torch.full((n, ldx, h, w), float('nan'), device=DEV).contiguous(memory_format=torch.channels_last)
            xb[:, :cin] = x
            yb = torch.full((n, ldy, ho, wo), float('nan'), device=DEV).contiguous(memory_format=torch.channels_last)
            yb[:, :cout] = dy
            dw, db = ops.conv2d_wgrad_ld(xb, ldx, yb, ldy, wshape, n, h, w)
        elif op == 'wgrad_pp':
            dw = torch.zeros(wshape, device=DEV)
            db = torch.zeros(cout, device=DEV)
            xa = ops.pp_from_f32(x) if row['xpp'] else x
            ya = ops.pp_from_f32(dy) if row['ypp'] else dy
            ops.conv2d_wgrad_pp_raw([(xa, ya, dw, db)])
        elif op == 'wgrad_multi':
            more = [(_rand(tuple(x.shape), g), _rand(tuple(dy.shape), g)) for _ in range(row.get('nprob', 2) - 1)]
            zw, zb = torch.zeros(wshape, device=DEV), torch.zeros(cout, device=DEV)
            items = [(xi, dyi, _flat_out(guards, wshape, zw), _flat_out(guards, (cout,), zb), s, p) for xi, dyi in [(x, dy)] + more]
            dw, db = items[0][2], items[0][3]
            ops.conv2d_wgrad_multi_raw(items)

            def emu_of(xi, dyi):
                def emu_i(a, with_abs=True):
                    r, ar = E.conv_wgrad(xi, dyi, wshape, s, p, a, with_abs=with_abs)
                    return r, (ar if ar is not None else torch.zeros_like(r))
                return emu_i
            for i, (xi, dyi, dwi, dbi, _, _) in enumerate(items[1:], 1):
                extra += [('dw[%d]' % i, dwi, emu_of(xi, dyi), True), ('db[%d]' % i, dbi, _colsum_emu(dyi, None), False)]
        else:
            ldx, ldy = row.get('ldx', cin), row.get('ldy', cout)
            xb, yb = _nhwc_out(None, n, cin, ldx, h, w, prefill=x), _nhwc_out(None, n, cout, ldy, ho, wo, prefill=dy)
            dw, db = ops.conv2d_dil_wgrad_raw(xb, ldx, yb, ldy, wshape, n, h, w, d, with_bias=row.get('bias', False))

        def emu(a, with_abs=True):
            r, ar = E.conv_wgrad(xs, dy, wshape, s, p, a, d, with_abs=with_abs)
            if ar is None:
                ar = torch.zeros_like(r)
            if prev_w is not None:
                r, ar = r + prev_w.double(), ar + prev_w.double().abs()
            return r, ar
        out.append(('dw', dw, emu, True))
        if db is not None:
            out.append(('db', db, _colsum_emu(dy, prev_b), False))
        out += extra
    return out


def _colsum_emu(dy, prev):
    """The bias gradient: a column sum of the raw fp32 gradient in every mode."""
    def emu(a, with_abs=True):
        r, ar = dy.double().sum((0, 2, 3)), dy.double().abs().sum((0, 2, 3))
        if prev is not None:
            r, ar = r + prev.double(), ar + prev.double().abs()
        return r, ar
    return emu


def _check(row, rid):
    from sradsgan_amd import ops
    lib = _lib()
    g = torch.Generator(device=DEV).manual_seed(zlib.crc32(rid.encode()))
    try:
        for key, v in row['knobs'].items():
            assert lib.srhip_debug_set(key, v) == 0
        with ops.conv_math(row['mode']):
            results = _run(row, g)
        torch.cuda.synchronize()
    finally:
        for key in row['knobs']:
            lib.srhip_debug_set(key, KNOB_DEFAULTS[key])
    report = []
    for name, got, emu, disc in results:
        expect = row['expect'] if disc else 'fp32'
        tau = TAU[expect]
        ref, absref = emu(expect)
        ratio = E.assert_conv_close(got, ref, absref, tau, what='%s %s (%s)' % (rid, name, expect))
        line = '%s %s: %s err/bound %.3f at tau %g * 2^-24' % (rid, name, expect, ratio, tau / U)
        if disc:
            rejected, close = [], []
            d_own = E.l2_dist(got, ref)
            for nb in NEIGHBOURS[expect]:
                ref_nb = emu(nb, with_abs=False)[0]
                sep = E.worst(ref_nb, ref, absref, tau)[0]            # how far apart the two arithmetics are, in bounds
                if sep > 8:                                            # element-wise: the result breaks the neighbour's bound
                    r_nb = E.worst(got, ref_nb, absref, tau)[0]
                    assert r_nb > 1, '%s %s: the result also fits %s (err/bound %.3f): the route may not run %s' % (
                        rid, name, nb, r_nb, expect)
                    rejected.append('%s(%.0f)' % (nb, r_nb))
                elif {nb, expect} == {'fp32', 'bf16x3'}:               # the close pair: 2-norm distances
                    q = E.l2_dist(got, ref_nb) / max(d_own, 1e-300)
                    assert q > 2, '%s %s: the result is as close to %s as to %s (2-norm ratio %.2f)' % (rid, name, nb, expect, q)
                    rejected.append('%s(2-norm x%.1f)' % (nb, q))
                else:
                    close.append('%s(sep %.1f)' % (nb, sep))
            assert rejected, '%s %s: no neighbouring arithmetic is discriminated' % (rid, name)
            line += '; rejects %s' % ' '.join(rejected) + ('; too close: %s' % ' '.join(close) if close else '')
        report.append(line)
    print('\n'.join(report))


@pytest.mark.parametrize('row', ROWS)
def test_conv_route(row, request):
    _check(row, request.node.callspec.id)


@pytest.mark.parametrize('row', D_ROWS)
def test_discriminator_stride2_training_shapes(row, request):
    _check(row, request.node.callspec.id)
