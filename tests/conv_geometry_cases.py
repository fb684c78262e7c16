"""The table of tests/test_conv_geometry_gpu.py: every conv kernel family at the geometries where a tiled implicit-GEMM kernel goes wrong.

A row is the dict tests/test_conv_routes_gpu.py runs (op, mode, expect, shape, knobs and the operand options) plus
  fam     the family section it is filed under (FAMILIES)
  cls     the class of that family it covers (CLASSES[fam]); tests/test_conv_geometry_cpu.py checks that every class has its modes
  route   what ONE line of srhip_conv2d_last_route must say: {'fam': name, 'tile': 'AxB', 'bn': .., 'epi': .., 'phases': .., ...}
  nlaunch (optional) the number of launches of the call
  patch   (patch family) the class of the recorded PH x PW against the output image, see PATCH_CLASSES: taken from the record, the
          table does not restate plan_patch
  same    (optional) knob sets whose result must equal this row's bit for bit (the identities the code documents)
  note    why a listed shape was replaced, where one was

shape: (n, cin, h, w, cout, k, stride, pad), h x w the INPUT image (the dx of a data gradient).

Sizes: n <= 64, images <= 72 on a side, channels <= 320 (CAPS).  M = 127 and M = 257 are prime, so a row with exactly that many output
pixels needs that many 1 x 1 images or an image side above 72: those rows carry big_n and use 1 x 1 images (with a 3 x 3 filter, pad 1,
which is also the "image smaller than the filter" geometry); the narrow kernel's M >= 65536 threshold needs n above 64 too.

Shapes the issue lists that are not convolutions: a stride-2 k = 4 pad-1 conv has no output on a 1 x W or H x 1 input (h + 2 pad < k), so
the k = 4 data gradients run onto 2 x 2, 3 x 3 and 2 x 7 only; the entry points refuse such a geometry (tests/test_conv_geometry_cpu.py).
Modes: the patch family and the row-tap kernel exist in the 16-bit arithmetics only (choose_fprop_route / rowtap_ok ask for
g_conv_math >= 1), so their classes run bf16x3 (and half once); every other class runs bf16x3 and fp32, and half once per family.
PW >= 47 tiles exist for padded-plane operands only (plan_patch with min_eff = 0), which keep their own files."""

CAPS = dict(n=64, side=72, chan=320)
FAMILIES = ('k32', 'regtile', 'dma', 'patch', 'narrow', 'dot', 'legacy', 'dil', 'rowtap', 'wdma', 'tail1x1', 'wreg', 'wlegacy')
# families whose kernels exist in the 16-bit arithmetics only
MODES16 = ('patch', 'rowtap')
PATCH_CLASSES = ('pw<16', '16<=pw<32', '32<=pw<47', 'ragged-row', 'ragged-col', 'ragged-both', 'ph-clipped', 'one-tile', 'tiles_w>=3')
CLASSES = {
    'k32': ('cdst-csrc-k-stride', 'M-edge', 'image<filter', 'many-samples', 'cdst1-residual', 'dgrad'),
    'regtile': ('M-edge', 'k32-declines', '1x1-chunks', 'odd-kernels', 'heuristic-64x64'),
    'dma': ('M-edge', 'cdst-csrc-k', 'many-samples', 'epilogues', 'accumulate-ld', 's2-dgrad-tiny'),
    'patch': PATCH_CLASSES + ('cdst', 'csrc', 'epilogues', 'pers-grid', 'ks-off'),
    'narrow': ('over-threshold', 'under-threshold'),
    'dot': ('M-edge', 'csrc', 'row-stride'),
    'legacy': ('cin-k-cout', 'dgrad', 'tiny-images'),
    'dil': ('fwd', 'dgrad', 'dgrad-accumulate', 'wgrad', 'wide-rows'),
    'rowtap': ('wo-ho', 'cout-cin', 'tails-off', 'accumulate', 'empty-splits', 'multi'),
    'wdma': ('cout-edge', 'cin-k', 'P-edge', 'stride2-odd', 'no-bias'),
    'tail1x1': ('hw-n', 'workspace-short'),
    'wreg': ('P-edge', 'ragged'),
    'wlegacy': ('P-edge', 'ragged'),
}

ROWS = []


def _arith(fam, op, mode, opt):
    """The arithmetic the family runs in a mode (tests/conv_emulation.py names)."""
    if opt.get('expect_by_mode'):
        pass                                          # a row filed under an exact-fp32 family that must land on a 16-bit kernel
    elif fam in ('narrow', 'dot', 'legacy', 'regtile', 'tail1x1', 'wreg', 'wlegacy') or opt.get('chanscale') and fam == 'k32':
        return 'fp32'
    if mode != 'half':
        return mode
    if op.startswith('wgrad') or op.startswith('dgrad') or opt.get('graddata'):
        return 'bf16'
    return 'fp16'


def add(fam, cls, rid, op, mode, shape, route, knobs=None, expect=None, **opt):
    assert fam in FAMILIES and cls in CLASSES[fam], (fam, cls)
    row = dict(id='%s-%s-%s' % (fam, rid, mode), fam=fam, cls=cls, op=op, mode=mode, shape=tuple(shape), knobs=dict(knobs or {}), route=dict(route),
               expect=expect or _arith(fam, op, mode, opt), **opt)
    ROWS.append(row)
    return row


def both(fam, cls, rid, op, shape, route, knobs=None, half=False, **opt):
    """The row in bf16x3 and fp32 (16-bit-only families: bf16x3), and in half where the family's most ragged case is marked."""
    modes = ['bf16x3'] + ([] if fam in MODES16 else ['fp32']) + (['half'] if half else [])
    for mode in modes:
        r = dict(route)
        for key, v in list(r.items()):
            if isinstance(v, dict):                   # a field that depends on the mode
                r[key] = v[mode]
        o = dict(opt)
        if mode != 'bf16x3':
            o.pop('same', None)                       # the documented identities are split-bf16 ones
        add(fam, cls, rid, op, mode, shape, r, knobs, **o)


BIG_N = 'a prime M needs that many 1 x 1 images'

# ================================================================================================================================ #
# <= 32-channel register kernel: launch_reg<128, 32, ...>, math 0 / 1 / 3 (2 on gradient data)
# ================================================================================================================================ #
K32 = {'fam': 'reg', 'tile': '128x32', 'math': {'fp32': 0, 'bf16x3': 1, 'half': 3}}
K32G = {'fam': 'reg', 'tile': '128x32', 'math': {'fp32': 0, 'bf16x3': 1, 'half': 2}}
for i, s in enumerate([(2, 16, 7, 9, 2, 1, 1, 0), (2, 48, 7, 9, 5, 3, 1, 1), (2, 16, 9, 7, 8, 5, 1, 2), (2, 16, 11, 9, 32, 5, 2, 2),
                       (2, 48, 7, 7, 32, 1, 2, 0), (3, 16, 5, 5, 31, 1, 1, 0)]):
    both('k32', 'cdst-csrc-k-stride', 'c%dx%d-k%ds%d' % (s[4], s[1], s[5], s[6]), 'fwd', s, K32, bias=i % 2 == 0, slope=0.2 if i % 3 == 0 else None)
both('k32', 'cdst-csrc-k-stride', 'c31x48-k3s2-ragged', 'fwd', (2, 48, 9, 11, 31, 3, 2, 1), K32, half=True, bias=True, slope=0.2)
both('k32', 'M-edge', 'M1', 'fwd', (1, 16, 1, 1, 32, 3, 1, 1), K32, bias=True)
both('k32', 'M-edge', 'M127', 'fwd', (127, 16, 1, 1, 32, 3, 1, 1), K32, big_n=BIG_N)
both('k32', 'M-edge', 'M128', 'fwd', (2, 16, 8, 8, 32, 3, 1, 1), K32)
both('k32', 'M-edge', 'M129', 'fwd', (1, 16, 3, 43, 32, 3, 1, 1), K32, bias=True)
both('k32', 'image<filter', '1x1', 'fwd', (2, 48, 1, 1, 8, 3, 1, 1), K32, bias=True)
both('k32', 'image<filter', '2x1', 'fwd', (3, 16, 2, 1, 31, 3, 1, 1), K32)
both('k32', 'image<filter', '2x1-k5', 'fwd', (3, 16, 2, 1, 5, 5, 1, 2), K32)
both('k32', 'many-samples', 'n9-3x3', 'fwd', (9, 16, 3, 3, 32, 3, 1, 1), K32, bias=True)
both('k32', 'many-samples', 'n40-2x2', 'fwd', (40, 48, 2, 2, 31, 3, 1, 1), K32)
both('k32', 'cdst1-residual', 'c1-res', 'fwd', (2, 16, 5, 7, 1, 3, 1, 1), K32, residual=True)
both('k32', 'dgrad', 'cin5', 'dgrad', (2, 5, 7, 9, 16, 3, 1, 1), K32G)
both('k32', 'dgrad', 'cin8-s2-odd', 'dgrad', (2, 8, 9, 7, 48, 3, 2, 1), K32G, half=True, nlaunch=4)
both('k32', 'dgrad', 'cin32-s2-1x5', 'dgrad', (3, 32, 1, 5, 16, 3, 2, 1), K32G, nlaunch=2)

# ================================================================================================================================ #
# register tiles: srhip_debug_set(0, 1..8) and the heuristic's 64 x 64 (exact fp32 products in every mode)
# ================================================================================================================================ #
#            cfg: (BM, BN, BK, needs >= 128 destination channels)
REG_TILES = {1: (128, 128, 32, True), 2: (64, 128, 16, True), 3: (64, 128, 32, True), 4: (256, 128, 16, True), 5: (128, 128, 16, True),
             6: (128, 64, 32, False), 7: (64, 64, 16, False), 8: (128, 64, 32, False)}
# (n, h, w) with n * h * w = M for a 3 x 3 pad-1 stride-1 conv
M_SHAPES = {63: (1, 7, 9), 64: (1, 8, 8), 65: (1, 5, 13), 127: (127, 1, 1), 128: (2, 8, 8), 129: (1, 43, 3), 255: (5, 3, 17), 256: (4, 8, 8),
            257: (257, 1, 1)}
_cd_wide, _cd_narrow = [130, 200, 130], [33, 36, 65]
for cfg, (bm, bn, bk, k128) in REG_TILES.items():
    for j, M in enumerate((bm - 1, bm, bm + 1)):
        n, h, w = M_SHAPES[M]
        cdst = (_cd_wide if k128 else _cd_narrow)[j]
        csrc = (32, 96, 32)[j] if bk == 32 else (16, 48, 16)[j]
        opt = dict(big_n=BIG_N) if n > 64 else {}
        both('regtile', 'M-edge', 'cfg%d-M%d' % (cfg, M), 'fwd', (n, csrc, h, w, cdst, 3, 1, 1), {'fam': 'reg', 'tile': '%dx%d' % (bm, bn), 'bn': bk},
             knobs={0: cfg}, bias=j == 0, residual=j == 1, half=(cfg == 4 and j == 2), **opt)
for cfg in (1, 3, 6, 8):             # source channels 48: not a multiple of 32, the _K32 tile declines and the heuristic's tile runs
    cdst = 130 if REG_TILES[cfg][3] else 65
    both('regtile', 'k32-declines', 'cfg%d-c48' % cfg, 'fwd', (2, 48, 7, 9, cdst, 3, 1, 1), {'fam': 'reg', 'tile': '64x64', 'bn': 16}, knobs={0: cfg})
both('regtile', '1x1-chunks', 'one-chunk', 'fwd', (2, 16, 7, 9, 65, 1, 1, 0), {'fam': 'reg', 'tile': '64x64', 'bn': 16}, knobs={0: 7}, bias=True)
both('regtile', '1x1-chunks', 'two-chunks', 'fwd', (2, 32, 7, 9, 36, 1, 1, 0), {'fam': 'reg', 'tile': '64x64', 'bn': 16}, knobs={0: 7})
both('regtile', '1x1-chunks', 'one-chunk-k32', 'fwd', (2, 32, 7, 9, 200, 1, 1, 0), {'fam': 'reg', 'tile': '128x128', 'bn': 32}, knobs={0: 1})
both('regtile', 'odd-kernels', 'k4s2p1', 'fwd', (2, 16, 9, 11, 36, 4, 2, 1), {'fam': 'reg', 'tile': '64x64', 'bn': 16}, knobs={0: 7}, bias=True, slope=0.2)
both('regtile', 'odd-kernels', 'k5p2', 'fwd', (2, 48, 7, 5, 130, 5, 1, 2), {'fam': 'reg', 'tile': '64x128', 'bn': 16}, knobs={0: 2})
both('regtile', 'odd-kernels', 'k4s2p1-dgrad', 'dgrad', (2, 36, 9, 11, 16, 4, 2, 1), {'fam': 'reg', 'tile': '64x64', 'bn': 16}, knobs={0: 7}, nlaunch=4)
for M in (63, 64, 65):
    n, h, w = M_SHAPES[M]
    both('regtile', 'heuristic-64x64', 'auto-M%d' % M, 'fwd', (n, 16, h, w, (33, 65, 200)[M - 63], 3, 1, 1), {'fam': 'reg', 'tile': '64x64', 'bn': 16})

# ================================================================================================================================ #
# LDS-DMA kernel: srhip_debug_set(0, -1)
# ================================================================================================================================ #
MATH = {'fp32': 0, 'bf16x3': 1, 'half': 3}
MATHG = {'fp32': 0, 'bf16x3': 1, 'half': 2}


def dma(bn, epi, grad=False, **kw):
    e = {'fp32': epi, 'bf16x3': epi, 'half': -1}      # SRHIP_MATH_HALF: run-time epilogue flags
    return dict({'fam': 'dma', 'tile': '128x%d' % bn, 'math': MATHG if grad else MATH, 'epi': e}, **kw)


both('dma', 'M-edge', 'M1', 'fwd', (1, 16, 1, 1, 64, 1, 1, 0), dma(64, 0), knobs={0: -1})
both('dma', 'M-edge', 'M127', 'fwd', (127, 32, 1, 1, 68, 3, 1, 1), dma(64, 1), knobs={0: -1}, bias=True, big_n=BIG_N)
both('dma', 'M-edge', 'M128', 'fwd', (2, 48, 8, 8, 100, 3, 1, 1), dma(64, 0), knobs={0: -1})
both('dma', 'M-edge', 'M129', 'fwd', (1, 64, 3, 43, 128, 1, 1, 0), dma(128, 3), knobs={0: -1}, bias=True, slope=0.2)
both('dma', 'M-edge', 'M255', 'fwd', (5, 16, 3, 17, 132, 3, 1, 1), dma(128, 0), knobs={0: -1})
both('dma', 'M-edge', 'M256', 'fwd', (1, 32, 16, 16, 192, 5, 1, 2), dma(128, 1), knobs={0: -1}, bias=True)
both('dma', 'M-edge', 'M257', 'fwd', (257, 48, 1, 1, 196, 1, 1, 0), dma(128, 0), knobs={0: -1}, big_n=BIG_N)
both('dma', 'cdst-csrc-k', 'k4s2-c68', 'fwd', (2, 64, 9, 11, 68, 4, 2, 1), dma(64, 3), knobs={0: -1}, bias=True, slope=0.2)
both('dma', 'cdst-csrc-k', 'k5-c196x16', 'fwd', (2, 16, 5, 7, 196, 5, 1, 2), dma(128, 0), knobs={0: -1})
both('dma', 'cdst-csrc-k', 'k1-c100x32', 'fwd', (3, 32, 5, 7, 100, 1, 1, 0), dma(64, 1), knobs={0: -1}, bias=True)
both('dma', 'cdst-csrc-k', 'k1-c64x48', 'fwd', (3, 48, 5, 7, 64, 1, 1, 0), dma(64, 0), knobs={0: -1})
both('dma', 'cdst-csrc-k', 'dgrad-cin132', 'dgrad', (2, 132, 7, 9, 16, 3, 1, 1), dma(128, 0, True), knobs={0: -1})
both('dma', 'many-samples', 'n20-3x3', 'fwd', (20, 16, 3, 3, 100, 3, 1, 1), dma(64, 1), knobs={0: -1}, bias=True)
_E = (2, 32, 7, 9, 100, 3, 1, 1)                      # M = 126, K = 100: ragged in M and N
both('dma', 'epilogues', 'epi0', 'fwd', _E, dma(64, 0), knobs={0: -1})
both('dma', 'epilogues', 'epi1', 'fwd', _E, dma(64, 1), knobs={0: -1}, bias=True)
both('dma', 'epilogues', 'epi3', 'fwd', _E, dma(64, 3), knobs={0: -1}, bias=True, slope=0.2, half=True)
both('dma', 'epilogues', 'epi4', 'fwd', _E, dma(64, 4), knobs={0: -1}, residual=True)
both('dma', 'epilogues', 'epi32-dgrad', 'dgrad', (2, 100, 7, 9, 32, 3, 1, 1), dma(64, 32, True), knobs={0: -1}, actmask=True, slope=0.2)
both('dma', 'epilogues', 'epi29', 'fwd', _E, dma(64, 29), knobs={0: -1}, bias=True, residual=True, rowscale=True, chanscale=True)
both('dma', 'epilogues', 'epi-runtime', 'fwd', _E, dma(64, -1), knobs={0: -1}, bias=True, residual=True)
both('dma', 'accumulate-ld', 'acc-ldx100', 'dgrad_ld', (2, 68, 7, 9, 32, 3, 1, 1), dma(64, -1, True), knobs={0: -1}, ldy=48, ldx=100, accumulate=True)
both('dma', 'accumulate-ld', 'noacc-ldx200', 'dgrad_ld', (2, 132, 5, 7, 16, 3, 1, 1), dma(128, 0, True), knobs={0: -1}, ldy=16, ldx=200, accumulate=False)
# stride-2 data gradients onto tiny dx: batched (one launch, 4 phases) where every phase has pixels, else one launch per non-empty phase
for (h, w) in ((1, 1), (1, 5), (5, 1), (2, 2), (3, 3), (2, 7)):
    for k in (3, 4):
        if k == 4 and min(h, w) < 2:
            continue                                  # no such convolution (module docstring)
        nph = (2 if h > 1 else 1) * (2 if w > 1 else 1)
        full = nph == 4
        cin = 64 if (h + w) % 2 else 100
        both('dma', 's2-dgrad-tiny', 'dx%dx%d-k%d-batched' % (h, w, k), 'dgrad', (3, cin, h, w, 16 if k == 3 else 48, k, 2, 1),
             dma(64, 0, True, phases=4 if full else 0), knobs={0: -1}, nlaunch=1 if full else nph, same=[{0: -1, 17: 0}] if full else None)
        both('dma', 's2-dgrad-tiny', 'dx%dx%d-k%d-perphase' % (h, w, k), 'dgrad', (3, cin, h, w, 16 if k == 3 else 48, k, 2, 1),
             dma(64, 0, True, phases=0), knobs={0: -1, 17: 0}, nlaunch=nph, half=(h, w, k) == (2, 7, 4))   # (half never batches its phases)

# ================================================================================================================================ #
# patch family: srhip_debug_set(0, -2); knob 5 = -1 (one-tile kernels), default, 1 and 3 (persistent walk); knob 10 = K-split form
# ================================================================================================================================ #
# one image size per tile class; the class is read back from the record's PH x PW
PATCH_SIZES = {'pw<16': (30, 3), '16<=pw<32': (5, 18), '32<=pw<47': (2, 45), 'ragged-row': (9, 20), 'ragged-col': (6, 30), 'ragged-both': (13, 14),
               'ph-clipped': (4, 23), 'one-tile': (9, 10), 'tiles_w>=3': (5, 54)}
ONE_TILE = {-1: 'one-tile kernels', 0: 'default', 1: 'one block walks every tile', 3: 'three blocks'}
for pc, (h, w) in PATCH_SIZES.items():
    s = (2, 32, h, w, 64, 3, 1, 1)
    # 64-wide tile: K-split one-tile kernel, the persistent walk by default and with 1 / 3 blocks; the classic one-tile kernel is the DMA kernel's bits
    both('patch', pc, '%dx%d-ks' % (h, w), 'fwd', s, {'fam': 'patch-ks', 'bn': 64, 'epi': 1}, knobs={0: -2, 5: -1}, patch=pc, bias=True)
    both('patch', pc, '%dx%d-classic' % (h, w), 'fwd', s, {'fam': 'patch', 'bn': 64, 'epi': 3}, knobs={0: -2, 5: -1, 10: 0}, patch=pc, bias=True, slope=0.2,
         same=[{0: -1}])
    for grid in (0, 1, 3):
        both('patch', pc, '%dx%d-pers%d' % (h, w, grid), 'fwd', s, {'fam': 'patch-pers', 'bn': 64, 'epi': 3}, knobs={0: -2, 5: grid}, patch=pc, bias=True,
             slope=0.2, same=[{0: -1}])
    # 128-wide tile, ragged in N, data gradient with the activation mask
    both('patch', pc, '%dx%d-wide-dgrad' % (h, w), 'dgrad', (2, 136, h, w, 32, 3, 1, 1), {'fam': 'patch-pers', 'bn': 128, 'epi': {'bf16x3': 32, 'half': -1}},
         knobs={0: -2, 5: 3}, patch=pc, actmask=True, slope=0.2, same=[{0: -1}], half=pc == 'ragged-both')
_P = (13, 14)                                         # ragged in both directions
for cdst in (64, 72, 128, 136, 192, 320):
    bn = 128 if cdst >= 128 else 64
    both('patch', 'cdst', 'c%d-onetile' % cdst, 'fwd', (2, 64, _P[0], _P[1], cdst, 3, 1, 1), {'fam': 'patch', 'bn': bn, 'epi': 0},
         knobs={0: -2, 5: -1, 10: 0}, same=[{0: -1}])
    both('patch', 'cdst', 'c%d-pers' % cdst, 'fwd', (2, 64, _P[0], _P[1], cdst, 3, 1, 1), {'fam': 'patch-pers', 'bn': bn, 'epi': 1}, knobs={0: -2, 5: 3},
         bias=True, same=[{0: -1}])
for csrc in (16, 32, 48, 64):
    even = csrc % 32 == 0                              # the K-split form and the persistent walk need an even number of 16-channel chunks
    both('patch', 'csrc', 'x%d-ks' % csrc, 'fwd', (2, csrc, _P[0], _P[1], 72, 3, 1, 1), {'fam': 'patch-ks' if even else 'patch', 'bn': 64, 'epi': 0},
         knobs={0: -2, 5: -1}, same=None if even else [{0: -1}])
    both('patch', 'csrc', 'x%d-default' % csrc, 'fwd', (2, csrc, _P[0], _P[1], 72, 3, 1, 1), {'fam': 'patch-pers' if even else 'patch', 'bn': 64, 'epi': 4},
         knobs={0: -2, 10: 0}, residual=True, same=[{0: -1}])
    both('patch', 'csrc', 'x%d-wide' % csrc, 'fwd', (2, csrc, _P[0], _P[1], 136, 3, 1, 1), {'fam': 'patch', 'bn': 128, 'epi': 1}, knobs={0: -2, 5: -1},
         bias=True, same=[{0: -1}])
for name, epi, o in (('epi0', 0, {}), ('epi1', 1, dict(bias=True)), ('epi3', 3, dict(bias=True, slope=0.2)), ('epi4', 4, dict(residual=True))):
    both('patch', 'epilogues', name + '-ks', 'fwd', (2, 32, 9, 20, 72, 3, 1, 1), {'fam': 'patch-ks', 'bn': 64, 'epi': epi if epi != 3 else -1},
         knobs={0: -2, 5: -1}, **o)
    both('patch', 'epilogues', name + '-wide', 'fwd', (2, 32, 9, 20, 136, 3, 1, 1), {'fam': 'patch', 'bn': 128, 'epi': epi}, knobs={0: -2, 5: -1},
         same=[{0: -1}], **o)
both('patch', 'epilogues', 'epi32-dgrad-classic', 'dgrad', (2, 72, 9, 20, 32, 3, 1, 1), {'fam': 'patch', 'bn': 64, 'epi': 32}, knobs={0: -2, 5: -1, 10: 0},
     actmask=True, slope=0.2, same=[{0: -1}])
both('patch', 'epilogues', 'epi32-dgrad-ks', 'dgrad', (2, 72, 9, 20, 32, 3, 1, 1), {'fam': 'patch-ks', 'bn': 64, 'epi': -1}, knobs={0: -2, 5: -1},
     actmask=True, slope=0.2)
for grid in (1, 3):
    both('patch', 'pers-grid', 'wide-grid%d' % grid, 'fwd', (3, 64, 9, 20, 192, 3, 1, 1), {'fam': 'patch-pers', 'bn': 128, 'epi': 0}, knobs={0: -2, 5: grid},
         same=[{0: -1}, {0: -2, 5: -1}])
both('patch', 'ks-off', 'x16-declines', 'fwd', (3, 16, 9, 20, 64, 3, 1, 1), {'fam': 'patch', 'bn': 64, 'epi': 1}, knobs={0: -2}, bias=True, same=[{0: -1}],
     note='16 source channels: the K-split form and the persistent walk both decline, the classic one-tile kernel runs')

# ================================================================================================================================ #
# narrow kernel: <= 4 destination channels, M >= 65536; one sample short it is another family's
# ================================================================================================================================ #
NARROW = 'M >= 65536 on images below 16 x 16 needs n above 64'
for cdst, csrc, (h, w) in ((2, 16, (15, 13)), (3, 64, (9, 14)), (4, 16, (13, 15))):
    n = -(-65536 // (h * w))
    nd = 3 if cdst == 3 else 4
    both('narrow', 'over-threshold', 'c%d-%dx%d' % (cdst, h, w), 'fwd', (n, csrc, h, w, cdst, 3, 1, 1), {'fam': 'narrow', 'bn': nd}, bias=True,
         slope=0.2 if cdst == 3 else None, big_n=NARROW, half=cdst == 3)
    both('narrow', 'under-threshold', 'c%d-%dx%d-short' % (cdst, h, w), 'fwd', (n - 1, csrc, h, w, cdst, 3, 1, 1), {'fam': 'reg', 'tile': '128x32'}, bias=True,
         big_n=NARROW, expect_by_mode=True)

# ================================================================================================================================ #
# dot kernel: one destination channel
# ================================================================================================================================ #
for M, (n, h, w), csrc in ((1, (1, 1, 1), 16), (3, (1, 1, 3), 48), (4, (1, 2, 2), 512), (5, (1, 5, 1), 16)):
    both('dot', 'M-edge', 'M%d-x%d' % (M, csrc), 'fwd', (n, csrc, h, w, 1, 3, 1, 1), {'fam': 'dot'}, bias=M % 2 == 1, big_c='the dot kernel at 512 source channels' if csrc > 320 else None,
         half=M == 5)
both('dot', 'csrc', 'x48-k1', 'fwd', (2, 48, 3, 5, 1, 1, 1, 0), {'fam': 'dot'}, bias=True)
both('dot', 'csrc', 'x512-k1', 'fwd', (2, 512, 3, 5, 1, 1, 1, 0), {'fam': 'dot'}, big_c='the dot kernel at 512 source channels')
both('dot', 'row-stride', 'ldx52-slice', 'fwd_ld', (2, 48, 3, 5, 1, 3, 1, 1), {'fam': 'dot'}, ldx=52, ldy=8, yoff=4, bias=True,
     note='a source row stride that is no multiple of 4 is refused by srhip_conv2d_fwd before any routing (tests/test_conv_geometry_cpu.py pins the refusal), so '
          'the dot kernel\'s own lds % 4 test cannot decline a call from outside; the nearest runnable case is a strided source and a destination slice, '
          'which the dot kernel takes.  A one-channel call that leaves the dot kernel (residual) is k32 / cdst1-residual.')

# ================================================================================================================================ #
# legacy generic kernels: source channels % 16 != 0 or k > 5
# ================================================================================================================================ #
LEG = {'fam': 'legacy'}
for i, (cin, k, cout, (h, w)) in enumerate(((1, 3, 1, (1, 1)), (2, 7, 3, (2, 3)), (3, 3, 4, (7, 5)), (5, 7, 5, (7, 5)), (17, 3, 64, (2, 3)), (3, 7, 65, (7, 5)),
                                            (16, 7, 64, (7, 5)))):
    both('legacy', 'cin-k-cout' if i > 1 else 'tiny-images', 'x%d-k%d-c%d-%dx%d' % (cin, k, cout, h, w), 'fwd', (3, cin, h, w, cout, k, 1, k // 2), LEG, bias=i % 2 == 0,
         slope=0.2 if i % 3 == 0 else None, half=i == 5)
both('legacy', 'tiny-images', 'x3-k3-c64-1x1', 'fwd', (5, 3, 1, 1, 64, 3, 1, 1), LEG, bias=True)
both('legacy', 'dgrad', 'cout1', 'dgrad', (3, 16, 7, 5, 1, 3, 1, 1), LEG)
both('legacy', 'dgrad', 'cout3-k7', 'dgrad', (3, 5, 2, 3, 3, 7, 1, 3), LEG)
both('legacy', 'dgrad', 'cout3-1x1', 'dgrad', (5, 64, 1, 1, 3, 3, 1, 1), LEG)

# ================================================================================================================================ #
# dilated gather / scatter around a dense inner conv (3 x 3, pad = dilation)
# ================================================================================================================================ #
# the inner conv of these sizes: 16 -> 48 forward runs the exact-fp32 register tile in every mode (a small launch above 32 destination channels),
# the data gradient (16 destination channels) the <= 32-channel kernel and the weight gradient the LDS-DMA kernel, both in the mode's arithmetic
DIL_GRAD = {'fp32': 'fp32', 'bf16x3': 'bf16x3', 'half': 'bf16'}
for d in (2, 3):
    for (h, w) in ((1, 1), (1, 4), (2, 2), (5, 7)):
        tag = 'd%d-%dx%d' % (d, h, w)
        s = (2, 16, h, w, 48, 3, 1, d)
        for mode in ('bf16x3', 'fp32') + (('half',) if (d, h, w) == (3, 5, 7) else ()):
            add('dil', 'fwd', tag + '-fwd', 'dil_fwd', mode, s, {'fam': 'dil-gather', 'bn': d}, expect='fp32', d=d, bias=True, slope=0.2, guard=True, route2={'fam': 'dil-scatter'})
            add('dil', 'dgrad', tag + '-dgrad', 'dil_dgrad', mode, s, {'fam': 'dil-scatter', 'bn': d}, expect=DIL_GRAD[mode], d=d, guard=True, route2={'fam': 'dil-gather'})
            add('dil', 'dgrad-accumulate', tag + '-dgrad-acc', 'dil_dgrad', mode, s, {'fam': 'dil-scatter', 'bn': d}, expect=DIL_GRAD[mode], d=d, guard=True, accumulate=True)
            add('dil', 'wgrad', tag + '-wgrad', 'dil_wgrad', mode, s, {'fam': 'dil-gather', 'bn': d}, expect={'bf16x3': 'bf16x3', 'fp32': 'fp32', 'half': 'bf16'}[mode],
                d=d, bias=True)
    for mode in ('bf16x3', 'fp32'):
        add('dil', 'wide-rows', 'd%d-5x7-fwd-ld' % d, 'dil_fwd', mode, (2, 16, 5, 7, 48, 3, 1, d), {'fam': 'dil-gather', 'bn': d}, expect='fp32', d=d, bias=True, guard=True,
            ldx=24, ldy=52)
        add('dil', 'wide-rows', 'd%d-5x7-dgrad-ld' % d, 'dil_dgrad', mode, (2, 16, 5, 7, 48, 3, 1, d), {'fam': 'dil-scatter', 'bn': d}, expect=DIL_GRAD[mode], d=d, guard=True,
            ldx=20, ldy=56, accumulate=True)
        add('dil', 'wide-rows', 'd%d-5x7-wgrad-ld' % d, 'dil_wgrad', mode, (2, 16, 5, 7, 48, 3, 1, d), {'fam': 'dil-gather', 'bn': d}, expect=mode, d=d, bias=True,
            ldx=24, ldy=52)

# ================================================================================================================================ #
# weight gradient: row-tap kernel, both forms (Cout >= 128 with Cin % 64; Cout = 64 with Cin % 128)
# ================================================================================================================================ #
def rowtap(form, rem=None, **kw):
    r = {'fam': 'rowtap', 'tile': '128x192' if form == 1 else '64x384', 'math': {'bf16x3': 1, 'half': 2}}
    if rem is not None:
        r['bn'] = rem                                 # the paired-tail remainder the launch ran with (0: no paired tails)
    return dict(r, **kw)


def _rem(wo, ho):
    r = wo & 15
    return r if (0 < r <= 8 and wo >= 16 and ho >= 2) else 0


_i = 0
for wo in (1, 8, 15, 16, 17, 24, 25, 31, 33):
    for ho in (1, 2, 3):
        n = (1, 2, 3)[_i % 3]                          # N * Ho odd and even
        form = 1 + _i % 2
        cin, cout = ((64, 128), (128, 64), (192, 132), (256, 64), (64, 192), (128, 64))[_i % 6]
        _i += 1
        both('rowtap', 'wo-ho', 'wo%d-ho%d-n%d-f%d' % (wo, ho, n, form), 'wgrad', (n, cin, ho, wo, cout, 3, 1, 1), rowtap(form, _rem(wo, ho)), bias=_i % 2 == 0,
             half=(wo, ho) == (25, 3))
        if _rem(wo, ho):
            both('rowtap', 'tails-off', 'wo%d-ho%d-n%d-f%d-knob9' % (wo, ho, n, form), 'wgrad', (n, cin, ho, wo, cout, 3, 1, 1), rowtap(form, 0), knobs={1: 9},
                 bias=True)
for cout, cin in ((128, 64), (132, 192), (192, 64), (320, 64), (64, 128), (64, 256)):
    both('rowtap', 'cout-cin', 'c%dx%d' % (cout, cin), 'wgrad', (2, cin, 3, 24, cout, 3, 1, 1), rowtap(2 if cout == 64 else 1, 8), bias=True)
both('rowtap', 'tails-off', 'wo40-knob9', 'wgrad', (2, 64, 5, 40, 128, 3, 1, 1), rowtap(1, 0), knobs={1: 9}, bias=True)
both('rowtap', 'accumulate', 'acc-c132', 'wgrad', (3, 64, 3, 25, 132, 3, 1, 1), rowtap(1, 0), accumulate=True, bias=True, guard=True)
both('rowtap', 'accumulate', 'acc-c64', 'wgrad', (2, 128, 2, 24, 64, 3, 1, 1), rowtap(2, 8), accumulate=True, bias=True, guard=True)
# P = 10 * 13 * 16 = 2080 pixels = 130 chunks of 16: at most ceil(130 / 16) = 9 splits of >= 16 chunks, rounded up to a multiple of 8 = 16 splits
# of 9 chunks; 15 of them hold the 130 chunks and the last one is empty (it must write zeros).  One pixel column more and the row has a tail.
both('rowtap', 'empty-splits', 'p2080', 'wgrad', (10, 64, 13, 16, 128, 3, 1, 1), rowtap(1, 0, nsplit=16, cps=9), bias=True)
both('rowtap', 'empty-splits', 'p2210-tail', 'wgrad', (10, 128, 13, 17, 64, 3, 1, 1), rowtap(2, 1, nsplit=16), bias=True)
# grouped launches: 8 x 32 x 32 pixels plan 32 splits, so 2, 3 and 4 problems share a launch with 16, 8 and 8 splits each.  (The code documents
# no bit-identity between a grouped and a single launch -- the split counts differ --, so every problem is held to the emulation.)
for nprob in (2, 3, 4):
    both('rowtap', 'multi', 'multi%d' % nprob, 'wgrad_multi', (8, 64, 32, 32, 128, 3, 1, 1), rowtap(1, 0, phases=nprob, nsplit=(16, 8, 8)[nprob - 2]), nprob=nprob,
         guard=True, multi_ok=4, half=nprob == 3)
both('rowtap', 'multi', 'multi-declined', 'wgrad', (1, 64, 9, 17, 128, 3, 1, 1), rowtap(1, 1, phases=0, nsplit=1), accumulate=True, bias=True, guard=True, multi_ok=0,
     note='multi_nsplit returns 0 (one split: nothing to share): srhip_conv2d_wgrad_multi_ok says 0 and the step accumulates with single launches, as this row does')

# ================================================================================================================================ #
# weight gradient: LDS-DMA tiles
# ================================================================================================================================ #
WMATH = {'fp32': 0, 'bf16x3': 1, 'half': 2}
#        tile: (knob 1, Cout at bm, Cin, k) -- what plan_fast_wgrad gives that tile; None where a mode's heuristic differs
#        the tile's own (knob 1, Cout, Cin, k) and the tiles Cout - 4 and Cout + 4 land on (plan_fast_wgrad: bm from Cout, bn from Ktot % 128)
WDMA_TILES = (('256x64', 5, 256, 64, 1, ('128x64', '128x64')), ('64x256', 5, 64, 256, 1, ('64x128', '128x128')), ('128x128', 0, 128, 128, 1, ('128x128', '128x128')),
              ('128x64', 0, 128, 16, 3, ('128x64', '128x64')), ('64x128', 0, 64, 128, 1, ('64x128', '128x128')), ('64x64', 0, 64, 16, 3, ('64x64', '128x64')))
_PS = {1: (1, 1, 1), 15: (1, 3, 5), 16: (1, 4, 4), 17: (1, 1, 17), 255: (5, 3, 17), 257: (257, 1, 1)}
for ti, (tile, knob, cout, cin, k, (below, above)) in enumerate(WDMA_TILES):
    for j, (co, t) in enumerate(((cout - 4, below), (cout, tile), (cout + 4, above))):
        P = (1, 15, 16, 17, 255, 257)[(j + 2 * ti) % 6]
        n, h, w = _PS[P]
        s = (n, cin, h, w, co, 1, 1, 0) if k == 1 else (n, cin, h, w, co, 3, 1, 1)
        both('wdma', 'cout-edge', '%s-c%d-P%d' % (tile, co, P), 'wgrad', s, {'fam': 'wdma', 'math': WMATH, 'tile': t}, knobs={1: knob} if knob else None, bias=j != 1,
             big_n=BIG_N if n > 64 else None)
for i, (cin, k, s_, p_, (h, w)) in enumerate(((16, 1, 1, 0, (3, 5)), (48, 3, 1, 1, (3, 5)), (16, 4, 2, 1, (9, 11)), (48, 5, 1, 2, (5, 7)), (48, 1, 1, 0, (1, 1)))):
    both('wdma', 'cin-k', 'x%d-k%d' % (cin, k), 'wgrad', (2, cin, h, w, (68, 100, 36, 132, 64)[i], k, s_, p_), {'fam': 'wdma', 'math': WMATH}, bias=i % 2 == 0,
         half=i == 2)
for P, (n, h, w) in ((1, (1, 1, 1)), (15, (1, 3, 5)), (16, (1, 4, 4)), (17, (1, 17, 1)), (255, (5, 17, 3)), (257, (257, 1, 1))):
    both('wdma', 'P-edge', 'P%d' % P, 'wgrad', (n, 48, h, w, 100, 3, 1, 1), {'fam': 'wdma', 'math': WMATH}, bias=True, big_n=BIG_N if n > 64 else None)
    add('wdma', 'P-edge', 'P%d-bk32' % P, 'wgrad', 'fp32', (n, 16, h, w, 64, 3, 1, 1), {'fam': 'wdma', 'tile': '64x64', 'bn': 32, 'math': 0}, knobs={1: 3},
        bias=True, big_n=BIG_N if n > 64 else None)      # 32-pixel K chunks exist in exact fp32 only
both('wdma', 'P-edge', 'P2080-empty-split', 'wgrad', (10, 16, 13, 16, 64, 3, 1, 1), {'fam': 'wdma', 'math': WMATH, 'tile': '64x64', 'nsplit': 16}, bias=True)
both('wdma', 'stride2-odd', 's2-9x11', 'wgrad', (3, 16, 9, 11, 132, 3, 2, 1), {'fam': 'wdma', 'math': WMATH}, bias=True)
both('wdma', 'stride2-odd', 's2-7x5-k4', 'wgrad', (3, 48, 7, 5, 64, 4, 2, 1), {'fam': 'wdma', 'math': WMATH}, bias=True)
both('wdma', 'no-bias', 'nobias', 'wgrad', (2, 48, 5, 7, 100, 3, 1, 1), {'fam': 'wdma', 'math': WMATH})
both('wdma', 'no-bias', 'reduce-scalar', 'wgrad', (2, 48, 5, 7, 100, 3, 1, 1), {'fam': 'reduce-scalar'}, knobs={1: 8}, bias=True, same=[{}],
     note='srhip_debug_set(1, 8): the scalar split-K reduce, bit-identical to the vectorised one')
both('wdma', 'no-bias', 'reduce-generic', 'wgrad', (2, 48, 5, 7, 100, 3, 1, 1), {'fam': 'reduce-scalar'}, knobs={1: 6}, bias=True, same=[{}])

# ================================================================================================================================ #
# weight gradient: the attention tail's 64 -> 64 1 x 1 conv with both operand scales; register kernel; legacy kernels
# ================================================================================================================================ #
_j = 0
for hw, (h, w) in ((1, (1, 1)), (2, (1, 2)), (63, (7, 9)), (64, (8, 8)), (65, (5, 13)), (129, (3, 43))):
    for n in (1, 3, 257):
        if n == 257 and hw not in (1, 65):
            continue                                  # n = 257 (more images than one-block-per-CU splits) at the smallest and at a ragged size
        _j += 1
        both('tail1x1', 'hw-n', 'hw%d-n%d' % (hw, n), 'wgrad', (n, 64, h, w, 64, 1, 1, 0), {'fam': 'tail1x1', 'tile': '64x64'}, xrow=True, xchan=True, bias=_j % 2 == 0,
             big_n='n = 257 is the class' if n > 64 else None, half=(hw, n) == (65, 3))
both('tail1x1', 'workspace-short', 'ws-1', 'wgrad', (3, 64, 5, 13, 64, 1, 1, 0), {'fam': 'wreg'}, xrow=True, xchan=True, bias=True, ws_short=True,
     note='workspace one byte short of the pixel-contraction kernel\'s need: the register kernel runs')
for P, (n, h, w) in ((1, (1, 1, 1)), (17, (1, 1, 17))):
    both('wreg', 'P-edge', 'xscale-P%d' % P, 'wgrad', (n, 16, h, w, 68, 3, 1, 1), {'fam': 'wreg'}, xrow=True, xchan=True, bias=True)
    both('wreg', 'P-edge', 'knob10-P%d' % P, 'wgrad', (n, 48, h, w, 64, 1, 1, 0), {'fam': 'wreg'}, knobs={1: 10}, bias=True)
    both('wlegacy', 'P-edge', 'P%d' % P, 'wgrad', (n, 3, h, w, 5, 7, 1, 3), {'fam': 'wlegacy'}, bias=True)
both('wreg', 'ragged', 'xchan-7x5', 'wgrad', (3, 48, 7, 5, 132, 3, 1, 1), {'fam': 'wreg'}, xchan=True, bias=True, half=True)
both('wreg', 'ragged', 'knob11-s2-9x11', 'wgrad', (2, 16, 9, 11, 100, 3, 2, 1), {'fam': 'wreg', 'tile': '128x64'}, knobs={1: 11}, bias=True)
both('wlegacy', 'ragged', 'x1-c1-7x5', 'wgrad', (3, 1, 7, 5, 1, 7, 1, 3), {'fam': 'wlegacy'}, bias=True, half=True)
both('wlegacy', 'ragged', 'x3-c3-2x3', 'wgrad', (3, 3, 2, 3, 3, 7, 1, 3), {'fam': 'wlegacy'})

IDS = [r['id'] for r in ROWS]
