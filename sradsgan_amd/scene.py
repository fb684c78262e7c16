"""Whole-scene super-resolution: a uint8 HWC raster larger than one training-size tile goes through the generator in
overlapping tiles, and the tiles' outputs are blended with feathered seams into one uint8 HWC scene on the device.

This is an APPROXIMATION of a whole-scene forward: the generators' attention (SGAM / CGAM, HAT's windows) sees one tile
at a time, so neighbouring tiles disagree where they overlap.  The feather hides the seams; it does not remove the
difference.

Geometry (pure Python, `ScenePlan`).  Per axis: scene length L, tile side t' = min(t, L), overlap 0 <= ov < t', stride
s = t' - ov; n = 1 tiles if L == t', else ceil((L - t') / s) + 1; positions p_i = min(i s, L - t') (every tile is full
size, the last one shifts inward).  In HR pixels a_i = p_i scale, T = t' scale, and tile i > 0 overlaps its predecessor
by o_i = a_{i-1} + T - a_i >= 0.  The 1-D weight of tile i at offset q in [0, T) is
    min(1, (q + 1) / (o_i + 1))  [1 for i = 0]   *   min(1, (T - q) / (o_{i+1} + 1))  [1 for the last tile]
computed in fp64 and rounded to fp32, one table per tile and axis.  The 2-D weight is the fp32 product wy * wx; the
blended value is (sum_k w_k sr_k) / (sum_k w_k) over the covering tiles in row-major tile order, in fp32.  Where one tile
alone covers a pixel its weight is 1, so overlap 0 on a scene that is a multiple of the tile is the identity.
Quantisation is save_img1's (utils/utils.py:169-187), as in mfe_test_single: trunc(clamp(255 out, 0, 255)); NaN -> 0.

Memory is bounded by bands, not by the scene: tiles run one tile row at a time in batches of `tiles_per_batch`; a ring
keeps the generator's outputs (no copy: the blend kernel reads them through their strides) of only the tile rows that
still cover un-finalised HR rows -- `ScenePlan.ring_depth`: normally two, more when the overlap exceeds half a tile or
the inward-shifted last row lands close behind its predecessors -- and every band
of HR rows is blended as soon as its last covering tile row is done.  The uint8 output is the only scene-sized buffer.
The only per-tile work outside the generator is two HIP kernels (csrc/scene.hip)."""
import ctypes

import numpy as np
import torch

from . import _hip


class AxisPlan:
    """One axis of the tiling: see the module docstring.  positions / hr_positions / overlaps: per tile; weights:
    float32 [n][hr_tile]; cover: int32 [hr_length][2] = first and one-past-last tile covering an HR coordinate."""

    def __init__(self, length, tile, overlap, scale):
        length, tile, overlap, scale = int(length), int(tile), int(overlap), int(scale)
        if length <= 0 or tile <= 0 or scale <= 0:
            raise ValueError('scene plan: length, tile and scale must be positive (got %d, %d, %d)' % (length, tile, scale))
        if not 0 <= overlap < tile:
            raise ValueError('scene plan: overlap must satisfy 0 <= overlap < tile (got overlap %d, tile %d)' % (overlap, tile))
        t = min(tile, length)
        self.length, self.tile, self.overlap, self.scale = length, t, overlap, scale
        if length == t:
            self.stride, self.n = t, 1
        else:                                       # here t == tile, so the stride is positive
            self.stride = t - overlap
            self.n = -(-(length - t) // self.stride) + 1
        self.positions = [min(i * self.stride, length - t) for i in range(self.n)]
        self.hr_length, self.hr_tile = length * scale, t * scale
        self.hr_positions = [p * scale for p in self.positions]
        a, T = self.hr_positions, self.hr_tile
        self.overlaps = [0] + [a[i - 1] + T - a[i] for i in range(1, self.n)]
        q = np.arange(T, dtype=np.float64)
        self.weights = np.empty((self.n, T), np.float32)
        for i in range(self.n):
            w = np.ones(T, np.float64)
            if i > 0:
                w = w * np.minimum(1.0, (q + 1.0) / (self.overlaps[i] + 1.0))
            if i + 1 < self.n:
                w = w * np.minimum(1.0, (T - q) / (self.overlaps[i + 1] + 1.0))
            self.weights[i] = w.astype(np.float32)
        self.cover = np.empty((self.hr_length, 2), np.int32)
        lo = hi = 0
        for y in range(self.hr_length):             # positions increase strictly, so the covering tiles are contiguous
            while a[lo] + T <= y:
                lo += 1
            while hi < self.n and a[hi] <= y:
                hi += 1
            self.cover[y] = (lo, hi)


class ScenePlan:
    """Tiling of an h x w scene (LR pixels) for a x`scale` generator.  ys / xs: AxisPlan per axis; th / tw: LR tile
    sides; row_final[j] = (r0, r1): the HR rows that are complete once tile row j is done (they partition [0, hr_h));
    ring_depth: how many consecutive tile rows have to be held to blend every such band."""

    def __init__(self, h, w, scale, tile, overlap):
        self.h, self.w, self.scale = int(h), int(w), int(scale)
        self.ys, self.xs = AxisPlan(h, tile, overlap, scale), AxisPlan(w, tile, overlap, scale)
        self.th, self.tw = self.ys.tile, self.xs.tile
        self.hr_h, self.hr_w = self.ys.hr_length, self.xs.hr_length
        a, T, n = self.ys.hr_positions, self.ys.hr_tile, self.ys.n
        self.row_final = [(a[j], a[j + 1] if j + 1 < n else self.hr_h) for j in range(n)]
        self.ring_depth = max(sum(1 for k in range(j + 1) if a[k] + T > a[j]) for j in range(n))

    def origins(self, j):
        """LR (y, x) origins of tile row j, left to right."""
        return [(self.ys.positions[j], x) for x in self.xs.positions]


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _require_scene(scene_u8, what):
    if not torch.is_tensor(scene_u8):
        scene_u8 = torch.as_tensor(np.asarray(scene_u8))
    if scene_u8.dtype != torch.uint8:
        raise ValueError('%s: the scene must be uint8, got %s' % (what, scene_u8.dtype))
    if scene_u8.dim() != 3 or scene_u8.shape[2] != 3 or scene_u8.shape[0] == 0 or scene_u8.shape[1] == 0:
        raise ValueError('%s: the scene must be [H, W, 3] (HWC), got %s' % (what, tuple(scene_u8.shape)))
    return scene_u8


def extract_tiles(scene_u8, origins, th, tw):
    """scene_u8: [H, W, 3] uint8 on the HIP device; origins: [(y, x), ...] in pixels.  Returns float32 [n, 3, th, tw]
    (channels_last memory), tile k bit-identical to data.to_tensor(scene_u8[y:y+th, x:x+tw][None])."""
    scene_u8 = _require_scene(scene_u8, 'extract_tiles')
    if not scene_u8.is_cuda:
        raise RuntimeError('extract_tiles: runs on the MI355X HIP path only (got a %s tensor); there is no CPU fallback'
                           % scene_u8.device.type)
    h, w = scene_u8.shape[:2]
    origins = [(int(y), int(x)) for y, x in origins]
    if not origins:
        raise ValueError('extract_tiles: no tile origins')
    for y, x in origins:
        if not (0 <= y <= h - th and 0 <= x <= w - tw):
            raise ValueError('extract_tiles: tile %dx%d at (%d, %d) leaves the %dx%d scene' % (th, tw, y, x, h, w))
    scene_u8 = scene_u8.contiguous()
    org = torch.tensor(origins, dtype=torch.int32).to(scene_u8.device)
    out = torch.empty(len(origins), th, tw, 3, device=scene_u8.device, dtype=torch.float32)
    _hip.check(_hip.lib().srhip_scene_tiles_u8(_p(scene_u8), h, w, _p(org), len(origins), th, tw, _p(out), _stream()),
               'scene_tiles_u8')
    return out.permute(0, 3, 1, 2)


class SceneBlender:
    """The band ring.  push_row(chunks) takes the float SR tiles of the next tile row, left to right, as one or more
    [k, 3, T, T] tensors (the generator's outputs, kept alive here instead of copied), and blends the HR rows that row
    finalises into `out` (uint8 [hr_h, hr_w, 3]) and, with float_out, `out_f32` (the un-quantised fp32 blend)."""

    def __init__(self, plan, device, ring_depth=None, float_out=False):
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('SceneBlender: runs on the MI355X HIP path only (got device %s); there is no CPU fallback' % device)
        self.plan, self.device = plan, device
        self.depth = plan.ring_depth if ring_depth is None else int(ring_depth)
        if self.depth < plan.ring_depth:
            raise ValueError('SceneBlender: this plan needs a ring of %d tile rows, got %d' % (plan.ring_depth, self.depth))
        self.out = torch.empty(plan.hr_h, plan.hr_w, 3, device=device, dtype=torch.uint8)
        self.out_f32 = torch.empty(plan.hr_h, plan.hr_w, 3, device=device, dtype=torch.float32) if float_out else None

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self._ycover, self._xcover = up(plan.ys.cover), up(plan.xs.cover)
        self._ay, self._ax = up(np.asarray(plan.ys.hr_positions, np.int32)), up(np.asarray(plan.xs.hr_positions, np.int32))
        self._wy, self._wx = up(plan.ys.weights), up(plan.xs.weights)
        self._ring = [None] * self.depth                                   # tensors of the resident tile rows
        self._ptrs = np.zeros((self.depth, plan.xs.n), np.int64)
        self._strides = None
        self.rows_done = 0

    def _conform(self, sr):
        T_h, T_w = self.plan.ys.hr_tile, self.plan.xs.hr_tile
        if not (torch.is_tensor(sr) and sr.is_cuda and sr.dtype == torch.float32):
            raise TypeError('SceneBlender: SR tiles must be float32 tensors on the HIP device')
        if sr.dim() != 4 or tuple(sr.shape[1:]) != (3, T_h, T_w):
            raise ValueError('SceneBlender: SR tiles must be [k, 3, %d, %d] (tile x scale), got %s' % (T_h, T_w, tuple(sr.shape)))
        st = tuple(sr.stride()[1:])
        if self._strides is None:
            if st not in ((T_h * T_w, T_w, 1), (1, 3 * T_w, 3)):           # neither NCHW-dense nor channels_last: densify once
                sr = sr.contiguous()
                st = tuple(sr.stride()[1:])
            self._strides = st
        elif st != self._strides:                                           # one stride triple serves the whole ring
            buf = torch.empty_strided(tuple(sr.shape), (3 * T_h * T_w,) + self._strides, device=sr.device, dtype=sr.dtype)
            sr = buf.copy_(sr)
        return sr

    def push_row(self, chunks):
        plan, j = self.plan, self.rows_done
        if j >= plan.ys.n:
            raise ValueError('SceneBlender: all %d tile rows were already pushed' % plan.ys.n)
        chunks = [self._conform(c) for c in chunks]
        if sum(c.shape[0] for c in chunks) != plan.xs.n:
            raise ValueError('SceneBlender: tile row %d needs %d tiles, got %d' % (j, plan.xs.n, sum(c.shape[0] for c in chunks)))
        slot, i = j % self.depth, 0
        for c in chunks:
            for k in range(c.shape[0]):
                self._ptrs[slot, i] = c.data_ptr() + 4 * k * c.stride(0)
                i += 1
        self._ring[slot] = chunks                                           # drops the tile row that no band needs any more
        ptrs = torch.from_numpy(self._ptrs).to(self.device)                 # a fresh table per launch: nothing in flight reads it
        sc, sy, sx = self._strides
        r0, r1 = plan.row_final[j]
        _hip.check(_hip.lib().srhip_scene_blend_u8(
            _p(ptrs), self.depth, sc, sy, sx, _p(self._ycover), _p(self._xcover), _p(self._ay), _p(self._ax), _p(self._wy),
            _p(self._wx), plan.ys.n, plan.xs.n, plan.ys.hr_tile, plan.xs.hr_tile, plan.hr_h, plan.hr_w, r0, r1, _p(self.out),
            _p(self.out_f32) if self.out_f32 is not None else None, _stream()), 'scene_blend_u8')
        self.rows_done += 1
        if self.rows_done == plan.ys.n:
            self._ring = [None] * self.depth


def run_plan(plan, scene_u8, tile_fn, tiles_per_batch=16, ring_depth=None, float_out=False):
    """The driver under super_resolve_scene: scene_u8 [H, W, 3] uint8 on the device; tile_fn maps a float LR batch
    [k, 3, th, tw] to its SR batch [k, 3, th scale, tw scale].  Returns the SceneBlender (out, out_f32)."""
    tiles_per_batch = int(tiles_per_batch)
    if tiles_per_batch < 1:
        raise ValueError('tiles_per_batch must be at least 1, got %d' % tiles_per_batch)
    blender = SceneBlender(plan, scene_u8.device, ring_depth=ring_depth, float_out=float_out)
    for j in range(plan.ys.n):
        origins = plan.origins(j)
        blender.push_row([tile_fn(extract_tiles(scene_u8, origins[c:c + tiles_per_batch], plan.th, plan.tw))
                          for c in range(0, len(origins), tiles_per_batch)])
    return blender


def super_resolve_scene(generator, scene_u8, scale, tile, overlap, tiles_per_batch=16):
    """scene_u8: uint8 [H, W, 3] at the generator's input resolution, host or device (a numpy array is accepted too).
    Returns the super-resolved scene, uint8 [H scale, W scale, 3], on the generator's device.  `tile` is the LR tile
    side, `overlap` the LR overlap of neighbouring tiles.  A generator's own refusal passes through, and one that returns
    anything but [k, 3, tile scale, tile scale] -- HAT pads a tile that is no multiple of its window and returns the padded
    size -- is refused with ValueError: nothing is padded or cropped silently.  The generator runs in eval() under
    no_grad; its training mode is restored afterwards.  Tiling approximates a whole-scene forward (module docstring)."""
    scene_u8 = _require_scene(scene_u8, 'super_resolve_scene')
    if int(tile) <= 0 or not 0 <= int(overlap) < int(tile):
        raise ValueError('super_resolve_scene: needs 0 <= overlap < tile (got overlap %s, tile %s)' % (overlap, tile))
    if int(tiles_per_batch) < 1:
        raise ValueError('super_resolve_scene: tiles_per_batch must be at least 1, got %s' % tiles_per_batch)
    plan = ScenePlan(scene_u8.shape[0], scene_u8.shape[1], scale, tile, overlap)
    from . import ops
    param = next(iter(generator.parameters()), None)
    if param is None:
        raise ValueError('super_resolve_scene: the generator has no parameters to tell its device from')
    ops._require_gpu(param, 'super_resolve_scene')
    scene_u8 = scene_u8.to(param.device).contiguous()
    was_training = generator.training
    generator.eval()
    try:
        with torch.no_grad():
            blender = run_plan(plan, scene_u8, generator, tiles_per_batch)
    finally:
        generator.train(was_training)
    return blender.out


def evaluate_scene(generator, hr_scene_u8, scale, tile, overlap, crop_border=None, y_channel=True, tiles_per_batch=16):
    """The papers' evaluation of a whole ground-truth scene: hr_scene_u8, uint8 [H, W, 3] with H and W multiples of `scale` (host or
    device), is reduced by `scale` with data.resize_u8 (Pillow-exact bicubic), super-resolved by super_resolve_scene(generator, LR,
    scale, tile, overlap, tiles_per_batch) and compared with the scene by metrics.published_metrics_u8(crop_border, y_channel);
    crop_border None = scale.  The same metrics are computed for the bicubic enlargement of the LR scene.
    Returns {'sr': {mse, psnr, ssim}, 'bicubic': {mse, psnr, ssim}, 'out': the uint8 SR scene}, metric values float64 [1] on the device."""
    from . import data as sdata, metrics as pub, ops
    hr = _require_scene(hr_scene_u8, 'evaluate_scene')
    scale = int(scale)
    if scale <= 0 or hr.shape[0] % scale or hr.shape[1] % scale:
        raise ValueError('evaluate_scene: the HR scene %dx%d is not a multiple of scale %d' % (hr.shape[0], hr.shape[1], scale))
    crop_border = scale if crop_border is None else crop_border
    param = next(iter(generator.parameters()), None)
    if param is None:
        raise ValueError('evaluate_scene: the generator has no parameters to tell its device from')
    ops._require_gpu(param, 'evaluate_scene')
    hr = hr.to(param.device).contiguous()
    h, w = hr.shape[:2]
    lr = sdata.resize_u8(hr[None], h // scale, w // scale, 'bicubic')
    out = super_resolve_scene(generator, lr[0], scale, tile, overlap, tiles_per_batch)
    bicubic = sdata.resize_u8(lr, h, w, 'bicubic')[0]
    return {'sr': pub.published_metrics_u8(out, hr, crop_border, y_channel),
            'bicubic': pub.published_metrics_u8(bicubic, hr, crop_border, y_channel), 'out': out}
