"""The reference's blur-and-noise degradation (SRADSGAN/model/util.py:237-492) for training batches that are already on the
device: one random isotropic or anisotropic Gaussian kernel per sample (BatchSRKernel), a reflection-padded per-sample blur
(BatchBlur), Pillow's 8-bit bicubic down-sampling (b_CPUVar_Bicubic) and per-sample Gaussian noise (random_batch_noise,
b_GaussianNoising), wrapped as SRMDPreprocessing / BlurPreprocessing.  The reference writes degraded LR folders with it, image by
image on the CPU; here it sits in the training loop: blur (csrc/degrade.hip), resample (csrc/resample.hip) and noise are three
kernels on uint8 tiles, the kernels and noise levels are drawn on the host and go up through pinned memory without a wait.

The blur's summation order is fixed (include/sradsgan_hip.h, srhip_blur_u8), so the LR bytes equal the reference's for the same
kernels (tests/golden/degrade.npz) and do not depend on the batch a tile sits in.

Differences from the reference, all deliberate:
  * the draws come from a torch.Generator seeded with seed + rank (like data.Augment), the noise from Philox keyed by
    (seed + rank, call number).  The reference draws from numpy's global generator: the distribution is the same, the stream is not;
  * inputs are uint8 [N, H, W, C] device batches, not float CPU tensors; `cuda` is accepted and ignored;
  * `pca_matrix` is optional (without it re_code is None); fitting one (PCA, torch.svd) is not carried over;
  * BlurPreprocessing(..)(x, noise=True) -- noise on the UNquantised blurred floats -- is a NotImplementedError: the noise kernel
    takes the quantised LR bytes, which is what SRMDPreprocessing feeds it;
  * there is no backward through the blur."""
import ctypes
import math

import numpy as np
import torch
import torch.nn as nn

from . import _hip
from . import data as sdata

MAX_KERNEL = 21


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _uniform(generator, n=None):
    """float64 uniforms in [0, 1) from `generator` (None = torch's global one): a Python float, or a numpy array of n."""
    u = torch.rand(() if n is None else (n,), generator=generator, dtype=torch.float64)
    return float(u) if n is None else u.numpy()


def _check_l(l):
    if int(l) != l or not 1 <= int(l) <= MAX_KERNEL:
        raise ValueError('blur kernel size must be an integer in 1..%d, got %r' % (MAX_KERNEL, l))
    return int(l)


# --------------------------------------------------------------------------------------------- #
# kernel generators (util.py:237-303): float64 on the host, cast to fp32 at the end as torch.FloatTensor(...) does there
# --------------------------------------------------------------------------------------------- #

def _axis(l):
    """The tap coordinates np.arange(-l // 2 + 1., l // 2 + 1.): centred for odd l, one further after than before for even l."""
    return np.arange(l, dtype=np.float64) - float((l - 1) // 2)


def _finish(kernel, tensor):
    kernel = kernel / np.sum(kernel)
    return torch.from_numpy(kernel.astype(np.float32)) if tensor else kernel


def cal_sigma(sig_x, sig_y, radians):
    """Covariance U diag(sig_x^2, sig_y^2) U^T of a Gaussian with axis deviations sig_x, sig_y turned by `radians`."""
    d = np.array([[sig_x ** 2, 0.0], [0.0, sig_y ** 2]], dtype=np.float64)
    c, s = np.cos(radians), np.sin(radians)
    u = np.array([[c, -s], [s, c]], dtype=np.float64)
    return np.dot(u, np.dot(d, u.T))


def anisotropic_gaussian_kernel(l, sigma_matrix, tensor=False):
    """l x l Gaussian exp(-v^T S^-1 v / 2) over the tap coordinates v = (column, row), normalised to sum 1."""
    ax = _axis(l)
    xx, yy = np.meshgrid(ax, ax)
    xy = np.stack((xx, yy), axis=2)                                   # [l, l, 2]
    inv = np.linalg.inv(np.asarray(sigma_matrix, dtype=np.float64))
    return _finish(np.exp(-0.5 * np.sum(np.dot(xy, inv) * xy, 2)), tensor)


def isotropic_gaussian_kernel(l, sigma, tensor=False):
    ax = _axis(l)
    xx, yy = np.meshgrid(ax, ax)
    return _finish(np.exp(-(xx ** 2 + yy ** 2) / (2.0 * sigma ** 2)), tensor)


def random_kernel_params(batch, sig_min=0.2, sig_max=4.0, rate_iso=1.0, scaling=3, generator=None):
    """float64 [batch, 4] = (sig_x, sig_y, theta, isotropic) in the reference's order of draws per sample: one uniform against
    rate_iso; isotropic: one for sigma; anisotropic: theta in [-pi, pi), sig_x in [sig_min, sig_max), sig_y = clip(u * scaling *
    sig_x, sig_min, sig_max)."""
    out = np.zeros((batch, 4), dtype=np.float64)
    for b in range(batch):
        if _uniform(generator) < rate_iso:
            sig = _uniform(generator) * (sig_max - sig_min) + sig_min
            out[b] = (sig, sig, 0.0, 1.0)
        else:
            theta = _uniform(generator) * math.pi * 2 - math.pi
            sx = _uniform(generator) * (sig_max - sig_min) + sig_min
            sy = float(np.clip(_uniform(generator) * scaling * sx, sig_min, sig_max))
            out[b] = (sx, sy, theta, 0.0)
    return out


def kernels_from_params(params, l, tensor=True):
    """The [batch, l, l] kernels of random_kernel_params rows."""
    l = _check_l(l)
    out = np.zeros((len(params), l, l), dtype=np.float64)
    for b, (sx, sy, theta, iso) in enumerate(np.asarray(params, dtype=np.float64)):
        out[b] = isotropic_gaussian_kernel(l, sx) if iso else anisotropic_gaussian_kernel(l, cal_sigma(sx, sy, theta))
    return torch.from_numpy(out.astype(np.float32)) if tensor else out


def random_batch_kernel(batch, l=21, sig_min=0.2, sig_max=4.0, rate_iso=1.0, scaling=3, tensor=True, generator=None):
    """One random Gaussian kernel per sample, isotropic with probability rate_iso (util.py:281-296).  Draws come from `generator`
    (a torch.Generator; None = torch's global one), not from numpy's global generator as in the reference: the same
    distribution, another stream."""
    return kernels_from_params(random_kernel_params(batch, sig_min, sig_max, rate_iso, scaling, generator), l, tensor)


def stable_batch_kernel(batch, l=21, sig=2.6, tensor=True):
    """The same isotropic kernel of deviation `sig` for every sample (util.py:299-303)."""
    l = _check_l(l)
    out = np.repeat(isotropic_gaussian_kernel(l, sig)[None], batch, axis=0)
    return torch.from_numpy(out.astype(np.float32)) if tensor else out


def random_batch_noise(batch, high, rate_cln=1.0, generator=None):
    """float64 [batch, 1] noise levels (util.py:334-339): `batch` uniforms times `high`, then `batch` mask uniforms; a sample whose
    mask draw is below rate_cln is clean (level 0).  Draws from `generator`, see random_batch_kernel."""
    level = _uniform(generator, batch) * high
    mask = _uniform(generator, batch)
    return (level * (mask >= rate_cln)).reshape(batch, 1)


# --------------------------------------------------------------------------------------------- #
# kernels on the device
# --------------------------------------------------------------------------------------------- #

def _check_pad(l, h, w):
    if l // 2 >= h or l // 2 >= w:
        raise ValueError('blur: reflection padding %d needs an image larger than it in both axes, got %dx%d (ReflectionPad2d raises '
                         'there too)' % (l // 2, h, w))


def _require_kernels(kernels, n, l, what):
    if not (torch.is_tensor(kernels) and kernels.is_cuda and kernels.dtype == torch.float32 and tuple(kernels.shape) == (n, l, l)):
        raise TypeError('%s: kernels must be a float32 [%d, %d, %d] tensor on the device' % (what, n, l, l))
    return kernels.contiguous()


def blur_u8(img_u8, kernels_dev):
    """img_u8: [N, H, W, C] uint8 on the device, kernels_dev: float32 [N, l, l] on the device -> uint8 [N, H, W, C]: sample k
    cross-correlated with kernel k on the reflection-padded image and quantised like to_pil_image (include/sradsgan_hip.h,
    srhip_blur_u8).  Asynchronous on the current stream."""
    sdata._require_gpu_u8(img_u8, 'blur_u8')
    n, h, w, c = img_u8.shape
    if kernels_dev.dim() != 3 or kernels_dev.shape[1] != kernels_dev.shape[2]:
        raise TypeError('blur_u8: kernels must be [N, l, l], got %s' % (tuple(kernels_dev.shape),))
    l = _check_l(kernels_dev.shape[1])
    _check_pad(l, h, w)
    kernels_dev = _require_kernels(kernels_dev, n, l, 'blur_u8')
    img_u8 = img_u8.contiguous()
    out = torch.empty_like(img_u8)
    _hip.check(_hip.lib().srhip_blur_u8(_p(img_u8), _p(kernels_dev), _p(out), n, h, w, c, l, _stream()), 'blur_u8')
    return out


def degrade_noise_u8(lr_u8, level_dev, z=None, seed=0, step=0):
    """lr_u8: [N, H, W, C] uint8 on the device, level_dev: float32 [N] on the device -> float32 [N, C, H, W] (channels-last memory,
    like data.to_tensor) = clamp(byte / 255 + z * level[n], 0, 1); z: a float32 [N, H, W, C] device tensor or None for the Philox
    normals gdp_kernels.randn_rows(seed, step) writes for the same elements."""
    sdata._require_gpu_u8(lr_u8, 'degrade_noise_u8')
    n, h, w, c = lr_u8.shape
    if not (torch.is_tensor(level_dev) and level_dev.is_cuda and level_dev.dtype == torch.float32 and level_dev.numel() == n):
        raise TypeError('degrade_noise_u8: levels must be a float32 tensor of %d elements on the device' % n)
    if z is not None and not (z.is_cuda and z.dtype == torch.float32 and tuple(z.shape) == (n, h, w, c)):
        raise TypeError('degrade_noise_u8: z must be a float32 [%d, %d, %d, %d] tensor on the device' % (n, h, w, c))
    lr_u8, level_dev = lr_u8.contiguous(), level_dev.contiguous()
    z = None if z is None else z.contiguous()
    out = torch.empty(lr_u8.shape, device=lr_u8.device, dtype=torch.float32)
    _hip.check(_hip.lib().srhip_degrade_noise_u8(_p(lr_u8), _p(level_dev), None if z is None else _p(z), _p(out), n, h, w, c,
                                                 int(z is None), int(seed), int(step), _stream()), 'degrade_noise_u8')
    return out.permute(0, 3, 1, 2)


class BatchBlur(nn.Module):
    """util.py:383-405 on srhip_blur_f32: input float32 [B, C, H, W] on the device (dense NCHW or channels-last; the output keeps the
    input's strides), kernel float32 [l, l] (one for all) or [B, l, l] (one per sample).  Forward only: an input or kernel that
    requires grad is an error."""

    def __init__(self, l=15):
        super().__init__()
        self.l = _check_l(l)

    def forward(self, input, kernel):
        l = self.l
        if not (torch.is_tensor(input) and input.dim() == 4 and input.dtype == torch.float32):
            raise TypeError('BatchBlur expects a float32 [B, C, H, W] tensor')
        b, c, h, w = input.shape
        if not (torch.is_tensor(kernel) and kernel.dtype == torch.float32 and tuple(kernel.shape) in ((l, l), (b, l, l))):
            raise TypeError('BatchBlur(l=%d): the kernel must be float32 [%d, %d] or [%d, %d, %d], got %s'
                            % (l, l, l, b, l, l, tuple(kernel.shape) if torch.is_tensor(kernel) else type(kernel)))
        _check_pad(l, h, w)
        if (input.requires_grad or kernel.requires_grad) and torch.is_grad_enabled():
            raise RuntimeError('BatchBlur has no backward: detach the input and the kernel')
        if not (input.is_cuda and kernel.is_cuda):
            raise RuntimeError('BatchBlur runs on the MI355X HIP path only (got %s / %s tensors); there is no CPU fallback'
                               % (input.device.type, kernel.device.type))
        if any(s < 0 for s in input.stride()) or input.numel() == 0:
            raise ValueError('BatchBlur: empty tensors and negative strides are not taken')
        kernel = kernel.contiguous()
        out = torch.empty_like(input)                     # preserve_format: a dense input's strides, NCHW and channels-last alike
        xs, ys = (ctypes.c_long * 4)(*input.stride()), (ctypes.c_long * 4)(*out.stride())
        _hip.check(_hip.lib().srhip_blur_f32(_p(input), xs, _p(kernel), int(kernel.dim() == 3), _p(out), ys, b, c, h, w, l, _stream()),
                   'blur_f32')
        return out


class _Preprocessing(object):
    """What SRMDPreprocessing and BlurPreprocessing share: the parameters, the host generator and the pinned upload."""

    def __init__(self, scale, random, kernel, sig, sig_min, sig_max, rate_iso, scaling, rate_cln, noise_high, seed, rank):
        self.l = _check_l(kernel)
        self.scale, self.random = scale, bool(random)
        self.sig, self.sig_min, self.sig_max, self.rate_iso, self.scaling = sig, sig_min, sig_max, rate_iso, scaling
        self.rate_cln, self.noise_high = rate_cln, noise_high
        self.generator = torch.Generator()
        self.seed = (self.generator.seed() if seed is None else int(seed) + int(rank)) & 0x7fffffffffffffff
        self.generator.manual_seed(self.seed)
        self.step = 0                                    # Philox step of the next call
        self.last_kernels, self.last_levels, self.last_step = None, None, None

    def draw_kernels(self, n):
        """Host float32 [n, l, l]."""
        if self.random:
            return random_batch_kernel(n, self.l, self.sig_min, self.sig_max, self.rate_iso, self.scaling, True, self.generator)
        return stable_batch_kernel(n, self.l, self.sig)

    def draw_levels(self, n):
        """Host float32 [n]."""
        return torch.from_numpy(random_batch_noise(n, self.noise_high, self.rate_cln, self.generator).astype(np.float32)).reshape(n)

    def _upload(self, device, kernels, levels):
        """The two host tables through ONE pinned buffer on the current stream; nothing waits for the device."""
        n, ll = kernels.shape[0], self.l * self.l
        staged = torch.empty(n * ll + (0 if levels is None else n), dtype=torch.float32, pin_memory=True)
        staged[:n * ll].copy_(kernels.reshape(-1))
        if levels is not None:
            staged[n * ll:].copy_(levels.reshape(-1))
        dev = staged.to(device, non_blocking=True)
        return dev[:n * ll].view(n, self.l, self.l), (None if levels is None else dev[n * ll:])

    def _tables(self, n, kernels, levels, want_levels):
        if kernels is None:
            kernels = self.draw_kernels(n)
        kernels = torch.as_tensor(kernels, dtype=torch.float32).cpu()
        if tuple(kernels.shape) != (n, self.l, self.l):
            raise TypeError('kernels must be [%d, %d, %d], got %s' % (n, self.l, self.l, tuple(kernels.shape)))
        if want_levels:
            levels = self.draw_levels(n) if levels is None else torch.as_tensor(levels, dtype=torch.float32).cpu().reshape(-1)
            if levels.numel() != n:
                raise TypeError('levels must have %d elements, got %d' % (n, levels.numel()))
        else:
            levels = None
        return kernels, levels


class SRMDPreprocessing(_Preprocessing):
    """util.py:408-462 for a uint8 [N, H, W, C] device batch: blur with one kernel per sample (random=True: drawn per call;
    False: the stable isotropic kernel of deviation `sig`), Pillow's bicubic to (int(H / scale), int(W / scale)) on the blurred
    BYTES (the reference goes through to_pil_image too), then, with noise=True, Gaussian noise of a per-sample level in
    [0, noise_high), zero with probability rate_cln.  Returns (lr, re_code) or, with kernel=True, (lr, re_code, kernels): lr float32
    [N, C, h, w] in channels-last memory, kernels float32 [N, l, l] on the device, re_code = kernels.view(N, l * l) @ pca_matrix
    (with the levels * 10 as a last column when noise=True), or None without a pca_matrix.

    The draws come from a torch.Generator seeded seed + rank, the normals from Philox keyed (seed + rank, call number): the
    reference's distribution, not numpy's stream.  `last_kernels` / `last_levels` (host float32) and `last_step` record the latest
    call; `last_lr_u8` is its LR before the noise.  kernels= / levels= / z= replace the draws (tests, replays)."""

    def __init__(self, scale, random, pca_matrix=None, kernel=21, noise=True, cuda=False, sig=2.6, sig_min=0.2, sig_max=4.0,
                 rate_iso=1.0, scaling=3, rate_cln=0.2, noise_high=0.08, seed=None, rank=0):
        super().__init__(scale, random, kernel, sig, sig_min, sig_max, rate_iso, scaling, rate_cln, noise_high, seed, rank)
        self.noise = bool(noise)
        if pca_matrix is not None and (pca_matrix.dim() != 2 or pca_matrix.shape[0] != self.l * self.l):
            raise TypeError('pca_matrix must be [%d, k], got %s' % (self.l * self.l, tuple(pca_matrix.shape)))
        self.pca_matrix = pca_matrix
        self.last_lr_u8 = None

    def __call__(self, hr_u8, kernel=False, kernels=None, levels=None, z=None):
        sdata._require_gpu_u8(hr_u8, 'SRMDPreprocessing')
        n, h, w, _ = hr_u8.shape
        _check_pad(self.l, h, w)
        k_host, lv_host = self._tables(n, kernels, levels, self.noise)                 # 1. draw on the host
        k_dev, lv_dev = self._upload(hr_u8.device, k_host, lv_host)                    # 2. up through pinned memory, no wait
        blurred = blur_u8(hr_u8, k_dev)                                                # 3. per-sample blur on the bytes
        lr_u8 = sdata.resize_u8(blurred, int(h / self.scale), int(w / self.scale), 'bicubic')   # 4. Pillow's bicubic
        if self.noise:                                                                 # 5. noise tail, or to_tensor
            lr = degrade_noise_u8(lr_u8, lv_dev, z, self.seed, self.step)
        else:
            lr = sdata.to_tensor(lr_u8)
        self.last_kernels, self.last_levels, self.last_step, self.last_lr_u8 = k_host, lv_host, self.step, lr_u8
        self.step += 1
        re_code = None
        if self.pca_matrix is not None:
            if self.pca_matrix.device != k_dev.device:
                self.pca_matrix = self.pca_matrix.to(k_dev.device, torch.float32)
            re_code = k_dev.reshape(n, self.l * self.l) @ self.pca_matrix
            if self.noise:
                re_code = torch.cat([re_code, lv_dev.reshape(n, 1) * 10], dim=1)
        return (lr, re_code, k_dev) if kernel else (lr, re_code)


class BlurPreprocessing(_Preprocessing):
    """util.py:465-492 for a uint8 [N, H, W, C] device batch: to_tensor, then BatchBlur with one kernel per sample; the result is
    the UNquantised float32 [N, C, H, W] blurred batch at the input's size.  noise=True at the call is not carried over."""

    def __init__(self, scale, random, pca_matrix=None, kernel=21, noise=False, cuda=False, sig=2.6, sig_min=0.2, sig_max=4.0,
                 rate_iso=1.0, scaling=3, rate_cln=0.2, noise_high=0.08, seed=None, rank=0):
        super().__init__(scale, random, kernel, sig, sig_min, sig_max, rate_iso, scaling, rate_cln, noise_high, seed, rank)
        self.blur = BatchBlur(self.l)

    def __call__(self, hr_u8, noise=False, kernels=None):
        if noise:
            raise NotImplementedError('BlurPreprocessing: noise on the unquantised blurred floats is not carried over; '
                                      'SRMDPreprocessing(noise=True) adds it to the quantised LR')
        sdata._require_gpu_u8(hr_u8, 'BlurPreprocessing')
        n, h, w, _ = hr_u8.shape
        _check_pad(self.l, h, w)
        k_host, _ = self._tables(n, kernels, None, False)
        k_dev, _ = self._upload(hr_u8.device, k_host, None)
        out = self.blur(sdata.to_tensor(hr_u8), k_dev)
        self.last_kernels, self.last_levels, self.last_step = k_host, None, self.step
        self.step += 1
        return out


def degraded_training_batch(hr_u8, scale, degrade, augment=None):
    """data.training_batch with the LR made by `degrade` (an SRMDPreprocessing of the same scale) instead of plain bicubic:
    hr_u8 [N, H, W, 3] uint8 on the device, augmented first when `augment` (a data.Augment) is given.  Returns (lr, hr, bc):
    lr = degrade(hr_u8), hr = to_tensor(hr_u8), bc = the bicubic up-sampling of the LR bytes BEFORE the noise.  bc is only the
    baseline image of validation; no loss reads it."""
    if degrade.scale != scale:
        raise ValueError('degraded_training_batch: the degradation is built for scale %r, the batch asks for %r' % (degrade.scale, scale))
    if augment is not None:
        hr_u8 = augment(hr_u8)
    n, h, w, c = hr_u8.shape
    if h % scale or w % scale:
        raise ValueError('HR tile %dx%d is not a multiple of scale %d (calculate_valid_crop_size)' % (h, w, scale))
    lr = degrade(hr_u8)[0]
    bc_u8 = sdata.resize_u8(degrade.last_lr_u8, h, w, 'bicubic')
    return lr, sdata.to_tensor(hr_u8), sdata.to_tensor(bc_u8)
