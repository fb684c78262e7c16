"""PSNR and SSIM by the protocol the SR papers report (EDSR, RCAN, ESRGAN, SwinIR, HAT and every BasicSR-based project), on the
device: csrc/metrics_pub.hip, arithmetic stated in include/sradsgan_hip.h.

  * the image quantised by tensor2img: clamp to [0, 1], x 255, round half to even (float front end only);
  * `crop_border` pixels shaved from every border;
  * optionally the BT.601 studio-range luma Y = 16 + (65.481 r + 128.553 g + 24.966 b) / 255 instead of the RGB channels, kept in
    fp64 (BasicSR rounds it through a float32 intermediate; the difference is recorded in DESIGN.md);
  * SSIM with an 11 x 11 Gaussian window of sigma 1.5 over the valid region, population covariance.

At their defaults `calculate_psnr` / `calculate_ssim` are the two functions of the reference's GDP_x0/core/metrics.py:109-160 (restated
from reading them: neither cv2 nor BasicSR is a dependency, and agreement with them is not pinned by a test).  `validate.quantized_metrics`
stays the reference trainer's own protocol (truncating quantiser with wrap, RGB, no crop, uniform 7 x 7 window, sample covariance).

Nothing here synchronises with the host, so every function may run under stream capture."""
import ctypes
import numbers

import torch

from . import _hip

WINDOW = 11          # side of the Gaussian window; a cropped side below it has no valid SSIM position


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check_protocol(what, h, w, c, crop_border, y_channel):
    if isinstance(crop_border, bool) or not isinstance(crop_border, numbers.Integral) or crop_border < 0:
        raise ValueError('%s: crop_border must be a non-negative integer, got %r' % (what, crop_border))
    if c not in (1, 3):
        raise ValueError('%s: images must have 1 or 3 channels, got %d' % (what, c))
    if y_channel and c != 3:
        raise ValueError('%s: y_channel needs 3 channels (RGB), got %d' % (what, c))
    if h - 2 * crop_border < WINDOW or w - 2 * crop_border < WINDOW:
        raise ValueError('%s: a %d x %d image cropped by %d leaves less than the %d x %d SSIM window'
                         % (what, h, w, crop_border, WINDOW, WINDOW))
    return int(crop_border)


def _require_device(what, *tensors):
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError('%s: sradsgan_amd metrics run on the MI355X HIP path only (got a %s tensor); there is no CPU fallback'
                               % (what, t.device))


def library_config():
    """(partials per image, SSIM tile side in valid positions) of the loaded library."""
    partials, tile = ctypes.c_int(0), ctypes.c_int(0)
    _hip.check(_hip.lib().srhip_pub_config(ctypes.byref(partials), ctypes.byref(tile)), 'pub_config')
    return partials.value, tile.value


def _launch(a, b, n, h, w, c, crop, luma, is_float):
    """a, b: dense NHWC memory on the device.  Three launches; returns float64 [3][n] = mse | psnr | ssim."""
    lib = _hip.lib()
    nb = library_config()[0]
    st = _stream()
    part = torch.empty(n, nb, 2, device=a.device, dtype=torch.int64)
    _hip.check(lib.srhip_pub_sse(_p(a), _p(b), _p(part), n, h, w, c, crop, luma, is_float, st), 'pub_sse')
    spart = torch.empty(n, nb, device=a.device, dtype=torch.float64)
    _hip.check(lib.srhip_pub_ssim(_p(a), _p(b), _p(spart), n, h, w, c, crop, luma, is_float, st), 'pub_ssim')
    out = torch.empty(3, n, device=a.device, dtype=torch.float64)
    _hip.check(lib.srhip_pub_finish(_p(part), _p(spart), _p(out), n, h, w, c, crop, luma, st), 'pub_finish')
    return out


def published_metrics_u8(a_u8, b_u8, crop_border=0, y_channel=False):
    """a_u8 (test), b_u8 (ground truth): uint8 [N, H, W, C] or [H, W, C] on the HIP device, C in {1, 3}.  Returns a dict of float64
    tensors [N]: mse, psnr (+inf where the images are equal), ssim -- per image, by the protocol of the module docstring."""
    what = 'published_metrics_u8'
    for t in (a_u8, b_u8):
        if not torch.is_tensor(t) or t.dtype != torch.uint8:
            raise ValueError('%s: images must be uint8 tensors, got %s' % (what, t.dtype if torch.is_tensor(t) else type(t).__name__))
        if t.dim() not in (3, 4):
            raise ValueError('%s: images must be [N, H, W, C] or [H, W, C], got %s' % (what, tuple(t.shape)))
    if a_u8.shape != b_u8.shape:
        raise ValueError('%s: shape mismatch %s vs %s' % (what, tuple(a_u8.shape), tuple(b_u8.shape)))
    if a_u8.dim() == 3:
        a_u8, b_u8 = a_u8[None], b_u8[None]
    n, h, w, c = a_u8.shape
    if n == 0:
        raise ValueError('%s: empty batch' % what)
    crop = _check_protocol(what, h, w, c, crop_border, y_channel)
    _require_device(what, a_u8, b_u8)
    out = _launch(a_u8.contiguous(), b_u8.contiguous(), n, h, w, c, crop, int(bool(y_channel)), 0)
    return dict(mse=out[0], psnr=out[1], ssim=out[2])


def _check_float(what, a, b):
    for t in (a, b):
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise ValueError('%s: images must be float32 tensors, got %s' % (what, t.dtype if torch.is_tensor(t) else type(t).__name__))
        if t.dim() != 4:
            raise ValueError('%s: images must be [N, C, H, W], got %s' % (what, tuple(t.shape)))
    if b is not a and a.shape != b.shape:
        raise ValueError('%s: shape mismatch %s vs %s' % (what, tuple(a.shape), tuple(b.shape)))
    if a.shape[0] == 0:
        raise ValueError('%s: empty batch' % what)


def published_metrics(a, b, crop_border=0, y_channel=False):
    """a (test), b (ground truth): float32 [N, C, H, W] in nominal [0, 1] on the HIP device, any memory format; quantised inside the
    kernels (NaN -> byte 0).  Returns what published_metrics_u8(quantise(a), quantise(b), ...) returns, bit for bit."""
    what = 'published_metrics'
    _check_float(what, a, b)
    n, c, h, w = a.shape
    crop = _check_protocol(what, h, w, c, crop_border, y_channel)
    _require_device(what, a, b)
    a = a.detach().contiguous(memory_format=torch.channels_last)
    b = b.detach().contiguous(memory_format=torch.channels_last)
    out = _launch(a, b, n, h, w, c, crop, int(bool(y_channel)), 1)
    return dict(mse=out[0], psnr=out[1], ssim=out[2])


def quantise(x):
    """tensor2img(min_max=(0, 1)) of x, float32 [N, C, H, W] on the HIP device (any memory format): uint8 [N, H, W, C] =
    rint(clamp(x, 0, 1) * 255) with the float32 product rounded half to even; a NaN becomes byte 0."""
    what = 'quantise'
    _check_float(what, x, x)
    _require_device(what, x)
    n, c, h, w = x.shape
    x = x.detach().contiguous(memory_format=torch.channels_last)
    out = torch.empty(n, h, w, c, device=x.device, dtype=torch.uint8)
    _hip.check(_hip.lib().srhip_diff_quant_u8(_p(x), c, _p(out), n * h * w, c, 0.0, 1.0, _stream()), 'diff_quant_u8')
    return out


def _single(what, img, img2):
    for t in (img, img2):
        if not torch.is_tensor(t) or t.dtype != torch.uint8:
            raise ValueError('%s: images must be uint8 tensors, got %s' % (what, t.dtype if torch.is_tensor(t) else type(t).__name__))
        if t.dim() == 2:
            raise ValueError('%s: a grey image is [H, W, 1] here, got %s' % (what, tuple(t.shape)))
        if t.dim() != 3:
            raise ValueError('%s: images must be [H, W, C], got %s' % (what, tuple(t.shape)))


def calculate_psnr(img, img2, crop_border=0, test_y_channel=False):
    """BasicSR's (and, at the defaults, the reference's) calculate_psnr for uint8 [H, W, C] device tensors: a float64 device scalar."""
    _single('calculate_psnr', img, img2)
    return published_metrics_u8(img, img2, crop_border, test_y_channel)['psnr'][0]


def calculate_ssim(img, img2, crop_border=0, test_y_channel=False):
    """BasicSR's (and, at the defaults, the reference's) calculate_ssim for uint8 [H, W, C] device tensors: a float64 device scalar."""
    _single('calculate_ssim', img, img2)
    return published_metrics_u8(img, img2, crop_border, test_y_channel)['ssim'][0]
