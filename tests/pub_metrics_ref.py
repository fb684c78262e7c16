"""numpy / scipy fp64 restatement of the papers' evaluation protocol (sradsgan_amd/metrics.py, include/sradsgan_hip.h): calculate_psnr /
calculate_ssim of the reference's GDP_x0/core/metrics.py:109-160 with BasicSR's crop_border and test_y_channel switches.  Restated from
reading those lines: cv2, skimage and BasicSR are not dependencies, so agreement with them is not pinned here.

The SSIM of `metrics` is the FULL 121-tap two-dimensional correlation (scipy.ndimage.correlate, cropped [5:-5, 5:-5] as the reference
crops cv2.filter2D) -- deliberately not the separable form the kernel uses; `ssim_separable` is that form, for the CPU test that
compares the two."""
import numpy as np
from scipy import ndimage

C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2


def gaussian():
    """cv2.getGaussianKernel(11, 1.5): g_i = exp(-(i - 5)^2 / (2 sigma^2)) / sum, fp64."""
    g = np.exp(-((np.arange(11, dtype=np.float64) - 5.0) ** 2) / 4.5)
    return g / g.sum()


def quantise(x):
    """tensor2img(min_max=(0, 1)): float32 clamp, float32 product with 255, round half to even; NaN -> 0 (a byte cannot carry it)."""
    x = np.asarray(x, np.float32)
    v = np.clip(np.where(np.isnan(x), np.float32(0), x), np.float32(0), np.float32(1))
    return np.rint(v * np.float32(255)).astype(np.uint8)


def luma(img_u8):
    """[..., 3] uint8 RGB -> fp64 Y of BT.601 studio range, from the exact integer numerator, never rounded."""
    v = img_u8.astype(np.int64)
    return 16.0 + (65481 * v[..., 0] + 128553 * v[..., 1] + 24966 * v[..., 2]).astype(np.float64) / 255000.0


def luma_basicsr(img_u8):
    """Y as BasicSR's calculate_* write it (to_y_channel + bgr2ycbcr(y_only=True)): float32 image / 255, fp64 dot with the BT.601 row,
    + 16, / 255 rounded to float32, x 255.  Used only to measure how far this package's fp64 Y departs from it."""
    img = img_u8.astype(np.float32) / np.float32(255.0)
    bgr = img[..., ::-1]
    y = np.dot(bgr, [24.966, 128.553, 65.481]) + 16.0
    y = (y / 255.0).astype(np.float32)
    return y.astype(np.float64) * 255.0


def planes(img_u8, crop, y, luma_fn=luma):
    """uint8 [H, W, C] -> fp64 [H', W', C or 1]: the cropped channels the metrics see."""
    h, w = img_u8.shape[:2]
    img = img_u8[crop:h - crop, crop:w - crop]
    return luma_fn(img)[..., None] if y else img.astype(np.float64)


def psnr_from_mse(mse):
    return float('inf') if mse == 0 else 10.0 * np.log10(255.0 * 255.0 / mse)


def _ssim_formula(mu1, mu2, e11, e22, e12):
    s1, s2, s12 = e11 - mu1 * mu1, e22 - mu2 * mu2, e12 - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def ssim_full(a, b):
    """a, b: fp64 [H, W, C].  Mean SSIM over valid positions and channels with the full 11 x 11 window."""
    g = gaussian()
    window = np.outer(g, g)
    vals = []
    for ch in range(a.shape[2]):
        x, y = a[..., ch], b[..., ch]
        f = lambda p: ndimage.correlate(p, window, mode='reflect')[5:-5, 5:-5]
        vals.append(_ssim_formula(f(x), f(y), f(x * x), f(y * y), f(x * y)))
    return float(np.mean(np.stack(vals)))


def ssim_separable(a, b):
    """The same with 11 horizontal taps, then 11 vertical taps (the kernel's form)."""
    g = gaussian()
    vals = []
    for ch in range(a.shape[2]):
        x, y = a[..., ch], b[..., ch]

        def f(p):
            hp = sum(g[k] * p[:, k:p.shape[1] - 10 + k] for k in range(11))
            return sum(g[k] * hp[k:hp.shape[0] - 10 + k] for k in range(11))
        vals.append(_ssim_formula(f(x), f(y), f(x * x), f(y * y), f(x * y)))
    return float(np.mean(np.stack(vals)))


def metrics(a_u8, b_u8, crop=0, y=False, luma_fn=luma, ssim_fn=ssim_full):
    """uint8 [H, W, C] test and ground-truth images -> dict(mse, psnr, ssim) in fp64.  In RGB mode mse is the int64 sum of squared byte
    differences divided once."""
    pa, pb = planes(a_u8, crop, y, luma_fn), planes(b_u8, crop, y, luma_fn)
    if y:
        mse = float(np.mean((pa - pb) ** 2))
    else:
        h, w = a_u8.shape[:2]
        d = a_u8[crop:h - crop, crop:w - crop].astype(np.int64) - b_u8[crop:h - crop, crop:w - crop].astype(np.int64)
        mse = float(np.sum(d * d)) / float(d.size)
    return dict(mse=mse, psnr=psnr_from_mse(mse), ssim=ssim_fn(pa, pb))


# ---- test images: uint8 [H, W, C] pairs (test, ground truth) ----------------------------------------------------------------------- #
CONTENTS = ('random', 'near_copy', 'equal_constants', 'constant_vs_random', 'step')


def pair(kind, h, w, c, seed):
    rng = np.random.RandomState(seed)
    if kind == 'random':
        return rng.randint(0, 256, (h, w, c)).astype(np.uint8), rng.randint(0, 256, (h, w, c)).astype(np.uint8)
    if kind == 'near_copy':
        b = rng.randint(0, 256, (h, w, c))
        d = rng.randint(-3, 4, (h, w, c)) * (rng.rand(h, w, c) < 1.0 / 3.0)
        return np.clip(b + d, 0, 255).astype(np.uint8), b.astype(np.uint8)
    if kind == 'equal_constants':
        v = np.full((h, w, c), 0, np.uint8) + np.array([37, 201, 118][:c], np.uint8)
        return v, v.copy()
    if kind == 'constant_vs_random':
        return np.full((h, w, c), 128, np.uint8), rng.randint(0, 256, (h, w, c)).astype(np.uint8)
    if kind == 'step':
        a = np.zeros((h, w, c), np.uint8)
        a[:, w // 2:] = 255
        b = np.zeros((h, w, c), np.uint8)
        b[:, w // 2 + 1:] = 250
        return a, b
    raise ValueError(kind)
