"""numpy restatement of the degradation kernels (csrc/degrade.hip) and of the kernel formulas (sradsgan_amd/degrade.py), written
from the contract in include/sradsgan_hip.h and from the mathematics, independent of both: float32 accumulators in the stated
order (rows outer, columns inner; product and sum rounded separately), explicit reflection indices, truncating quantisation."""
import numpy as np

F = np.float32


def pads(l):
    """(lo, hi): rows / columns put before and after the image."""
    return l // 2, (l // 2 if l % 2 else l // 2 - 1)


def reflect_index(i, size):
    """nn.ReflectionPad2d's source index (the edge is not repeated)."""
    if i < 0:
        i = -i
    if i >= size:
        i = 2 * (size - 1) - i
    assert 0 <= i < size
    return i


def reflect_pad(x, l):
    """x: [..., H, W] -> [..., H + l - 1, W + l - 1], by explicit indices."""
    lo, hi = pads(l)
    h, w = x.shape[-2:]
    assert lo < h and lo < w
    rows = [reflect_index(i, h) for i in range(-lo, h + hi)]
    cols = [reflect_index(j, w) for j in range(-lo, w + hi)]
    return x[..., rows, :][..., cols]


def blur_f32(x, kernels):
    """x: float32 [N, C, H, W]; kernels: float32 [N, l, l] or [l, l].  acc = 0; acc = acc + k[i][j] * xpad[y + i][x + j], every
    product and every sum a float32."""
    x = np.asarray(x, F)
    k = np.asarray(kernels, F)
    n, c, h, w = x.shape
    if k.ndim == 2:
        k = np.broadcast_to(k, (n,) + k.shape)
    l = k.shape[-1]
    xp = reflect_pad(x, l)
    acc = np.zeros((n, c, h, w), F)
    with np.errstate(invalid='ignore'):
        for i in range(l):
            for j in range(l):
                prod = (k[:, i, j].reshape(n, 1, 1, 1) * xp[:, :, i:i + h, j:j + w]).astype(F)
                acc = (acc + prod).astype(F)
    assert acc.dtype == F
    return acc


def blur_abs_sum(x, kernels):
    """S = sum |k[i][j] * xpad| per output in float64: the scale of the rounding-error bound of an fp32 sum of l * l terms."""
    x = np.asarray(x, np.float64)
    k = np.asarray(kernels, np.float64)
    n, c, h, w = x.shape
    if k.ndim == 2:
        k = np.broadcast_to(k, (n,) + k.shape)
    l = k.shape[-1]
    xp = reflect_pad(x, l)
    s = np.zeros((n, c, h, w), np.float64)
    for i in range(l):
        for j in range(l):
            s += np.abs(k[:, i, j].reshape(n, 1, 1, 1) * xp[:, :, i:i + h, j:j + w])
    return s


def blur_bound(x, kernels):
    """2 (l^2 + 1) 2^-24 S: two fp32 sums of the same l^2 non-negative-weight terms, in any two orders, differ by at most this
    (each is within gamma_{l^2} S of the exact sum, the products' own roundings included in the + 1)."""
    l = np.asarray(kernels).shape[-1]
    return 2.0 * (l * l + 1) * 2.0 ** -24 * blur_abs_sum(x, kernels)


def to_float(u8):
    """uint8 -> float32 value / 255 (to_tensor, srhip_u8_to_float), same layout."""
    return (np.asarray(u8).astype(F) / F(255.0)).astype(F)


def quantise(x):
    """to_pil_image's mul(255).byte(): a float32 product, truncated."""
    return (np.asarray(x, F) * F(255.0)).astype(F).astype(np.int32).astype(np.uint8)


def blur_u8(img, kernels):
    """img: uint8 [N, H, W, C]; kernels [N, l, l] -> uint8 [N, H, W, C]."""
    x = to_float(img).transpose(0, 3, 1, 2)
    return np.ascontiguousarray(quantise(blur_f32(x, kernels)).transpose(0, 2, 3, 1))


def pil_resize(img, out_h, out_w):
    """Pillow's bicubic per image, uint8 [N, H, W, C] (C = 1 as mode L)."""
    from PIL import Image
    out = []
    for a in img:
        pil = Image.fromarray(a[..., 0] if a.shape[-1] == 1 else a)
        r = np.asarray(pil.resize((out_w, out_h), Image.BICUBIC))
        out.append(r[..., None] if a.shape[-1] == 1 else r)
    return np.stack(out)


def noise_tail(lr_u8, levels, z):
    """clamp(byte / 255 + z * level[n], 0, 1) in float32, product and sum rounded separately; layout of lr_u8 and z alike."""
    x = to_float(lr_u8)
    lv = np.asarray(levels, F).reshape((-1,) + (1,) * (x.ndim - 1))
    q = (x + (np.asarray(z, F) * lv).astype(F)).astype(F)
    return np.minimum(np.maximum(q, F(0.0)), F(1.0)).astype(F)


# ---- kernel formulas, float64 ---------------------------------------------------------------- #

def taps(l):
    """Tap coordinates: -(l // 2) .. l // 2 for odd l; -(l / 2 - 1) .. l / 2 for even l."""
    return np.array([t - (l // 2 if l % 2 else l // 2 - 1) for t in range(l)], np.float64)


def gaussian_kernel(l, sig_x, sig_y, theta):
    """exp(-v^T S^-1 v / 2) / sum, v = (column, row) tap coordinates, S = R(theta) diag(sig_x^2, sig_y^2) R(theta)^T, float64."""
    t = taps(l)
    c, s = np.cos(theta), np.sin(theta)
    rot = np.array([[c, -s], [s, c]])
    inv = np.linalg.inv(rot @ np.diag([sig_x ** 2, sig_y ** 2]) @ rot.T)
    k = np.empty((l, l), np.float64)
    for i in range(l):            # row
        for j in range(l):        # column
            v = np.array([t[j], t[i]])
            k[i, j] = np.exp(-0.5 * (v @ inv @ v))
    return k / k.sum()


def isotropic_kernel(l, sig):
    t = taps(l)
    k = np.exp(-(t[None, :] ** 2 + t[:, None] ** 2) / (2.0 * sig ** 2))
    return k / k.sum()


def ulp_distance(a, b):
    """Distance in float32 units in the last place (same-sign finite values)."""
    a = np.asarray(a, F).view(np.int32).astype(np.int64)
    b = np.asarray(b, F).view(np.int32).astype(np.int64)
    return np.abs(a - b)
