"""A from-scratch restatement of LPIPS (net-lin, AlexNet, v0.1) with stock torch ops, in any dtype, and a deterministic AlexNet weight
generator that needs no RNG state and no file (the 2.47 M backbone weights are never committed).

    x = 2x - 1;  x = (x - shift) / scale                       per channel
    AlexNet features[0:12], the five ReLU outputs are the taps  (conv padding is zero in the scaled space)
    per tap and pixel: f / (sqrt(sum_c f^2) + 1e-10) for both images, sum_c w_c (f0_c - f1_c)^2, mean over pixels
    sum of the five taps

Weights: an integer hash of the element index onto a 16-bit grid (exact in fp32), scaled by 2 * sqrt(6 / fan_in) (He-uniform, so every
tap stays alive through the ReLUs); biases in +-0.1.  Images for the large case come from the same hash."""
import os

import numpy as np
import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
# features index -> (cin, cout, k, stride, pad)
CONVS = {0: (3, 64, 11, 4, 2), 3: (64, 192, 5, 1, 2), 6: (192, 384, 3, 1, 1), 8: (384, 256, 3, 1, 1), 10: (256, 256, 3, 1, 1)}
CHANNELS = (64, 192, 384, 256, 256)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'lpips_alex.npz')
SMALL_SHAPES = ((2, 3, 35, 47), (1, 3, 31, 31), (2, 3, 64, 50))
BIG_SHAPE = (2, 3, 216, 216)


def hash16(n, salt):
    """n values in (-0.5, 0.5) on a 16-bit grid: (u + 0.5) / 65536 - 0.5 with u the low 16 bits of a 32-bit integer hash of index + salt."""
    m = 0xFFFFFFFF
    x = (torch.arange(n, dtype=torch.int64) + 1 + salt * 0x9E3779B1) & m
    for _ in range(2):
        x = (((x >> 16) ^ x) * 0x45D9F3B) & m
    x = ((x >> 16) ^ x) & 0xFFFF
    return (x.double() + 0.5) / 65536.0 - 0.5


def alexnet_state_dict():
    """torchvision-style keys features.{0,3,6,8,10}.{weight,bias}, float32."""
    sd = {}
    for i, (cin, cout, k, _, _) in CONVS.items():
        n = cout * cin * k * k
        sd['features.%d.weight' % i] = (hash16(n, 2 * i + 1) * 2.0 * (6.0 / (cin * k * k)) ** 0.5).float().reshape(cout, cin, k, k)
        sd['features.%d.bias' % i] = (hash16(cout, 2 * i + 2) * 0.2).float()
    return sd


def weights_checksum(sd):
    """A float64 digest of the generated backbone: per tensor (sum, sum of squares, index-weighted sum)."""
    out = []
    for k in sorted(sd):
        v = sd[k].double().flatten()
        out += [float(v.sum()), float((v * v).sum()), float((v * torch.arange(v.numel(), dtype=torch.float64)).sum())]
    return np.array(out, dtype=np.float64)


def hash_image(shape, salt):
    """[0, 1) image on the 16-bit grid, float32."""
    n = int(np.prod(shape))
    return (hash16(n, salt) + 0.5).float().reshape(shape)


def big_inputs():
    """(sr, hr) of the (2, 3, 216, 216) case: hr from the hash, sr a blend of hr with a second hash image."""
    hr = hash_image(BIG_SHAPE, 101)
    sr = 0.75 * hr + 0.25 * hash_image(BIG_SHAPE, 102)
    return sr, hr


def lin_state_dict(golden):
    return {'lin%d.model.1.weight' % k: torch.from_numpy(golden['lin%d' % k]).reshape(1, -1, 1, 1) for k in range(5)}


def scaled(x, normalize=True):
    if normalize:
        x = 2 * x - 1
    shift = torch.tensor(SHIFT, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    return (x - shift) / scale


def _conv(x, w, b, stride, pad, conv=None):
    if conv is not None:
        return conv(x, w, b, stride, pad)
    return F.conv2d(x, w, b, stride, pad)


def taps(x, sd, normalize=True, conv=None):
    """The five ReLU taps of [N,3,H,W] images in x's dtype.  conv(x, w, b, stride, pad), when given, replaces F.conv2d for convs 2-5."""
    cast = lambda k: sd[k].to(dtype=x.dtype, device=x.device)
    f = F.relu(F.conv2d(scaled(x, normalize), cast('features.0.weight'), cast('features.0.bias'), 4, 2))
    out = [f]
    for i in (3, 6, 8, 10):
        if i in (3, 6):
            f = F.max_pool2d(f, 3, 2)
        f = F.relu(_conv(f, cast('features.%d.weight' % i), cast('features.%d.bias' % i), CONVS[i][3], CONVS[i][4], conv))
        out.append(f)
    return out


def head(f0, f1, w):
    """One tap: [N,C,h,w] features of the two images, w [C] -> [N] (mean over pixels)."""
    n0 = f0 / (torch.sqrt((f0 * f0).sum(1, keepdim=True)) + 1e-10)
    n1 = f1 / (torch.sqrt((f1 * f1).sum(1, keepdim=True)) + 1e-10)
    d = (n0 - n1) ** 2
    return (d * w.to(d.dtype).view(1, -1, 1, 1)).sum(1).mean((1, 2))


def lpips(pred, target, sd, lin, dtype=torch.float64, normalize=True, conv=None, per_tap=False):
    """[N] distances (and, with per_tap, the [5, N] tap values).  lin: the five [C] weight vectors."""
    t0 = taps(target.to(dtype), sd, normalize, conv)
    t1 = taps(pred.to(dtype), sd, normalize, conv)
    vals = torch.stack([head(a, b, torch.as_tensor(w).flatten()) for a, b, w in zip(t0, t1, lin)])
    return (vals.sum(0), vals) if per_tap else vals.sum(0)
