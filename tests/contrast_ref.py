"""A from-scratch restatement of the reference's contrastive VGG19 losses (model/loss.py:121-298) with stock torch ops, in any dtype and
differentiable by autograd, and a deterministic VGG19 weight generator that needs no RNG state and no file (the 12.9 M backbone weights
up to relu5_1 are never committed).

    taps: relu1_1, relu2_1, relu3_1, relu4_1, relu5_1 of torchvision's vgg19.features on the UNNORMALISED image
    L1 forms:      sum_t w_t * mean|a - p| / (sum_j mean|a - n_j| + 1e-7)                      (ablation: w_t * mean|a - p|)
    cosine forms:  E_x = exp(mean_hw cos(a, x) / 0.07) per sample;
                   single: mean_b sum_t w_t * -log(E_p / (E_n + 1e-7))                         (ablation: -log(E_p))
                   N:      mean_b sum_t w_t * -log(E_p / (sum_j E_nj + E_p))
    w = 1/32, 1/16, 1/8, 1/4, 1

`cos` restates F.cosine_similarity(dim=1) as the installed torch computes it: each vector is divided by its own norm clamped at 1e-8,
then the products are summed.  A zero-norm vector therefore gives cosine 0 and a finite gradient.

Weights: tests/lpips_ref.hash16 (an integer hash of the element index onto a 16-bit grid), scaled by 2 * sqrt(6 / fan_in) (He-uniform,
so every tap stays alive through the ReLUs); biases in +-0.1."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests.lpips_ref import hash16, hash_image, weights_checksum  # noqa: F401

# features index -> (cin, cout); ReLU after each conv, MaxPool2d(2) at 4, 9, 18, 27
CONVS = {0: (3, 64), 2: (64, 64), 5: (64, 128), 7: (128, 128), 10: (128, 256), 12: (256, 256), 14: (256, 256), 16: (256, 256),
         19: (256, 512), 21: (512, 512), 23: (512, 512), 25: (512, 512), 28: (512, 512)}
POOLS = (4, 9, 18, 27)
TAPS = (0, 5, 10, 19, 28)
CHANNELS = (64, 128, 256, 512, 512)
WEIGHTS = (1.0 / 32, 1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0)
T = 0.07
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'contrast.npz')
SHAPES = ((2, 3, 32, 32), (2, 3, 40, 44), (1, 3, 16, 16))      # all pools even; odd at the third and fourth pool; tap 5 is 1 x 1
MAX_N = 3
KINDS = ('ContrastLoss', 'NContrastLoss', 'ContrastCosineLoss', 'NContrastCosineLoss')
MARGIN = 64.0                                                  # smallest non-zero |a - x| over the largest fp32 feature error, per tap

_SD = {}


def vgg19_state_dict():
    """torchvision-style keys features.N.{weight,bias} of the 13 convs up to relu5_1, float32.  Cached: treat as read-only."""
    if not _SD:
        for i, (cin, cout) in CONVS.items():
            n = cout * cin * 9
            _SD['features.%d.weight' % i] = (hash16(n, 2 * i + 1) * 2.0 * (6.0 / (cin * 9)) ** 0.5).float().reshape(cout, cin, 3, 3)
            _SD['features.%d.bias' % i] = (hash16(cout, 2 * i + 2) * 0.2).float()
    return _SD


def reference_keys():
    """The state-dict keys and shapes of the reference's Vgg19 module (loss.py:121-139): slice names with torchvision's indices."""
    out = {}
    for i, (cin, cout) in CONVS.items():
        s = 1 + sum(i >= lo for lo in (2, 7, 12, 21))
        out['slice%d.%d.weight' % (s, i)] = (cout, cin, 3, 3)
        out['slice%d.%d.bias' % (s, i)] = (cout,)
    return out


def inputs(shape, salt):
    """(a, p, n): a, p [B,3,H,W], n [B,MAX_N,3,H,W], float32.  p is a hash image, a = 0.75 p + 0.25 noise (the super-resolved image),
    n_j = 0.5 p + 0.5 noise_j (the degraded images)."""
    b = shape[0]
    p = hash_image(shape, 1000 * salt + 1)
    a = 0.75 * p + 0.25 * hash_image(shape, 1000 * salt + 2)
    n = torch.stack([0.5 * p + 0.5 * hash_image(shape, 1000 * salt + 3 + j) for j in range(MAX_N)], 1)
    assert n.shape[0] == b
    return a, p, n


def taps(x, sd=None, conv=None):
    """The five ReLU taps of [M,3,H,W] images in x's dtype.  conv(x, w, b, stride, pad), when given, replaces F.conv2d."""
    sd = vgg19_state_dict() if sd is None else sd
    cast = lambda k: sd[k].to(dtype=x.dtype, device=x.device)
    f, out = x, []
    for i in range(30):
        if i in CONVS:
            w, b = cast('features.%d.weight' % i), cast('features.%d.bias' % i)
            f = F.relu(F.conv2d(f, w, b, 1, 1) if conv is None else conv(f, w, b, 1, 1))
            if i in TAPS:
                out.append(f)
        elif i in POOLS:
            f = F.max_pool2d(f, 2)
    return out


def cos(a, x, eps=1e-8):
    """F.cosine_similarity(a, x, dim=1) of the installed torch, restated: [B,C,h,w] x 2 -> [B,h,w]."""
    na = torch.linalg.vector_norm(a, 2, 1, keepdim=True).clamp_min(eps)
    nx = torch.linalg.vector_norm(x, 2, 1, keepdim=True).clamp_min(eps)
    return ((a / na) * (x / nx)).sum(1)


def l1_from_taps(fa, fp, fn, ablation=False):
    """fa, fp: the taps of a and p; fn: per negative, its taps."""
    total = 0
    for t, w in enumerate(WEIGHTS):
        dap = (fa[t] - fp[t]).abs().mean()
        if ablation:
            total = total + w * dap
        else:
            dan = sum((fa[t] - f[t]).abs().mean() for f in fn)
            total = total + w * (dap / (dan + 1e-7))
    return total


def cos_from_taps(fa, fp, fn, n_form, ablation=False):
    total = 0
    for t, w in enumerate(WEIGHTS):
        ep = (cos(fa[t], fp[t]).mean((1, 2)) / T).exp()
        en = [(cos(fa[t], f[t]).mean((1, 2)) / T).exp() for f in fn]
        if n_form:
            term = -torch.log(ep / (sum(en) + ep))
        elif ablation:
            term = -torch.log(ep)
        else:
            term = -torch.log(ep / (en[0] + 1e-7))
        total = total + w * term
    return total.mean()


def loss(kind, a, p, n, ablation=False, dtype=torch.float64, conv=None, sd=None):
    """kind: one of KINDS; n: [B,3,H,W] for the single-negative kinds, [B,N,3,H,W] for the N kinds -> a 0-d tensor of `dtype`,
    differentiable in a.  As in the reference, the N kinds ignore `ablation`."""
    many = kind.startswith('N')
    negs = [n[:, j] for j in range(n.shape[1])] if many else [n]
    fa, fp = taps(a.to(dtype), sd, conv), taps(p.to(dtype), sd, conv)
    fn = [taps(x.to(dtype), sd, conv) for x in negs]
    if 'Cosine' in kind:
        return cos_from_taps(fa, fp, fn, many, ablation and not many)
    return l1_from_taps(fa, fp, fn, ablation and not many)


def loss_and_grad(kind, a, p, n, ablation=False, dtype=torch.float64, conv=None, sd=None):
    """(loss, d loss / d a) by autograd in `dtype`."""
    x = a.detach().to(dtype).requires_grad_(True)
    val = loss(kind, x, p, n, ablation, dtype, conv, sd)
    g, = torch.autograd.grad(val, x)
    return val.detach(), g


def emulated_conv(arith):
    """conv(x, w, b, stride, pad) whose forward and data gradient run tests/conv_emulation's contraction in `arith`."""
    from tests.lpips_loss_ref import emulated_conv as make
    return make(arith)


def margins(a, p, n):
    """Per tap: (the smallest non-zero |a - x| over x in {p, n_1 ..} in float64, the largest |fp32 feature - fp64 feature| over all
    images, the number of elements whose sign(a - x) differs between the fp32 and the fp64 run).  n: [B,N,3,H,W]."""
    imgs = [a, p] + [n[:, j] for j in range(n.shape[1])]
    with torch.no_grad():
        f64 = [taps(x.double()) for x in imgs]
        f32 = [taps(x.float()) for x in imgs]
    out = []
    for t in range(5):
        err = max(float((f32[k][t].double() - f64[k][t]).abs().max()) for k in range(len(imgs)))
        small, flips = float('inf'), 0
        for k in range(1, len(imgs)):
            d64, d32 = f64[0][t] - f64[k][t], f32[0][t] - f32[k][t]
            nz = d64.abs()[d64 != 0]
            small = min(small, float(nz.min())) if nz.numel() else small
            flips += int((torch.sign(d64) != torch.sign(d32.double())).sum())
        out.append((small, err, flips))
    return out


def margins_hold(m):
    return all(small >= MARGIN * err and flips == 0 for small, err, flips in m)
