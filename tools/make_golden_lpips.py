"""Generate tests/golden/lpips_alex.npz by running the REFERENCE utils/PerceptualSimilarity PerceptualLoss('net-lin', 'alex',
use_gpu=False) on the CPU (build container only).  torchvision is absent, so `torchvision.models.alexnet` is stubbed by an nn.Sequential
of the same thirteen feature layers filled with tests/lpips_ref.alexnet_state_dict() (the pretrained file is a download; the metric's
arithmetic does not depend on which weights it runs); skimage and tqdm are stubbed when absent.  The five lin heads are the reference's
own weights/v0.1/alex.pth (1 344 floats), which the reference loads itself.

Per case the reference is called as its validation loop calls it (sradsgan.py:1125-1132, 1326-1332): once per image,
`forward(sr[i:i+1], hr[i:i+1], normalize=True)`, and through the model's `retPerLayer` for the per-tap values (row 0 of that list is
the total, not tap 0: the reference adds the other layers into res[0] in place, networks_basic.py:85-87; rows 1-4 are taps).
Stored: the five head vectors, the small inputs, the outputs, and a checksum of the generated backbone weights.  The (2, 3, 216, 216) case stores outputs only
(its inputs are tests/lpips_ref.big_inputs())."""
import importlib
import importlib.machinery as mach
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle.make_golden import REF  # noqa: E402
from tests import lpips_ref as R  # noqa: E402


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    m.__path__ = []
    m.__spec__ = mach.ModuleSpec(name, None)
    sys.modules[name] = m
    return m


def alexnet_standin(pretrained=True):
    """torchvision.models.alexnet().features, layer for layer, with the generated weights."""
    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.features = nn.Sequential(
                nn.Conv2d(3, 64, 11, 4, 2), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2),
                nn.Conv2d(64, 192, 5, 1, 2), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2),
                nn.Conv2d(192, 384, 3, 1, 1), nn.ReLU(inplace=True), nn.Conv2d(384, 256, 3, 1, 1), nn.ReLU(inplace=True),
                nn.Conv2d(256, 256, 3, 1, 1), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2))
    net = Net()
    net.load_state_dict(R.alexnet_state_dict(), strict=True)
    return net


def import_perceptual():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    tv = _stub('torchvision')
    tv.models = _stub('torchvision.models', alexnet=alexnet_standin)
    for name in ('skimage', 'skimage.measure', 'skimage.transform', 'skimage.color', 'tqdm'):
        try:
            importlib.import_module(name)
        except Exception:
            _stub(name)
    sk = sys.modules['skimage']
    for sub in ('measure', 'transform', 'color'):
        if not hasattr(sk, sub):
            setattr(sk, sub, sys.modules['skimage.' + sub])
    if not hasattr(sys.modules['skimage.measure'], 'compare_ssim'):
        sys.modules['skimage.measure'].compare_ssim = None
    if not hasattr(sys.modules['tqdm'], 'tqdm'):
        sys.modules['tqdm'].tqdm = lambda it, *a, **k: it
    return importlib.import_module('utils.PerceptualSimilarity')


def small_inputs(idx, shape):
    hr = R.hash_image(shape, 11 + 2 * idx)
    sr = 0.75 * hr + 0.25 * R.hash_image(shape, 12 + 2 * idx)
    return sr, hr


def run(metric, sr, hr):
    total, layers = [], []
    with torch.no_grad():
        for i in range(sr.shape[0]):
            total.append(metric.forward(sr[i:i + 1], hr[i:i + 1], normalize=True).reshape(()).double())
            _, res = metric.model.forward(2 * hr[i:i + 1] - 1, 2 * sr[i:i + 1] - 1, retPerLayer=True)
            layers.append(torch.stack([r.reshape(()).double() for r in res]))
    return torch.stack(total).numpy(), torch.stack(layers, 1).numpy()              # [N], [5, N]


def main():
    torch.set_num_threads(8)
    ps = import_perceptual()
    metric = ps.PerceptualLoss(model='net-lin', net='alex', use_gpu=False)
    sd = R.alexnet_state_dict()
    net = metric.model.net
    out = {'backbone_checksum': R.weights_checksum(sd)}
    for k in range(5):
        out['lin%d' % k] = getattr(net, 'lin%d' % k).model[1].weight.detach().reshape(-1).numpy().astype(np.float32)
    cases = [('s%d' % i, small_inputs(i, shape), True) for i, shape in enumerate(R.SMALL_SHAPES)] + [('big', R.big_inputs(), False)]
    for name, (sr, hr), store in cases:
        if store:
            out[name + '_sr'], out[name + '_hr'] = sr.numpy(), hr.numpy()
        out[name + '_lpips'], out[name + '_taps'] = run(metric, sr, hr)
        print(name, tuple(sr.shape), out[name + '_lpips'])
    np.savez_compressed(R.GOLDEN, **out)
    print('%s: %.1f KB' % (R.GOLDEN, os.path.getsize(R.GOLDEN) / 1024.0))


if __name__ == '__main__':
    main()
