"""Generate tests/golden/augment.npz: the training augmentation of the reference's Dataset.__getitem__ (data/dataset.py:273-324)
with explicit draws instead of its random ones.  torchvision is not needed: the steps are restated with the Pillow calls
torchvision's transforms make --

    CenterCrop / RandomCrop         img.crop((x0, y0, x0 + cs, y0 + cs))
    noise, ToPILImage               Image.fromarray((asarray(img) + sigma * z).clip(0, 255).astype(uint8))       (float64)
    img.rotate(90 * rv, expand=True)
    RandomHorizontalFlip            img.transpose(FLIP_LEFT_RIGHT)
    img.transpose(FLIP_TOP_BOTTOM)
    Resize(.., BICUBIC)             img.resize((w, h), BICUBIC): HR (the identity at the crop size), LR, and BC from LR

Recorded: three asymmetric 17 x 15 x 3 sources (random bytes: no symmetry, so every op and offset gives different bytes), every
(rv, fliplr, fliptb) in {0 (rotate=False), 1, 2, 3} x {0, 1} x {0, 1}, crops of 12 at the four corners and two interior offsets,
one case with Gaussian noise from a recorded fp32 z; per case the HR bytes and the LR / BC bytes at scales 2 and 3.

    python tools/make_golden_augment.py"""
import os

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, CS = 17, 15, 12
SIGMA = 12.5


def reference_item(src, y0, x0, rv, fliplr, fliptb, sigma=0.0, z=None):
    img = Image.fromarray(src).crop((x0, y0, x0 + CS, y0 + CS))
    if sigma:
        noisy = np.asarray(img) + sigma * z.astype(np.float64)
        img = Image.fromarray(noisy.clip(0, 255).astype(np.uint8))
    if rv:
        img = img.rotate(90 * rv, expand=True)
    if fliplr:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    if fliptb:
        img = img.transpose(Image.FLIP_TOP_BOTTOM)
    out = {'hr': np.asarray(img.resize((CS, CS), Image.BICUBIC))}
    for scale in (2, 3):
        lr = img.resize((CS // scale, CS // scale), Image.BICUBIC)
        out['lr%d' % scale] = np.asarray(lr)
        out['bc%d' % scale] = np.asarray(lr.resize((CS, CS), Image.BICUBIC))
    return out


def main():
    rng = np.random.RandomState(20260)
    src = rng.randint(0, 256, (3, H, W, 3)).astype(np.uint8)
    offsets = [(0, 0), (H - CS, W - CS), (2, 1), (0, W - CS), (H - CS, 0), (3, 2)]
    cases = []
    for rv in range(4):
        for fliplr in (0, 1):
            for fliptb in (0, 1):
                k = len(cases)
                cases.append((k % 3, ) + offsets[k % len(offsets)] + (rv, fliplr, fliptb))
    cases.append((1, 3, 2, 1, 1, 0))                                   # the noise case: the last row
    z = rng.standard_normal((CS, CS, 3)).astype(np.float32)
    rows = {}
    for k, (s, y0, x0, rv, fliplr, fliptb) in enumerate(cases):
        noisy = k == len(cases) - 1
        item = reference_item(src[s], y0, x0, rv, fliplr, fliptb, SIGMA if noisy else 0.0, z if noisy else None)
        for name, a in item.items():
            rows.setdefault(name, []).append(a)
    out = os.path.join(ROOT, 'tests', 'golden', 'augment.npz')
    np.savez_compressed(out, src=src, cases=np.asarray(cases, np.int32), noise_sigma=np.float64(SIGMA), noise_z=z,
                        **{name: np.stack(v) for name, v in rows.items()})
    print('wrote %s (%d bytes, %d cases)' % (out, os.path.getsize(out), len(cases)))


if __name__ == '__main__':
    main()
