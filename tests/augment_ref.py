"""numpy restatement of the dihedral kernels (csrc/augment.hip) written from what include/sradsgan_hip.h documents, not from the
kernels: crop, float64 noise, op, inverse op, and the fixed-order fp32 merge.  tests/test_augment_cpu.py holds it against Pillow
and against tests/golden/augment.npz; the GPU tests hold the kernels against it."""
import numpy as np

# (rv, fliplr, fliptb) -> op, written out by hand (the package computes its table): Pillow rotate(90 rv, expand=True), then
# FLIP_LEFT_RIGHT, then FLIP_TOP_BOTTOM
OP_OF = {(0, 0, 0): 0, (0, 0, 1): 2, (0, 1, 0): 4, (0, 1, 1): 6,
         (1, 0, 0): 3, (1, 0, 1): 1, (1, 1, 0): 7, (1, 1, 1): 5,
         (2, 0, 0): 6, (2, 0, 1): 4, (2, 1, 0): 2, (2, 1, 1): 0,
         (3, 0, 0): 5, (3, 0, 1): 7, (3, 1, 0): 1, (3, 1, 1): 3}
INVERSE = (0, 1, 2, 5, 4, 3, 6, 7)


def apply_op(a, op, axes=(0, 1)):
    """y = fliplr^b2(flipud^b1(transpose^b0(a))) on the two axes `axes` = (rows, columns)."""
    r, c = axes
    if op & 1:
        a = np.swapaxes(a, r, c)
    if op & 2:
        a = np.flip(a, r)
    if op & 4:
        a = np.flip(a, c)
    return np.ascontiguousarray(a)


def add_noise(crop_u8, sigma, z):
    """numpy's (img + noises).clip(0, 255).astype(uint8) of dataset.py:289-290 with noises = sigma * z in float64."""
    x = crop_u8.astype(np.float64) + np.float64(sigma) * z.astype(np.float64)
    return np.trunc(x.clip(0, 255)).astype(np.uint8)


def augment(src, params, cs, sigma=0.0, z=None):
    """src uint8 [N, H, W, C], params int [N, 4] = (y0, x0, op, 0), z float32 [N, cs, cs, C] or None -> uint8 [N, cs, cs, C]."""
    out = np.empty((src.shape[0], cs, cs, src.shape[3]), np.uint8)
    for n in range(src.shape[0]):
        y0, x0, op = (int(v) for v in params[n][:3])
        assert 0 <= y0 <= src.shape[1] - cs and 0 <= x0 <= src.shape[2] - cs and 0 <= op < 8
        crop = src[n, y0:y0 + cs, x0:x0 + cs]
        if sigma:
            crop = add_noise(crop, sigma, z[n])
        out[n] = apply_op(crop, op)
    return out


def merge(views, ops):
    """views[k] float32 [N, C, *, *] of the shape of ops[k](result) -> (((u_0 + u_1) + ...) + u_{m-1}) * fp32(1 / m), u_k the view
    mapped back, every operation rounded to fp32."""
    acc = None
    for v, op in zip(views, ops):
        u = apply_op(np.asarray(v, np.float32), INVERSE[op], axes=(2, 3))
        acc = u if acc is None else (acc + u).astype(np.float32)
    return (acc * (np.float32(1.0) / np.float32(len(views)))).astype(np.float32)
