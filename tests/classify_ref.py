"""fp64 restatement (plain torch / numpy, no kernels) of the scene-classification evaluation, written from the reference's
Scene_classification_mfe.py: the VGG19 trunk, the preprocessing, the dense head with its closed-form backward, cross-entropy, Adam,
and the counter-based dropout function in numpy integers; the derived error bounds of the GPU tests; and the synthetic data set the
CPU test fixes and the GPU tests train on.  Nothing here reads the reference tree.

Every function takes a `dtype`: float64 is the reference, float32 on the CPU is the yardstick of the training test (the convention of
tests/reduction_ref.py: 8 x the error of stock fp32 torch, never below its FLOOR)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

U24 = 2.0 ** -24
HIDDEN = 256
LR, B1, B2, EPS = 1e-4, 0.9, 0.999, 1e-7

# torchvision vgg19.features: conv indices per block; a 2x2 max pool closes every block
BLOCKS = ((0, 2), (5, 7), (10, 12, 14, 16), (19, 21, 23, 25), (28, 30, 32, 34))


# ---- dropout: Philox4x32-10, first output word, keep when < 2^31 --------------------------------------------------------------- #
_M32 = np.uint64(0xFFFFFFFF)


def philox_first(e, step, seed):
    """First output word of Philox4x32-10 with counter {e lo, e hi, step lo, step hi} and key {seed lo, seed hi}; e: array of
    element indices.  Pure integer arithmetic on uint64 arrays (a product of two 32-bit words fits)."""
    e = np.asarray(e, dtype=np.uint64)
    step, seed = int(step), int(seed)
    c0, c1 = e & _M32, e >> np.uint64(32)
    c2 = np.full_like(e, step & 0xFFFFFFFF)
    c3 = np.full_like(e, (step >> 32) & 0xFFFFFFFF)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _M32)
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0


def dropout_keep(seed, step, rows, cols):
    """bool [rows, cols]: keep(seed, step, e = row * cols + col)."""
    e = np.arange(rows * cols, dtype=np.uint64)
    return (philox_first(e, step, seed) < np.uint64(1 << 31)).reshape(rows, cols)


# ---- preprocessing --------------------------------------------------------------------------------------------------------------- #
def channel_means_ref(images):
    """Script lines 111-118: np.mean over images of np.mean(image, axis=(0, 1)); images: iterable of uint8 [H, W, C]."""
    return np.mean([np.mean(im.astype(np.float64), axis=(0, 1)) for im in images], axis=0)


def preprocess_ref32(u8, means):
    """The fp32 expression, one rounding per operation: (float32(x) - float32(mean_c)) * float32(1 / 255)."""
    return (u8.astype(np.float32) - np.asarray(means, np.float64).astype(np.float32)) * np.float32(1.0 / 255.0)


# ---- VGG19 ----------------------------------------------------------------------------------------------------------------------- #
def tap_sequence():
    """[(torchvision features index, 'conv' | 'pool')] in forward order, from BLOCKS alone: the convs of a block, each followed by
    its ReLU (index + 1), then MaxPool2d(2, 2) right after the last ReLU (index + 2)."""
    seq = []
    for block in BLOCKS:
        seq += [(i, 'conv') for i in block]
        seq.append((block[-1] + 2, 'pool'))
    return seq


def vgg19_block_ref(f_nchw, state, b, dtype=torch.float64):
    """Block b (0..4) of the trunk on f_nchw [N, C, h, w]: its conv + ReLU layers, then the 2x2 max pool.  NCHW in, NCHW out."""
    f = f_nchw.to(dtype)
    for i in BLOCKS[b]:
        f = F.relu(F.conv2d(f, state['features.%d.weight' % i].to(f.device, dtype), state['features.%d.bias' % i].to(f.device, dtype),
                            padding=1))
    return F.max_pool2d(f, 2, 2)


def vgg19_ref(x_nhwc, state, dtype=torch.float64):
    """x_nhwc: [N, H, W, 3]; state: {'features.N.weight' / '.bias'}.  Returns the five pooled block outputs as [N, h, w, C]."""
    f = torch.as_tensor(x_nhwc).to(dtype).permute(0, 3, 1, 2)
    out = []
    for b in range(len(BLOCKS)):
        f = vgg19_block_ref(f, state, b, dtype)
        out.append(f.permute(0, 2, 3, 1).contiguous())
    return out


# ---- the head -------------------------------------------------------------------------------------------------------------------- #
def head_forward(x, p, keep=None):
    """p = dict(w1 [K, 256], b1, w2 [256, C], b2); keep: bool [m, 256] or None (inference).  Returns (pre, h, z)."""
    pre = x @ p['w1'] + p['b1']
    h = pre.clamp_min(0)
    if keep is not None:
        h = h * (2.0 * keep.to(h.dtype))
    return pre, h, h @ p['w2'] + p['b2']


def ce_ref(z, y):
    """Mean categorical cross-entropy from log-softmax (no clipping) and its gradient at z."""
    logp = torch.log_softmax(z, 1)
    m = z.shape[0]
    onehot = F.one_hot(y.long(), z.shape[1]).to(z.dtype)
    return -(logp * onehot).sum() / m, (logp.exp() - onehot) / m


def head_backward(x, p, pre, h, dz, keep=None):
    """Closed-form gradients of the mean loss: dict(w1, b1, w2, b2)."""
    dh = dz @ p['w2'].t()
    if keep is not None:
        dh = dh * (2.0 * keep.to(dh.dtype))
    dpre = dh * (pre > 0).to(dh.dtype)
    return {'w1': x.t() @ dpre, 'b1': dpre.sum(0), 'w2': h.t() @ dz, 'b2': dz.sum(0)}


def adam_update(p, g, st, t):
    """torch.optim.Adam's placement of eps: p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps).  st = dict(m, v) per name."""
    for k in p:
        st['m'][k] = st['m'][k] + (g[k] - st['m'][k]) * (1 - B1)
        st['v'][k] = st['v'][k] * B2 + (1 - B2) * g[k] * g[k]
        p[k] = p[k] - (LR / (1 - B1 ** t)) * (st['m'][k] / (st['v'][k].sqrt() / math.sqrt(1 - B2 ** t) + EPS))


class HeadRef:
    """The training loop of sradsgan_amd.classify.SceneClassifier restated: the same host random streams (numpy RandomState(seed) for
    the shuffles, the Philox function for the masks), arithmetic in `dtype` on the CPU."""

    def __init__(self, kernels, num_classes, dtype=torch.float64):
        self.dtype, self.c = dtype, num_classes
        self.set(kernels)

    def set(self, kernels):
        w1, w2 = kernels
        self.p = {'w1': w1.to(self.dtype).clone(), 'b1': torch.zeros(HIDDEN, dtype=self.dtype), 'w2': w2.to(self.dtype).clone(),
                  'b2': torch.zeros(self.c, dtype=self.dtype)}
        self.st = {'m': {k: torch.zeros_like(v) for k, v in self.p.items()}, 'v': {k: torch.zeros_like(v) for k, v in self.p.items()}}
        self.steps = 0

    def train_batch(self, xb, yb, seed):
        keep = torch.from_numpy(dropout_keep(seed, self.steps, xb.shape[0], HIDDEN))
        pre, h, z = head_forward(xb.to(self.dtype), self.p, keep)
        loss, dz = ce_ref(z, yb)
        g = head_backward(xb.to(self.dtype), self.p, pre, h, dz, keep)
        self.steps += 1
        adam_update(self.p, g, self.st, self.steps)
        return float(loss), z

    def logits(self, X):
        return head_forward(X.to(self.dtype), self.p)[2]

    def epochs(self, X, y, epochs, batch_size, seed, Xval=None, yval=None):
        rng = np.random.RandomState(seed)
        val_loss = []
        for _ in range(epochs):
            order = torch.from_numpy(rng.permutation(X.shape[0]))
            Xs, ys = X[order], y[order]
            for a in range(0, X.shape[0], batch_size):
                self.train_batch(Xs[a:a + batch_size], ys[a:a + batch_size], seed)
            if Xval is not None:
                val_loss.append(float(ce_ref(self.logits(Xval), yval)[0]))
        return val_loss

    def fit_refit(self, kernels_fit, kernels_refit, Xtr, ytr, Xval, yval, epochs, batch_size, seed):
        """fit on train with validation, then refit a fresh model on train + validate for argmin(val_loss) + 1 epochs."""
        self.set(kernels_fit)
        val_loss = self.epochs(Xtr, ytr, epochs, batch_size, seed, Xval, yval)
        best = int(np.argmin(val_loss)) + 1
        self.set(kernels_refit)
        X, y = torch.cat([Xtr, Xval]), torch.cat([ytr, yval])
        order = torch.from_numpy(np.random.RandomState(seed + 1).permutation(X.shape[0]))
        self.epochs(X[order], y[order], best, batch_size, seed + 1)
        return best


# ---- derived bounds -------------------------------------------------------------------------------------------------------------- #
def gamma(length):
    """Higham's gamma_L = L u / (1 - L u), u = 2^-24: |fl(sum of L products) - exact| <= gamma_L * sum |a_i b_i| in ANY order."""
    return length * U24 / (1.0 - length * U24)


def dense_bound(a, b, bias=None):
    """Element-wise bound of fl(a @ b (+ bias)) for fp32 operands: gamma_L * (|a| @ |b| (+ |bias|)), L = the products plus the bias
    addition.  (ReLU is exact; doubling by the dropout is exact.)"""
    a, b = a.double().abs(), b.double().abs()
    length = a.shape[1] + (1 if bias is not None else 0)
    s = a @ b
    if bias is not None:
        s = s + bias.double().abs()
    return gamma(length) * s + 1e-45


def conv_gain(weight):
    """An upper bound of the 2-norm gain of a zero-padded stride-1 conv with this [Cout, Cin, kh, kw] weight: the conv is the sum
    over its taps of a shift (which cannot lengthen a vector) followed by the tap's Cout x Cin matrix at every pixel, so
    || conv(e) ||_2 <= sum over taps || W_tap ||_2 * || e ||_2.  ReLU and the 2x2 max pool move no output by more than their inputs
    move, so they do not raise it.  This is what carries a layer's error bar through the layers after it."""
    w = weight.detach().cpu().double()
    return float(sum(torch.linalg.matrix_norm(w[:, :, i, j], 2) for i in range(w.shape[2]) for j in range(w.shape[3])))


CE_OPS = 16


def ce_bounds(z, y, scale):
    """Bounds of one softmax-CE row pass in fp32, from its operation count.  With x = z - max (one rounding: u |x|), e = exp(x)
    (<= 2 ulp; its argument's rounding moves it by |x| u relatively), s = sum e over a 6-level butterfly (6 u), log s (<= 2 ulp of
    |log s|, plus the relative error of s), p = e / s (one more u):
        loss_r  = log s - x_y    : u * (CE_OPS + 2 |x_y| + 2 |log s| + sum_i p_i |x_i|)
        dlogit  = (p - 1{i=y}) k : k u * (p_i (CE_OPS + |x_i| + sum_j p_j |x_j|) + 2 |p_i - 1{i=y}|) + 2^-126 k (flushed tails of exp)
    CE_OPS = 16 counts the roundings named above (1 + 2 + 6 + 2 + 1 + the final subtraction and product) with the 2 ulp of expf and
    logf taken as 4 u each way.  Returns (loss bound [m], dlogits bound [m, C]) as float64 tensors."""
    z = z.double()
    x = z - z.max(1, keepdim=True).values
    e = x.exp()
    s = e.sum(1, keepdim=True)
    p = e / s
    onehot = F.one_hot(y.long(), z.shape[1]).double()
    px = (p * x.abs()).sum(1, keepdim=True)
    xy = (x * onehot).sum(1, keepdim=True).abs()
    loss_b = U24 * (CE_OPS + 2 * xy + 2 * s.log().abs() + px)
    d_b = scale * U24 * (p * (CE_OPS + x.abs() + px) + 2 * (p - onehot).abs()) + scale * 2.0 ** -126
    return loss_b[:, 0], d_b


def err(got, ref):
    """max |got - ref| / max |ref| of one tensor (tests/reduction_ref.py's measure)."""
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    if not bool(torch.isfinite(got).all()):
        return float('inf')
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


# ---- the synthetic data set ------------------------------------------------------------------------------------------------------ #
DATA_CLASSES, DATA_PER_CLASS, DATA_SIZE, DATA_SEED = 3, 20, 32, 20261
SPLIT_SEED, FIT_SEED, FIT_EPOCHS, FIT_BATCH = 5, 11, 60, 8


def synthetic_tiles(classes=DATA_CLASSES, per_class=DATA_PER_CLASS, size=DATA_SIZE, seed=DATA_SEED):
    """uint8 [classes * per_class, size, size, 3] and int64 labels: every class has its own tint and its own texture (horizontal
    stripes, vertical stripes, checkerboard, ... of a class-specific period), every tile its own phase, contrast and noise."""
    rng = np.random.RandomState(seed)
    tints = np.array([[200, 80, 60], [60, 190, 90], [70, 90, 210], [190, 190, 60], [180, 70, 190], [70, 190, 190]], np.float64)
    yy, xx = np.mgrid[0:size, 0:size]
    imgs, labels = [], []
    for k in range(classes):
        period = 4 + 2 * (k // 3)
        for _ in range(per_class):
            ph = rng.randint(0, period)
            kind = k % 3
            wave = (((yy + ph) // (period // 2)) % 2) if kind == 0 else ((((xx + ph) // (period // 2)) % 2) if kind == 1 else
                                                                         ((((yy + ph) // (period // 2)) + (xx // (period // 2))) % 2))
            amp = 35.0 + 15.0 * rng.rand()
            im = tints[k % len(tints)][None, None, :] + amp * (2.0 * wave[:, :, None] - 1.0) + 6.0 * rng.randn(size, size, 3)
            imgs.append(np.clip(np.rint(im), 0, 255).astype(np.uint8))
            labels.append(k)
    return np.stack(imgs), np.asarray(labels, np.int64)
