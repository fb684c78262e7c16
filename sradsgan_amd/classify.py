"""Scene-classification evaluation of SR outputs on the device: the reference's `Scene_classification_mfe.py` --
does a land-use classifier recognise super-resolved tiles better than bicubic ones? -- without TensorFlow and without the folders of
PNGs between its stages: HR uint8 -> LR -> generator -> uint8 -> VGG19 bottleneck features -> dense head -> confusion matrix.

  VGG19Features     keras.applications.VGG19(include_top=False): 16 conv + ReLU (the ordinary conv kernels, bias + ReLU epilogue) and
                    five 2x2 max pools; channels-last output [n, H/32, W/32, 512].  Structure here, weights from the user
                    (`load_torchvision_vgg19`), the precedent of FeatureExtractor and LPIPS; until then a deterministic init.
  preprocess        ImageDataGenerator(rescale=1/255, preprocessing_function=x - channel_means): Keras applies the function first
                    and the rescale second, so in fp32 (float(x) - mean_c) * fp32(1/255)        (script lines 151, 255)
  channel_means     the mean over images of each image's per-channel mean of raw 0..255 values   (script lines 111-118)
  SceneClassifier   build_fully_connected (script lines 239-250) + train() (252-311): Flatten in NHWC order, Dense(256), ReLU,
                    Dropout(0.5), Dense(num_classes), softmax; Adam(lr 1e-4, eps 1e-7) on one flat arena (srhip_adam_step)
  classify_sr / classify_folder   evaluate() (313-352) with the PNG round trip removed

The head's arithmetic (csrc/classify.hip) is exact fp32 and does not depend on the conv arithmetic mode.  Departures from the
script are listed in DESIGN 9."""
import ctypes
import math
import os
from fractions import Fraction

import numpy as np
import torch
import torch.nn as nn

from . import _hip, data as sdata, ops

# torchvision.models.vgg19().features: index -> (cin, cout) of every conv; ReLU follows each, MaxPool2d(2, 2) sits at POOLS
CONVS = {0: (3, 64), 2: (64, 64), 5: (64, 128), 7: (128, 128), 10: (128, 256), 12: (256, 256), 14: (256, 256), 16: (256, 256),
         19: (256, 512), 21: (512, 512), 23: (512, 512), 25: (512, 512), 28: (512, 512), 30: (512, 512), 32: (512, 512), 34: (512, 512)}
POOLS = (4, 9, 18, 27, 36)
HIDDEN = 256                      # Dense(256), script line 245
MAX_ROWS = 64                     # rows per dense call = the script's batch size
LR, B1, B2, EPS = 1e-4, 0.9, 0.999, 1e-7          # keras.optimizers.Adam(lr=0.0001) and Keras's defaults


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _require_u8(t, what):
    if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() != 4:
        raise TypeError('%s expects a [N, H, W, C] uint8 tensor' % what)
    if not t.is_cuda:
        raise RuntimeError('%s: runs on the MI355X HIP path only (got a %s tensor); there is no CPU fallback' % (what, t.device.type))


# ------------------------------------------------------------------------------------------------------------------------------ #
# input statistics and preprocessing
# ------------------------------------------------------------------------------------------------------------------------------ #
def channel_sums(u8_nhwc):
    """[N, H, W, C] uint8 on the device -> int64 [N, C]: the exact per-image per-channel sums."""
    _require_u8(u8_nhwc, 'channel_sums')
    u8 = u8_nhwc.contiguous()
    n, h, w, c = u8.shape
    lib = _hip.lib()
    ws = torch.empty(max(1, lib.srhip_cls_channel_sums_workspace(n, h, w) // 8), device=u8.device, dtype=torch.int64)
    out = torch.empty(n, c, device=u8.device, dtype=torch.int64)
    _hip.check(lib.srhip_cls_channel_sums(_p(u8), _p(out), _p(ws), ws.numel() * 8, n, h, w, c, _stream()), 'cls_channel_sums')
    return out


def channel_means(batches):
    """The script's `channel_means` (lines 111-118): np.mean over images of np.mean(image, axis=(0, 1)).  batches: one uint8
    [N, H, W, C] device tensor or a sequence of them (sizes may differ between batches).  The sums are integers, the mean of the
    per-image means is formed in exact rationals and rounded once: float64 [C], independent of the order of the images."""
    batches = [batches] if torch.is_tensor(batches) else list(batches)
    total, count = None, 0
    for b in batches:
        s = channel_sums(b).cpu().numpy()
        hw = int(b.shape[1]) * int(b.shape[2])
        if total is None:
            total = [Fraction(0)] * s.shape[1]
        for row in s:
            total = [t + Fraction(int(v), hw) for t, v in zip(total, row)]
        count += s.shape[0]
    if not count:
        raise ValueError('channel_means: no images')
    return np.array([float(t / count) for t in total], np.float64)


def _means_tensor(means, c, device):
    m = torch.as_tensor(np.asarray(means.detach().cpu() if torch.is_tensor(means) else means, dtype=np.float64).astype(np.float32))
    if m.numel() != c:
        raise ValueError('preprocess: %d channel means for %d channels' % (m.numel(), c))
    return m.reshape(c).to(device)


def preprocess(u8_nhwc, means):
    """[N, H, W, C] uint8 on the device, C channel means (raw 0..255 scale) -> float32 [N, H, W, C] =
    (float(x) - fp32(mean_c)) * fp32(1 / 255)."""
    _require_u8(u8_nhwc, 'preprocess')
    u8 = u8_nhwc.contiguous()
    m = _means_tensor(means, u8.shape[3], u8.device)
    out = torch.empty(u8.shape, device=u8.device, dtype=torch.float32)
    _hip.check(_hip.lib().srhip_cls_preprocess(_p(u8), _p(m), _p(out), u8.numel(), u8.shape[3], _stream()), 'cls_preprocess')
    return out


# ------------------------------------------------------------------------------------------------------------------------------ #
# VGG19 without its top
# ------------------------------------------------------------------------------------------------------------------------------ #
class _Conv(nn.Module):
    """Parameter holder with nn.Conv2d's names (weight OIHW, bias)."""

    def __init__(self, cin, cout):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin, 3, 3), requires_grad=False)
        self.bias = nn.Parameter(torch.empty(cout), requires_grad=False)


class VGG19Features(nn.Module):
    """keras.applications.VGG19(include_top=False) (script line 237), forward only, frozen."""

    def __init__(self):
        super().__init__()
        self.features = nn.Sequential(*[_Conv(*CONVS[i]) if i in CONVS else nn.Identity() for i in range(37)])
        g = torch.Generator().manual_seed(0)                       # deterministic init; real use loads the pretrained file
        with torch.no_grad():
            for i, (cin, _) in CONVS.items():
                bound = math.sqrt(6.0 / (cin * 9))
                self.features[i].weight.copy_((torch.rand(self.features[i].weight.shape, generator=g) * 2 - 1) * bound)
                self.features[i].bias.zero_()
        ops.mark_static(self)
        self.eval()

    def load_torchvision_vgg19(self, state_dict):
        """torchvision VGG19 state dict: `features.N.{weight,bias}` of all 16 convs are taken, every other key is ignored."""
        named = {}
        for i in CONVS:
            for leaf in ('weight', 'bias'):
                key = 'features.%d.%s' % (i, leaf)
                if key not in state_dict:
                    raise KeyError('load_torchvision_vgg19: %s is missing' % key)
                param = getattr(self.features[i], leaf)
                if tuple(state_dict[key].shape) != tuple(param.shape):
                    raise ValueError('load_torchvision_vgg19: %s has shape %s, expected %s'
                                     % (key, tuple(state_dict[key].shape), tuple(param.shape)))
                named[key] = (param, state_dict[key])
        with torch.no_grad():
            for param, value in named.values():
                param.copy_(value)                                 # bumps the version: packed images are rebuilt on next use
        return sorted(named)

    @torch.no_grad()
    def forward(self, x_nhwc, taps=False):
        """x_nhwc: float32 [N, H, W, 3] (preprocess's output), H and W multiples of 32 -> [N, H/32, W/32, 512], channels last.
        taps=True: also the list of (torchvision index, tensor) of every conv + ReLU and pool output, as logical NCHW."""
        if x_nhwc.dim() != 4 or x_nhwc.shape[3] != 3:
            raise ValueError('VGG19Features: input must be [N, H, W, 3] float32, got %s' % (tuple(x_nhwc.shape),))
        if x_nhwc.shape[1] % 32 or x_nhwc.shape[2] % 32 or not x_nhwc.shape[1] or not x_nhwc.shape[2]:
            raise ValueError('VGG19Features: H and W must be positive multiples of 32 (five 2x2 pools), got %d x %d'
                             % (x_nhwc.shape[1], x_nhwc.shape[2]))
        ops._require_gpu(x_nhwc, 'VGG19Features')
        if ops.get_conv_math() == 'half':                # an evaluation must not move with the training arithmetic
            with ops.conv_math('bf16x3'):
                return self.forward(x_nhwc, taps)
        f = x_nhwc.contiguous().permute(0, 3, 1, 2)      # logical NCHW over channels-last memory: no copy
        seen = []
        for i in range(37):
            if i in CONVS:
                conv = self.features[i]
                f = ops.conv2d_fwd_raw(f, conv.weight, conv.bias, 1, 1, slope=0.0)      # conv + bias + ReLU in one kernel
            elif i in POOLS:
                f = ops.max_pool2x2_raw(f)
            else:
                continue
            if taps:
                seen.append((i, f))
        out = f.permute(0, 2, 3, 1)
        return (out, seen) if taps else out


# ------------------------------------------------------------------------------------------------------------------------------ #
# the head
# ------------------------------------------------------------------------------------------------------------------------------ #
def dense_fwd(x, w, bias=None, relu=False, dropout=None):
    """y[m, N] = x[m, K] @ w[K, N] + bias, m <= 64, K % 8 == 0, exact fp32 (csrc/classify.hip).  dropout: None or (seed, step)."""
    _check_dense(x, w, 'dense_fwd')
    m, k = x.shape
    n = w.shape[1]
    if bias is not None:
        ops._require_gpu(bias, 'dense_fwd')
        if bias.device != x.device or bias.dtype != torch.float32 or tuple(bias.shape) != (n,) or not bias.is_contiguous():
            raise ValueError('dense_fwd: bias must be a contiguous float32 [%d] on %s, got %s %s on %s'
                             % (n, x.device, bias.dtype, tuple(bias.shape), bias.device))
    lib = _hip.lib()
    part = torch.empty(lib.srhip_cls_dense_chunks(k) * m * n, device=x.device, dtype=torch.float32)
    y = torch.empty(m, n, device=x.device, dtype=torch.float32)
    seed, step = dropout if dropout is not None else (0, 0)
    _hip.check(lib.srhip_cls_dense_fwd(_p(x), _p(w), _p(bias), _p(y), _p(part), part.numel() * 4, m, k, n, int(bool(relu)),
                                       int(dropout is not None), int(seed), int(step), _stream()), 'cls_dense_fwd')
    return y


def dense_wgrad(x, dy, dw=None, db=None):
    """dw[K, N] = x[m, K]^T @ dy[m, N] and db[N] = dy.sum(0), written into dw / db when given."""
    _check_dense(x, None, 'dense_wgrad')
    _check_dense(dy, None, 'dense_wgrad')
    m, k = x.shape
    n = dy.shape[1]
    if dy.shape[0] != m:
        raise ValueError('dense_wgrad: x has %d rows, dy %d' % (m, dy.shape[0]))
    dw = torch.empty(k, n, device=x.device, dtype=torch.float32) if dw is None else dw
    db = torch.empty(n, device=x.device, dtype=torch.float32) if db is None else db
    if tuple(dw.shape) != (k, n) or tuple(db.shape) != (n,) or not dw.is_contiguous() or not db.is_contiguous():
        raise ValueError('dense_wgrad: destinations must be contiguous [%d, %d] and [%d]' % (k, n, n))
    _hip.check(_hip.lib().srhip_cls_dense_wgrad(_p(x), _p(dy), _p(dw), _p(db), m, k, n, _stream()), 'cls_dense_wgrad')
    return dw, db


def dense_dgrad(dy, w, act=None, dropout=None):
    """dx[m, K] = dy[m, N] @ w[K, N]^T; with `act` (the [m, K] output of the layer below) also that layer's ReLU backward, and with
    dropout = (seed, step) its dropout backward (the mask is recomputed)."""
    _check_dense(dy, None, 'dense_dgrad')
    _check_dense(w, None, 'dense_dgrad')
    m, n = dy.shape
    k = w.shape[0]
    if w.shape[1] != n or (act is not None and (tuple(act.shape) != (m, k) or not act.is_contiguous())):
        raise ValueError('dense_dgrad: shapes do not match')
    dx = torch.empty(m, k, device=dy.device, dtype=torch.float32)
    seed, step = dropout if dropout is not None else (0, 0)
    _hip.check(_hip.lib().srhip_cls_dense_dgrad(_p(dy), _p(w), _p(act), _p(dx), m, k, n, int(act is not None), int(dropout is not None),
                                                int(seed), int(step), _stream()), 'cls_dense_dgrad')
    return dx


def _check_dense(x, w, what):
    ops._require_gpu(x, what)
    if x.dim() != 2 or not x.is_contiguous():
        raise ValueError('%s: operands are contiguous 2-d tensors, got %s' % (what, tuple(x.shape)))
    if w is not None:
        ops._require_gpu(w, what)
        if w.dim() != 2 or not w.is_contiguous() or w.shape[0] != x.shape[1]:
            raise ValueError('%s: weight must be contiguous [K, N] with K = %d, got %s' % (what, x.shape[1], tuple(w.shape)))
        if x.shape[0] > MAX_ROWS or x.shape[0] < 1 or x.shape[1] % 8:
            raise ValueError('%s: 1 <= rows <= %d and K %% 8 == 0 (got %s)' % (what, MAX_ROWS, tuple(x.shape)))


def softmax_ce(logits, labels, scale=None, need_grad=True):
    """logits float32 [m, C <= 64], labels int32 [m] -> (row_loss float32 [m], loss_sum float64 [1], dlogits or None); dlogits =
    (softmax - onehot) * scale, scale = 1 / m by default (the mean over the batch, as Keras reduces)."""
    ops._require_gpu(logits, 'softmax_ce')
    m, c = logits.shape
    if labels.dtype != torch.int32 or tuple(labels.shape) != (m,) or not logits.is_contiguous():
        raise ValueError('softmax_ce: labels must be int32 [%d] and logits contiguous' % m)
    row = torch.empty(m, device=logits.device, dtype=torch.float32)
    total = torch.empty(1, device=logits.device, dtype=torch.float64)
    d = torch.empty_like(logits) if need_grad else None
    _hip.check(_hip.lib().srhip_cls_softmax_ce_fwd_bwd(_p(logits), _p(labels), _p(row), _p(total), _p(d), m, c,
                                                       float(1.0 / m if scale is None else scale), _stream()), 'cls_softmax_ce')
    return row, total, d


def argmax_confusion(logits, labels=None, table=None):
    """First-index arg-max of every row -> int32 [m]; with labels (int32 [m]) and table (int32 [C, C], accumulated into):
    ++table[label, arg]."""
    ops._require_gpu(logits, 'argmax_confusion')
    m, c = logits.shape
    pred = torch.empty(m, device=logits.device, dtype=torch.int32)
    if table is not None and (table.dtype != torch.int32 or tuple(table.shape) != (c, c) or not table.is_contiguous()
                              or labels is None or labels.dtype != torch.int32 or tuple(labels.shape) != (m,)):
        raise ValueError('argmax_confusion: table must be int32 [%d, %d] with int32 labels [%d]' % (c, c, m))
    _hip.check(_hip.lib().srhip_cls_confusion(_p(logits.contiguous()), _p(labels), _p(pred), _p(table), m, c, _stream()),
               'cls_confusion')
    return pred


def report_from_confusion(cm):
    """sklearn's classification_report numbers from a confusion matrix [true, pred]: per class precision / recall / f1 / support, the
    macro and the support-weighted averages, and the accuracy.  A ratio with a zero denominator is 0 (sklearn's zero_division
    default, which also warns)."""
    cm = np.asarray(cm, dtype=np.int64)
    tp = np.diag(cm).astype(np.float64)
    predicted, support = cm.sum(0).astype(np.float64), cm.sum(1).astype(np.float64)

    def ratio(a, b):
        return np.divide(a, b, out=np.zeros_like(a, dtype=np.float64), where=b > 0)
    precision, recall = ratio(tp, predicted), ratio(tp, support)
    f1 = ratio(2 * precision * recall, precision + recall)
    total = support.sum()
    rep = {'classes': [dict(precision=float(precision[i]), recall=float(recall[i]), f1=float(f1[i]), support=int(support[i]))
                       for i in range(cm.shape[0])]}
    rep['macro avg'] = dict(precision=float(precision.mean()), recall=float(recall.mean()), f1=float(f1.mean()), support=int(total))
    wts = support / total if total > 0 else support
    rep['weighted avg'] = dict(precision=float((precision * wts).sum()), recall=float((recall * wts).sum()),
                               f1=float((f1 * wts).sum()), support=int(total))
    rep['accuracy'] = float(tp.sum() / total) if total > 0 else 0.0
    return rep


def split_indices(labels, seed):
    """The script's per-class split (lines 69-82): a random permutation of every class, the first 65 % for training, the next 10 %
    for validation, the rest (25 %) for testing.  Returns three int64 index arrays, classes in ascending order."""
    labels = np.asarray(labels.detach().cpu() if torch.is_tensor(labels) else labels).astype(np.int64)
    rng = np.random.RandomState(seed)
    parts = ([], [], [])
    for cls in np.unique(labels):
        idx = np.flatnonzero(labels == cls)
        idx = idx[rng.permutation(len(idx))]
        n_tr, n_va = int(round(0.65 * len(idx))), int(round(0.10 * len(idx)))
        for part, sl in zip(parts, (idx[:n_tr], idx[n_tr:n_tr + n_va], idx[n_tr + n_va:])):
            part.append(sl)
    return tuple(np.concatenate(p) for p in parts)


def initial_kernels(k, num_classes, seed):
    """The head's initial kernels on the host: Keras's glorot_uniform (limit sqrt(6 / (fan_in + fan_out))) from a seeded generator,
    float32 [k, 256] and [256, num_classes].  Biases start at zero."""
    g = torch.Generator().manual_seed(int(seed))
    out = []
    for shape in ((int(k), HIDDEN), (HIDDEN, int(num_classes))):
        limit = math.sqrt(6.0 / (shape[0] + shape[1]))
        out.append((torch.rand(shape, generator=g) * 2 - 1) * limit)
    return out


class SceneClassifier:
    """build_fully_connected + its training (script lines 239-311).  Parameters w1 [K, 256], b1, w2 [256, C], b2 are views of one flat
    fp32 arena (Keras's kernel layout: input-major), with gradient and Adam moment arenas beside it."""

    def __init__(self, num_classes, feature_shape, device='cuda:0', seed=0):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('SceneClassifier: runs on the MI355X HIP path only (got device %s); there is no CPU fallback' % device)
        self.num_classes, self.feature_shape = int(num_classes), tuple(int(s) for s in feature_shape)
        self.k = int(np.prod(self.feature_shape))
        if not 2 <= self.num_classes <= 64 or self.k % 8:
            raise ValueError('SceneClassifier: 2 <= num_classes <= 64 and a feature count that is a multiple of 8 (got %d, %d)'
                             % (self.num_classes, self.k))
        sizes = [self.k * HIDDEN, HIDDEN, HIDDEN * self.num_classes, self.num_classes]
        self._offsets = np.concatenate([[0], np.cumsum([-(-s // 4) * 4 for s in sizes])])     # every tensor 16-byte aligned
        self._shapes = [(self.k, HIDDEN), (HIDDEN,), (HIDDEN, self.num_classes), (self.num_classes,)]
        numel = int(self._offsets[-1])
        self.flat_p, self.flat_g = (torch.zeros(numel, device=self.device) for _ in range(2))
        self.exp_avg, self.exp_avg_sq = (torch.zeros(numel, device=self.device) for _ in range(2))
        self.state = torch.zeros(4, device=self.device)
        self.w1, self.b1, self.w2, self.b2 = self._views(self.flat_p)
        self.gw1, self.gb1, self.gw2, self.gb2 = self._views(self.flat_g)
        self.step_count = 0
        self.reset(seed)

    def _views(self, flat):
        return [flat[int(o):int(o) + int(np.prod(s))].view(s) for o, s in zip(self._offsets[:-1], self._shapes)]

    def reset(self, seed=0):
        """A fresh model and a fresh optimiser: Keras's glorot_uniform kernels (limit sqrt(6 / (fan_in + fan_out))) from a seeded
        host generator, zero biases, zero moments, step 0."""
        self.flat_p.zero_()
        for w, init in zip((self.w1, self.w2), initial_kernels(self.k, self.num_classes, seed)):
            w.copy_(init)
        for t in (self.flat_g, self.exp_avg, self.exp_avg_sq, self.state):
            t.zero_()
        self.step_count = 0

    def parameters(self):
        return {'w1': self.w1, 'b1': self.b1, 'w2': self.w2, 'b2': self.b2}

    def _flat(self, X):
        X = X.reshape(X.shape[0], -1)
        if X.shape[1] != self.k:
            raise ValueError('SceneClassifier: %d features per sample, expected %d' % (X.shape[1], self.k))
        ops._require_gpu(X, 'SceneClassifier')
        return X.contiguous()                             # Flatten of [n, h, w, c] features: (h, w, c) order

    @staticmethod
    def _labels(y, device):
        return torch.as_tensor(np.asarray(y.detach().cpu() if torch.is_tensor(y) else y)).to(torch.int32).to(device)

    def logits(self, xb, dropout=None):
        h = dense_fwd(xb, self.w1, self.b1, relu=True, dropout=dropout)
        return h, dense_fwd(h, self.w2, self.b2)

    def train_batch(self, xb, yb, seed):
        """One optimiser step on rows xb [m <= 64, K] with int32 labels yb; returns (the batch's loss sum, float64 [1] on the device,
        the logits [m, C] the step was taken from).  The dropout mask is the function of (seed, number of steps taken so far,
        element)."""
        drop = (int(seed), self.step_count)
        h, z = self.logits(xb, dropout=drop)
        _, total, dz = softmax_ce(z, yb)
        dense_wgrad(h, dz, self.gw2, self.gb2)
        dh = dense_dgrad(dz, self.w2, act=h, dropout=drop)
        dense_wgrad(xb, dh, self.gw1, self.gb1)
        _hip.check(_hip.lib().srhip_adam_step(_p(self.flat_p), _p(self.flat_g), _p(self.exp_avg), _p(self.exp_avg_sq), _p(self.state),
                                              self.flat_p.numel(), LR, B1, B2, EPS, 1.0, 0.0, _stream()), 'adam_step')
        self.step_count += 1
        return total, z

    def _run_eval(self, X, y=None, table=None):
        """Inference over all rows in slabs of 64: (predictions int32 [n], loss sum float64 [1] or None)."""
        if not X.shape[0]:
            raise ValueError('SceneClassifier: no rows to classify')
        preds, total = [], None
        for a in range(0, X.shape[0], MAX_ROWS):
            _, z = self.logits(X[a:a + MAX_ROWS])
            yb = y[a:a + MAX_ROWS] if y is not None else None
            preds.append(argmax_confusion(z, yb, table))
            if y is not None:
                _, t, _ = softmax_ce(z, yb, need_grad=False)
                total = t if total is None else total + t
        return torch.cat(preds), total

    def _epochs(self, X, y, epochs, batch_size, seed, Xval=None, yval=None):
        rng = np.random.RandomState(seed)
        n = X.shape[0]
        hist = {'loss': [], 'accuracy': [], 'val_loss': [], 'val_accuracy': []}
        for _ in range(int(epochs)):
            order = torch.from_numpy(rng.permutation(n)).to(self.device)
            Xs, ys = X.index_select(0, order), y.index_select(0, order)
            total, hits = torch.zeros(1, device=self.device, dtype=torch.float64), torch.zeros((), device=self.device, dtype=torch.int64)
            for a in range(0, n, batch_size):                                   # the partial last batch is kept, as Keras keeps it
                yb = ys[a:a + batch_size]
                t, z = self.train_batch(Xs[a:a + batch_size], yb, seed)
                total += t
                hits += (argmax_confusion(z) == yb).sum()
            hist['loss'].append(float(total) / n)
            hist['accuracy'].append(int(hits) / n)
            if Xval is not None:
                pred, vt = self._run_eval(Xval, yval)
                hist['val_loss'].append(float(vt) / Xval.shape[0])
                hist['val_accuracy'].append(int((pred == yval).sum()) / Xval.shape[0])
        return hist

    def fit(self, Xtr, ytr, Xval, yval, epochs=100, batch_size=64, seed=0):
        """model.fit(..., validation_data=...) (script lines 275-280) on a fresh model.  Returns (history, argmin(val_loss) + 1)."""
        if not 1 <= int(batch_size) <= MAX_ROWS:
            raise ValueError('fit: 1 <= batch_size <= %d' % MAX_ROWS)
        self.reset(seed)
        hist = self._epochs(self._flat(Xtr), self._labels(ytr, self.device), epochs, int(batch_size), seed,
                            self._flat(Xval), self._labels(yval, self.device))
        return hist, int(np.argmin(hist['val_loss'])) + 1

    def refit(self, X, y, epochs, batch_size=64, seed=0):
        """The script's second training (lines 282-294): a fresh model on train + validate, shuffled once, for the epochs `fit`
        found.  The optimiser is fresh too (the script reuses its Adam object: DESIGN 9)."""
        if not 1 <= int(batch_size) <= MAX_ROWS:
            raise ValueError('refit: 1 <= batch_size <= %d' % MAX_ROWS)
        self.reset(seed + 1)
        X, y = self._flat(X), self._labels(y, self.device)
        order = torch.from_numpy(np.random.RandomState(seed + 1).permutation(X.shape[0])).to(self.device)
        return self._epochs(X.index_select(0, order), y.index_select(0, order), epochs, int(batch_size), seed + 1)

    def predict(self, X):
        """model.predict_classes: the arg-max class of every row (the first index on ties), int64 on the device."""
        return self._run_eval(self._flat(X))[0].long()

    def evaluate(self, X, y):
        """accuracy_score, confusion_matrix [true, pred] (int64 numpy) and classification_report's numbers (script lines 320-327)."""
        table = torch.zeros(self.num_classes, self.num_classes, device=self.device, dtype=torch.int32)
        pred, _ = self._run_eval(self._flat(X), self._labels(y, self.device), table)
        cm = table.cpu().numpy().astype(np.int64)
        rep = report_from_confusion(cm)
        return {'accuracy': rep['accuracy'], 'confusion': cm, 'report': rep, 'pred': pred.long().cpu().numpy()}


# ------------------------------------------------------------------------------------------------------------------------------ #
# evaluate() without the PNG round trip
# ------------------------------------------------------------------------------------------------------------------------------ #
def _conform(u8, hw):
    """Keras's flow_from_directory loads every image at target_size with nearest interpolation: a batch of another size is resized on
    the host with PIL nearest.  Batches of the right size pass untouched."""
    if tuple(u8.shape[1:3]) == tuple(hw):
        return u8
    from PIL import Image
    host = u8.cpu().numpy()
    out = np.stack([np.asarray(Image.fromarray(im).resize((hw[1], hw[0]), Image.NEAREST)) for im in host])
    return torch.from_numpy(out).to(u8.device)


def quantise(sr):
    """save_img1 (utils/utils.py:169-187): trunc(clamp(255 y, 0, 255)) of a float [N, 3, H, W] batch -> uint8 [N, H, W, 3]."""
    return (sr * 255.0).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def degraded_tiles(generator, scale, hr_u8, mode='sr'):
    """One of the script's rows for a batch of HR tiles (uint8 [N, H, W, 3] on the device, H and W multiples of scale):
    'sr' = generator(bicubic-down LR) quantised like save_img1, 'bicubic' = the LR tile bicubic-up, 'lr' = the bare LR tile."""
    _require_u8(hr_u8, 'degraded_tiles')
    if mode not in ('sr', 'bicubic', 'lr'):
        raise ValueError("mode must be 'sr', 'bicubic' or 'lr', got %r" % (mode,))
    n, h, w, _ = hr_u8.shape
    if h % scale or w % scale:
        raise ValueError('HR tile %dx%d is not a multiple of scale %d' % (h, w, scale))
    lr = sdata.resize_u8(hr_u8, h // scale, w // scale, 'bicubic')
    if mode == 'lr':
        return lr
    if mode == 'bicubic':
        return sdata.resize_u8(lr, h, w, 'bicubic')
    was_training = generator.training
    generator.eval()
    try:
        with torch.no_grad():
            sr = generator(sdata.to_tensor(lr))
    finally:
        generator.train(was_training)
    return quantise(sr)


def features_of(u8, vgg, means, hw=None):
    """uint8 tiles -> flattened VGG19 bottleneck features [N, h * w * 512], (h, w, c) order."""
    if hw is not None:
        u8 = _conform(u8, hw)
    f = vgg(preprocess(u8, means))
    return f.reshape(f.shape[0], -1)


def _input_hw(head):
    if len(head.feature_shape) != 3:
        raise ValueError('the head must have been built for [h, w, 512] features')
    return head.feature_shape[0] * 32, head.feature_shape[1] * 32


def classify_sr(generator, scale, hr_u8_batches, labels, vgg, head, means, mode='sr', return_tiles=False):
    """The script's evaluate() for one (model, scale) row, on the device: every HR batch is degraded (`degraded_tiles`), the
    uint8 tiles go through preprocess, VGG19 and the head.  labels: one integer per tile over all batches.  Returns the head's
    evaluate() dict (with return_tiles also 'tiles': the uint8 batches that reached the classifier)."""
    batches = [hr_u8_batches] if torch.is_tensor(hr_u8_batches) else list(hr_u8_batches)
    hw = _input_hw(head)
    tiles = [degraded_tiles(generator, scale, b.to(head.device), mode) for b in batches]
    feats = torch.cat([features_of(t, vgg, means, hw) for t in tiles])
    out = head.evaluate(feats, labels)
    if return_tiles:
        out['tiles'] = tiles
    return out


def classify_folder(root, vgg, head, means, batch_size=64, class_names=None):
    """evaluate(dataset, dirpath, ...) on a directory of class folders, as flow_from_directory reads it: classes are the sorted
    sub-directory names (or `class_names`), every image is loaded as RGB and, where its size differs from the head's input size,
    resized with PIL nearest."""
    from PIL import Image
    names = sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d))) if class_names is None else list(class_names)
    hw = _input_hw(head)
    files, labels = [], []
    for k, name in enumerate(names):
        for fn in sorted(os.listdir(os.path.join(root, name))):
            if sdata.is_image_file(fn):
                files.append(os.path.join(root, name, fn))
                labels.append(k)
    if not files:
        raise ValueError('classify_folder: no image files under %s' % root)
    feats = []
    for a in range(0, len(files), batch_size):
        imgs = []
        for fn in files[a:a + batch_size]:
            with Image.open(fn) as im:
                im = im.convert('RGB')
                if (im.height, im.width) != hw:
                    im = im.resize((hw[1], hw[0]), Image.NEAREST)
                imgs.append(np.asarray(im, dtype=np.uint8))
        feats.append(features_of(torch.from_numpy(np.stack(imgs)).to(head.device), vgg, means))
    out = head.evaluate(torch.cat(feats), labels)
    out['class_names'] = names
    return out
