"""LPIPS on the device: the reference's `PerceptualLoss(model='net-lin', net='alex')` (sradsgan.py:561; utils/PerceptualSimilarity/
__init__.py:13-40, networks_basic.py:27-115, pretrained_networks.py:57-96, weights v0.1): the metric (`forward`, `pairs`, under no_grad) and
the same distance as a training loss (`loss`, one autograd node with its own backward kernels).

Structure here, weights from the user -- the precedent of FeatureExtractor.load_torchvision_vgg19: the pretrained AlexNet file is
torchvision's to download, so `load_torchvision_alexnet` takes its state dict (`features.{0,3,6,8,10}.{weight,bias}`); the five learned
linear heads come from the reference's own `weights/v0.1/alex.pth` through `load_lin` (`lin{0..4}.model.1.weight`).  Until both are
loaded the module holds a deterministic init and its numbers mean nothing.

The arithmetic (csrc/lpips.hip): scaling layer + conv1 + ReLU in one exact-fp32 pass, 3x3 stride-2 max pools, convs 2-5 through the
ordinary conv kernels with the bias + ReLU epilogue, then per tap one head pass (channel normalisation, squared difference, the lin
weights, pixel sums in float64) and one finish launch.  Features are computed once per image and compared through an index-pair list,
so validation runs the backbone once over [SR; HR; bicubic]."""
import math

import torch
import torch.nn as nn

from . import _hip, ops

# torchvision.models.alexnet().features: index -> (cin, cout, k, stride, pad); ReLU follows each conv, MaxPool2d(3, 2) sits at 2 and 5
_CONVS = {0: (3, 64, 11, 4, 2), 3: (64, 192, 5, 1, 2), 6: (192, 384, 3, 1, 1), 8: (384, 256, 3, 1, 1), 10: (256, 256, 3, 1, 1)}
CHANNELS = (64, 192, 384, 256, 256)                  # networks_basic.py:44
MIN_SIDE = 31                                        # the smallest side for which the second pool still has an output


class _Conv(nn.Module):
    """Parameter holder with nn.Conv2d's names (weight OIHW, bias)."""

    def __init__(self, cin, cout, k, bias=True):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin, k, k), requires_grad=False)
        self.bias = nn.Parameter(torch.empty(cout), requires_grad=False) if bias else None


class _Lin(nn.Module):
    """NetLinLayer (networks_basic.py:108-115): `model` = [Dropout, 1x1 conv without bias]; dropout is the identity in eval."""

    def __init__(self, c):
        super().__init__()
        self.model = nn.Sequential(nn.Identity(), _Conv(c, 1, 1, bias=False))


def tap_sizes(h, w):
    """(h, w) of the five taps for an H x W image."""
    h0, w0 = (h + 4 - 11) // 4 + 1, (w + 4 - 11) // 4 + 1
    h1, w1 = (h0 - 3) // 2 + 1, (w0 - 3) // 2 + 1
    h2, w2 = (h1 - 3) // 2 + 1, (w1 - 3) // 2 + 1
    return [(h0, w0), (h1, w1), (h2, w2), (h2, w2), (h2, w2)]


class _Loss(torch.autograd.Function):
    """LPIPS.loss as one autograd node: the batch mean of the distances, differentiable in pred alone.  The forward is `pairs` over the
    stacked [target; pred] batch with the taps kept; the backward walks the backbone down again (see LPIPS.loss)."""

    @staticmethod
    def forward(ctx, pred, target, model, normalize, mode):
        n = pred.shape[0]
        with ops.conv_math(mode):
            taps = model.feature_taps([target, pred], normalize)
            dist = model._distances(taps, [(i, n + i) for i in range(n)])
        ctx.model, ctx.normalize, ctx.mode, ctx.taps, ctx.image_hw = model, normalize, mode, taps, tuple(pred.shape[2:])
        return dist.mean().to(torch.float32)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        model, taps = ctx.model, ctx.taps
        n = taps[0].shape[0] // 2
        pt = model._pairs_tensor([(i, n + i) for i in range(n)], 2 * n, taps[0].device)
        grad = grad.detach().to(torch.float32).contiguous()
        conv = lambda i: model.features[i].weight
        with ops.conv_math(ctx.mode):
            # each head gradient arrives through its tap's ReLU; the conv chain adds it after masking its own gradient with the same tap
            hg = [ops.lpips_head_bwd_raw(f, pt, model.lin(k), grad, n * f.shape[2] * f.shape[3]) for k, f in enumerate(taps)]
            tp = [f[n:] for f in taps]
            g = ops.conv2d_dgrad_raw(hg[4], conv(10), tuple(tp[3].shape), 1, 1, residual=hg[3], actmask=tp[3])
            g = ops.conv2d_dgrad_raw(g, conv(8), tuple(tp[2].shape), 1, 1, residual=hg[2], actmask=tp[2])
            g = ops.conv2d_dgrad_raw(g, conv(6), (n, CHANNELS[1]) + tuple(tp[2].shape[2:]), 1, 1)
            g = ops.max_pool3x3s2_bwd_raw(tp[1], g, relu=True, residual=hg[1])
            h1, w1 = (tp[0].shape[2] - 3) // 2 + 1, (tp[0].shape[3] - 3) // 2 + 1
            g = ops.conv2d_dgrad_raw(g, conv(3), (n, CHANNELS[0], h1, w1), 1, 2)
            g = ops.max_pool3x3s2_bwd_raw(tp[0], g, relu=True, residual=hg[0])
            dx = ops.lpips_stem_bwd_raw(g, model._stem_weight(), ctx.image_hw, ctx.normalize)
        return dx, None, None, None, None


class LPIPS(nn.Module):
    def __init__(self):
        super().__init__()
        self.features = nn.Sequential(*[_Conv(*_CONVS[i][:3]) if i in _CONVS else nn.Identity() for i in range(12)])
        for k, c in enumerate(CHANNELS):
            setattr(self, 'lin%d' % k, _Lin(c))
        g = torch.Generator().manual_seed(0)                       # deterministic init; real use loads both state dicts
        with torch.no_grad():
            for i, (cin, _, k, _, _) in _CONVS.items():
                bound = math.sqrt(6.0 / (cin * k * k))
                self.features[i].weight.copy_((torch.rand(self.features[i].weight.shape, generator=g) * 2 - 1) * bound)
                self.features[i].bias.zero_()
            for k, c in enumerate(CHANNELS):
                self.lin(k).fill_(1.0 / c)
        ops.mark_static(self)
        self._pair_lists = {}
        self.eval()

    def lin(self, k):
        return getattr(self, 'lin%d' % k).model[1].weight

    # ------------------------------------------------------------------ weights ---------------- #
    def _load(self, named, what):
        for name, (param, value) in named.items():
            if tuple(value.shape) != tuple(param.shape):
                raise ValueError('%s: %s has shape %s, expected %s' % (what, name, tuple(value.shape), tuple(param.shape)))
        with torch.no_grad():
            for param, value in named.values():
                param.copy_(value)                                 # bumps the version: packed images are rebuilt on next use
        return sorted(named)

    def load_torchvision_alexnet(self, state_dict):
        """torchvision AlexNet state dict: `features.{0,3,6,8,10}.{weight,bias}` are taken, every other key is ignored."""
        named = {}
        for i in _CONVS:
            for leaf in ('weight', 'bias'):
                key = 'features.%d.%s' % (i, leaf)
                if key not in state_dict:
                    raise KeyError('load_torchvision_alexnet: %s is missing' % key)
                named[key] = (getattr(self.features[i], leaf), state_dict[key])
        return self._load(named, 'load_torchvision_alexnet')

    def load_lin(self, state_dict):
        """The reference's weights/v0.1/alex.pth: `lin{0..4}.model.1.weight` [1, C, 1, 1]."""
        named = {}
        for k in range(len(CHANNELS)):
            key = 'lin%d.model.1.weight' % k
            if key not in state_dict:
                raise KeyError('load_lin: %s is missing' % key)
            named[key] = (self.lin(k), state_dict[key])
        return self._load(named, 'load_lin')

    def _stem_weight(self):
        # [ky][kx][ci][co], kept on the parameter beside its packed images: ops.weights_changed refreshes it with them
        return ops.derived_weight(self.features[0].weight, 'hwio', lambda w: w.detach().permute(2, 3, 1, 0).contiguous())

    def _pairs_tensor(self, index_pairs, m, device):
        key = (tuple(map(tuple, index_pairs)), str(device))
        t = self._pair_lists.get(key)
        if t is None:                       # built outside a capture (the warm-up pass), reused inside
            if not key[0] or any(len(p) != 2 or not (0 <= p[0] < m and 0 <= p[1] < m) for p in key[0]):
                raise ValueError('LPIPS.pairs: index pairs must be (i0, i1) with 0 <= i < %d' % m)
            t = self._pair_lists[key] = torch.tensor(key[0], dtype=torch.int32, device=device)
        elif max(max(p) for p in key[0]) >= m:
            raise ValueError('LPIPS.pairs: index out of range for %d images' % m)
        return t

    # ------------------------------------------------------------------ forward ---------------- #
    def feature_taps(self, images, normalize=True):
        """The five ReLU taps for a list of image batches (logically concatenated along N; the stem writes each batch into its slice of
        one tensor, so nothing is copied)."""
        images = [images] if torch.is_tensor(images) else list(images)
        for t in images:
            ops._require_gpu(t, 'LPIPS')
            if t.dim() != 4 or t.shape[1] != 3 or tuple(t.shape[2:]) != tuple(images[0].shape[2:]):
                raise ValueError('LPIPS: images must be [N, 3, H, W] of one size, got %s' % (tuple(t.shape),))
        h, w = images[0].shape[2:]
        if min(h, w) < MIN_SIDE:
            raise ValueError('LPIPS: images must be at least %d x %d (AlexNet\'s second pool), got %d x %d' % (MIN_SIDE, MIN_SIDE, h, w))
        m = sum(t.shape[0] for t in images)
        (h0, w0) = tap_sizes(h, w)[0]
        f = ops.empty_nhwc(m, 64, h0, w0, images[0])
        wk, at = self._stem_weight(), 0
        for t in images:
            ops.lpips_stem_raw(t.detach(), wk, self.features[0].bias, normalize, out=f[at:at + t.shape[0]])
            at += t.shape[0]
        taps = [f]
        for i in (3, 6, 8, 10):
            if i in (3, 6):
                f = ops.max_pool3x3s2_raw(f)
            conv = self.features[i]
            f = ops.conv2d_fwd_raw(f, conv.weight, conv.bias, _CONVS[i][3], _CONVS[i][4], slope=0.0)
            taps.append(f)
        return taps

    @torch.no_grad()
    def pairs(self, images, index_pairs, normalize=True):
        """images: a tensor [M,3,H,W] or a list of such batches (indices run over their concatenation); index_pairs: [(i0, i1), ...].
        Returns float64 [P]: the LPIPS distance of each pair.  Features are computed once per image."""
        if ops.get_conv_math() == 'half':                # a validation metric must not move with the training arithmetic
            with ops.conv_math('bf16x3'):
                return self.pairs(images, index_pairs, normalize)
        return self._distances(self.feature_taps(images, normalize), index_pairs)

    def _distances(self, taps, index_pairs):
        """The heads and the finish over computed taps -> float64 [P]."""
        dev = taps[0].device
        pt = self._pairs_tensor(index_pairs, taps[0].shape[0], dev)
        partial = torch.empty(len(taps), pt.shape[0], _hip.lib().srhip_lpips_blocks(), device=dev, dtype=torch.float64)
        for k, f in enumerate(taps):
            ops.lpips_head_raw(f, pt, self.lin(k), partial[k])
        return ops.lpips_finish_raw(partial, [f.shape[2] * f.shape[3] for f in taps])

    def loss(self, pred, target, normalize=True):
        """The batch mean of forward(pred, target) as a 0-d float32 tensor that trains: one autograd node whose gradient goes to pred
        alone (the reference's PerceptualLoss is an ordinary differentiable module; here `pairs` stays a no_grad metric and this is the
        loss).  Backward: the head backward of every tap, conv2d_dgrad down convs 10, 8, 6 and 3 with each tap's ReLU mask and head
        gradient fused in, the two pool backwards, the stem backward.  A pred pixel whose features are all zero at a tap receives a zero
        gradient from that tap where torch autograd would produce NaN (the root of a zero norm).  Conv arithmetic follows ops.conv_math,
        'half' mapped to 'bf16x3' as in `pairs`; the mode of the forward is the mode of the backward.  Under no_grad, or for a pred
        that does not require grad, this is the forward alone."""
        if target.requires_grad:
            raise ValueError('LPIPS.loss: the gradient goes to pred only; detach the target')
        ops._require_gpu(pred, 'LPIPS.loss')
        ops._require_gpu(target, 'LPIPS.loss')
        if pred.shape != target.shape:
            raise ValueError('LPIPS: shape mismatch %s vs %s' % (tuple(pred.shape), tuple(target.shape)))
        mode = ops.get_conv_math()
        mode = 'bf16x3' if mode == 'half' else mode
        if not (torch.is_grad_enabled() and pred.requires_grad):
            with ops.conv_math(mode), torch.no_grad():
                return self.forward(pred, target, normalize).mean().to(torch.float32)
        return _Loss.apply(pred, target, self, normalize, mode)

    def forward(self, pred, target, normalize=True):
        """PerceptualLoss.forward (__init__.py:26-40): pred, target [N,3,H,W], in [0,1] when normalize else in [-1,1] -> float64 [N]."""
        ops._require_gpu(pred, 'LPIPS')
        ops._require_gpu(target, 'LPIPS')
        if pred.shape != target.shape:
            raise ValueError('LPIPS: shape mismatch %s vs %s' % (tuple(pred.shape), tuple(target.shape)))
        n = pred.shape[0]
        return self.pairs([target, pred], [(i, n + i) for i in range(n)], normalize)
