"""Plain-torch restatement (stock CPU / ATen ops, no kernels) of the reference's patch discriminator with its choice of
normalisation (base_networks.py:1747-1805) and of its GroupNorm (:12-31), with the reference's state_dict keys; the deterministic
filling and the inputs that tools/make_golden_disc_norms.py records tests/golden/disc_norms.npz with; and the gradient penalty on
it (oracle.sradsgan_ref.gradient_penalty).  tests/test_disc_norms_cpu.py holds this file to the recorded numbers; the GPU tests and
tools/time_d_norms.py then use it where the reference itself cannot travel."""
import torch
import torch.nn as nn

from oracle import sradsgan_ref as O

NORM_TYPES = ('', 'instance', 'group')
VARIANTS = [(nt, att) for nt in NORM_TYPES for att in (False, True)]
IMG_SHAPE = (2, 3, 32, 32)        # the smallest input with a 2 x 2 map in block 8


def tag(norm_type, attention):
    return '%s_%s' % (norm_type or 'none', 'att' if attention else 'plain')


class GroupNorm(nn.Module):
    """Groups of adjacent channels, the unbiased variance, eps inside the root, weight / bias of shape (1, C, 1, 1)."""

    def __init__(self, num_features, num_groups=32, eps=1e-5):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(1, num_features, 1, 1))
        self.bias = nn.Parameter(torch.zeros(1, num_features, 1, 1))
        self.num_groups, self.eps = num_groups, eps

    def forward(self, x):
        n, c, h, w = x.shape
        g = x.reshape(n, self.num_groups, -1)
        g = (g - g.mean(-1, keepdim=True)) / torch.sqrt(g.var(-1, unbiased=True, keepdim=True) + self.eps)
        return g.reshape(n, c, h, w) * self.weight + self.bias


class Discriminator(nn.Module):
    _PLAN = [(64, 1, False), (64, 2, True), (128, 1, True), (128, 2, True), (256, 1, True), (256, 2, True), (512, 1, True), (512, 2, True)]

    def __init__(self, in_channels=3, norm_type='', use_spectralnorm=False, attention=False):
        super().__init__()
        assert not use_spectralnorm and norm_type in NORM_TYPES + ('batch',)
        layers, cin = [], in_channels
        for idx, (cout, stride, norm) in enumerate(self._PLAN, start=1):
            layers.append(nn.Conv2d(cin, cout, 3, stride, 1))
            if norm and norm_type:
                layers.append({'batch': nn.BatchNorm2d, 'instance': nn.InstanceNorm2d, 'group': GroupNorm}[norm_type](cout))
            layers.append(nn.LeakyReLU(0.2))
            if attention and idx == 6:
                layers += [O.ChannelAttention(256), O.SpatialAttention()]
            cin = cout
        layers.append(nn.Conv2d(cin, 1, 3, 1, 1))
        self.model = nn.Sequential(*layers)

    def forward(self, img):
        return self.model(img)


def prefix(suffix):
    """The filler tag of a fixture: 'D.' for suffix 0, 'D<suffix>.' otherwise (the fixture records which suffix it was made with)."""
    return 'D.' if suffix == 0 else 'D%d.' % suffix


def fill_(d, suffix, conv_scale):
    """oracle det_init_ by state_dict key; group-norm weights around 1 and biases around 0 like the BatchNorm ones (det_init_ knows
    nn.BatchNorm2d only); then every 3 x 3 conv weight times conv_scale (the fixture's signal factor)."""
    pre = prefix(suffix)
    O.det_init_(d, prefix=pre)
    with torch.no_grad():
        for name, m in d.named_modules():
            if m.__class__.__name__ == 'GroupNorm':
                m.weight.copy_(O.det_fill(pre + name + '.weight', tuple(m.weight.shape), 0.05, 1.0))
                m.bias.copy_(O.det_fill(pre + name + '.bias', tuple(m.bias.shape), 0.05, 0.0))
            elif isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3):
                m.weight.mul_(conv_scale)
    return d


def inputs(suffix):
    """img, the cotangent of D(img), and the penalty's real / fake pair."""
    s = '' if suffix == 0 else '.%d' % suffix
    return dict(img=O.det_fill('dimg' + s, IMG_SHAPE, 0.5, 0.5), dy=O.det_fill('D.dy' + s, (IMG_SHAPE[0], 1, 2, 2), 1.0),
                real=O.det_fill('gp.real' + s, IMG_SHAPE, 0.5, 0.5), fake=O.det_fill('gp.fake' + s, IMG_SHAPE, 0.5, 0.5))


def digest(t):
    return O.digest(t, full_max=16, nsample=8)


def run(d, t, alpha, penalty):
    """What the fixture records of one discriminator: y, dx, the parameter gradients of <dy, D(img)>, the penalty and its parameter
    gradients.  penalty(d, real, fake, alpha) returns the penalty after having backpropagated it (the reference's method does so)."""
    dt = next(d.parameters()).dtype
    img = t['img'].to(dt).clone().requires_grad_(True)
    d.zero_grad()
    y = d(img)
    y.backward(t['dy'].to(dt))
    out = dict(y=y.detach().clone(), dx=img.grad.clone(), grads={k: p.grad.clone() for k, p in d.named_parameters()})
    d.zero_grad()
    gp = penalty(d, t['real'].to(dt), t['fake'].to(dt), alpha)
    out['gp'] = float(gp)
    out['gp_grads'] = {k: (p.grad.clone() if p.grad is not None else torch.zeros_like(p)) for k, p in d.named_parameters()}
    d.zero_grad()
    return out


def restated_penalty(d, real, fake, alpha):
    return O.gradient_penalty(d, real, fake, alpha.to(real.dtype), 'L2', 'LS').detach()      # (it backpropagates the penalty itself)
