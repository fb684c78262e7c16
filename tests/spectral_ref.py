"""Plain-torch restatement (stock CPU / ATen ops, no kernels) of the reference's SpectralNorm wrapper (base_networks.py:73-131) and of
its patch discriminator built with use_spectralnorm=True (:1747-1805), with the reference's state_dict keys; the deterministic filling,
the inputs and the sequence of passes tools/make_golden_spectral.py records tests/golden/disc_spectral.npz with.
tests/test_spectral_cpu.py holds this file to the recorded numbers; the GPU tests and tools/time_spectral.py then use it where the
reference itself cannot travel.  Reuses tests/disc_norms_ref.py (GroupNorm, the inputs, the digests) and tests/gan_options_ref.py."""
import numpy as np
import torch
import torch.nn as nn
from torch.nn import Parameter

from oracle import sradsgan_ref as O
from tests import disc_norms_ref as DR

NORM_TYPES = ('', 'instance', 'group', 'batch')
VARIANTS = [(nt, att) for nt in NORM_TYPES for att in (False, True)]                    # keys and shapes: all 8
NUMBERED = [('', False), ('', True), ('instance', False), ('batch', False)]             # numbers: these four
IMG_SHAPE = DR.IMG_SHAPE
TRAIN_CASES = {'plain': dict(relative=False), 'relative': dict(relative=True)}          # one iteration each, '' + attention
N_PASSES = 4
tag = DR.tag


EPS = 1e-12


def l2normalize(x):
    """x scaled to unit length, the length taken with EPS added."""
    return x / (x.norm() + EPS)


class SpectralNorm(nn.Module):
    """A conv whose weight is divided by an estimate of its largest singular value.  The conv's `weight` is replaced by three
    parameters: `weight_bar` (the weight itself), `weight_u` [Cout] and `weight_v` [Cin kh kw] (unit vectors, no gradient).  Every
    forward advances u and v by one power iteration in place, takes sigma = u . (Wm v) with Wm = weight_bar as a [Cout, K] matrix and
    convolves with weight_bar / sigma; sigma is differentiated through weight_bar only.  `operand` (tools only) rounds the conv's two
    operands in the forward."""

    def __init__(self, module, name='weight', power_iterations=1):
        super().__init__()
        self.module, self.name, self.power_iterations = module, name, power_iterations
        self.operand = None
        weight = module._parameters.pop(name)
        rows, cols = weight.shape[0], weight[0].numel()
        fresh = {'_u': l2normalize(torch.randn(rows, dtype=weight.dtype)), '_v': l2normalize(torch.randn(cols, dtype=weight.dtype)),
                 '_bar': weight.data}
        for suffix in ('_u', '_v', '_bar'):
            module.register_parameter(name + suffix, Parameter(fresh[suffix], requires_grad=suffix == '_bar'))

    def forward(self, x):
        conv = self.module
        u, v, w_bar = conv.weight_u, conv.weight_v, conv.weight_bar
        with torch.no_grad():                       # the vectors are constants of the graph; a later pass must not disturb this one's
            wm, u_now, v_now = w_bar.flatten(1), u, v
            for _ in range(self.power_iterations):
                v_now = l2normalize(wm.t() @ u_now)
                u_now = l2normalize(wm @ v_now)
            v.copy_(v_now), u.copy_(u_now)
        sigma = torch.dot(u_now, w_bar.flatten(1) @ v_now)
        weight = w_bar / sigma
        if self.operand is not None:
            weight, x = self.operand(weight), self.operand(x)
        return nn.functional.conv2d(x, weight, conv.bias, conv.stride, conv.padding)


class Discriminator(nn.Module):
    _PLAN = DR.Discriminator._PLAN

    def __init__(self, in_channels=3, norm_type='', use_spectralnorm=True, attention=False):
        super().__init__()
        assert use_spectralnorm and norm_type in NORM_TYPES
        layers, cin = [], in_channels
        for idx, (cout, stride, norm) in enumerate(self._PLAN, start=1):
            layers.append(SpectralNorm(nn.Conv2d(cin, cout, 3, stride, 1)))
            if norm and norm_type:
                layers.append({'batch': nn.BatchNorm2d, 'instance': nn.InstanceNorm2d, 'group': DR.GroupNorm}[norm_type](cout))
            layers.append(nn.LeakyReLU(0.2))
            if attention and idx == 6:
                layers += [O.ChannelAttention(256), O.SpatialAttention()]
            cin = cout
        layers.append(nn.Conv2d(cin, 1, 3, 1, 1))
        self.model = nn.Sequential(*layers)

    def forward(self, img):
        return self.model(img)


def wrappers(d):
    """The spectral wrappers of a discriminator (the reference's, this file's or the HIP one's), in layer order."""
    return [m for m in d.modules() if m.__class__.__name__ == 'SpectralNorm']


def fill_(d, suffix=0, conv_scale=1.0):
    """oracle det_init_ by state_dict key (weight_bar like any conv weight, biases, BatchNorm), group-norm weights and biases as
    disc_norms_ref.fill_ fills them, weight_u / weight_v = l2normalize of U(-1, 1) by key, then weight_bar and the last conv's weight
    times conv_scale (W = weight_bar / sigma does not see the factor; the plain last conv does)."""
    pre = DR.prefix(suffix)
    O.det_init_(d, prefix=pre)
    with torch.no_grad():
        for name, m in d.named_modules():
            if m.__class__.__name__ == 'GroupNorm':
                m.weight.copy_(O.det_fill(pre + name + '.weight', tuple(m.weight.shape), 0.05, 1.0))
                m.bias.copy_(O.det_fill(pre + name + '.bias', tuple(m.bias.shape), 0.05, 0.0))
        for key, p in d.named_parameters():
            if key.endswith(('weight_u', 'weight_v')):
                p.copy_(l2normalize(O.det_fill(pre + key, tuple(p.shape), 1.0).to(p.dtype)))
            elif key.endswith('weight_bar') or (p.dim() == 4 and tuple(p.shape[2:]) == (3, 3) and p.shape[0] == 1):
                p.mul_(conv_scale)
    return d


def inputs(suffix=0):
    return DR.inputs(suffix)


def uv_digest(t, nsample=16):
    """Up to `nsample` evenly strided entries (entries of unit vectors: no sums, whose rounding grows with the length)."""
    a = t.detach().cpu().double().numpy().ravel()
    return a[::max(1, a.size // nsample)][:nsample]


def sigma_of(sn):
    """sigma as the pass that has just run computed it: u . (weight_bar v) with the updated u and v."""
    m = sn.module
    w = m.weight_bar.detach()
    return float(m.weight_u.detach().dot(w.view(w.shape[0], -1).mv(m.weight_v.detach())))


def state_after_pass(d):
    """(u digests, v digests, sigmas) of every wrapper, concatenated in layer order."""
    ws = wrappers(d)
    return (np.concatenate([uv_digest(w.module.weight_u) for w in ws]), np.concatenate([uv_digest(w.module.weight_v) for w in ws]),
            np.array([sigma_of(w) for w in ws], dtype=np.float64))


def trainable(d):
    return {k: p for k, p in d.named_parameters() if p.requires_grad}


def run(d, t, alpha, penalty, after_pass=state_after_pass):
    """The recorded sequence of N_PASSES passes of one discriminator from its filled state:
      1  y = D(img), backward with the cotangent dy               -> y, d img, the trainable parameters' gradients
      2  the gradient penalty on (real, fake, alpha)               -> its value and parameter gradients
      3  D(real) under no_grad        4  D(fake) under no_grad, eval mode
    and after each pass (u, v, sigma) of every layer.  penalty(d, real, fake, alpha) returns the penalty after having backpropagated
    it (the reference's method does so)."""
    dt = next(d.parameters()).dtype
    img = t['img'].to(dt).clone().requires_grad_(True)
    d.zero_grad()
    states = []
    y = d(img)
    states.append(after_pass(d))
    y.backward(t['dy'].to(dt))
    out = dict(y=y.detach().clone(), dx=img.grad.clone(), grads={k: p.grad.clone() for k, p in trainable(d).items()})
    d.zero_grad()
    gp = penalty(d, t['real'].to(dt), t['fake'].to(dt), alpha)
    states.append(after_pass(d))
    out['gp'] = float(gp)
    out['gp_grads'] = {k: (p.grad.clone() if p.grad is not None else torch.zeros_like(p)) for k, p in trainable(d).items()}
    d.zero_grad()
    with torch.no_grad():
        d(t['real'].to(dt))
        states.append(after_pass(d))
        was = d.training
        d.eval()
        d(t['fake'].to(dt))
        d.train(was)
        states.append(after_pass(d))
    out['states'] = states
    return out


restated_penalty = DR.restated_penalty


def clamp_uv(d, clip=0.01):
    """(u digests, v digests) as the step leaves them: every D parameter clamped to +- clip_value (sradsgan.py:891-892)."""
    ws = wrappers(d)
    return (np.concatenate([uv_digest(w.module.weight_u.detach().clamp(-clip, clip)) for w in ws]),
            np.concatenate([uv_digest(w.module.weight_v.detach().clamp(-clip, clip)) for w in ws]))
