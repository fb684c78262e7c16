"""Spectral normalisation on the HIP path: the reference's SpectralNorm wrapper (base_networks.py:73-131) and its patch discriminator
built with use_spectralnorm=True (base_networks.py:1747-1805), with the reference's class name, constructor arguments and state_dict
keys -- per wrapped conv, in this order: `module.bias`, `module.weight_u` [Cout], `module.weight_v` [Cin kh kw], `module.weight_bar`
[Cout, Cin, kh, kw], all four Parameters, u and v with requires_grad=False.

What the wrapper does on EVERY forward (train, eval and no_grad alike), with Wb = weight_bar viewed as [Cout, K]:
    v <- l2normalize(Wb^T u);  u <- l2normalize(Wb v);  sigma = u . (Wb v);  conv with W = weight_bar / sigma
u and v are overwritten in place, so the weights of two passes of one training step differ: D(fake) of the discriminator phase is NOT
D(gen_hr) of the generator phase.  TrainStep therefore runs a spectral discriminator on its plain order -- every pass of the reference,
in the reference's sequence -- whatever `reuse_d_fake` says.  The gradient treats u and v as constants and sigma as a function of
weight_bar (ops._SpectralWeights); each pass keeps its own (u, v, sigma).  Only power_iterations = 1 is reachable in the reference.

SpectralPatchDiscriminator is its own class because PatchDiscriminator(use_spectralnorm=True) keeps refusing (the one-walk step rests
on the equality above).  It runs ONE batched call (csrc/sn.hip: 4 launches) for the 8 wrapped convs per forward; a SpectralNorm used
on its own runs the same call for its one layer.  The final 512 -> 1 conv is a plain conv, as in the reference.

Departure from the reference, initialisation: `discriminator.apply(weights_init_normal)` raises AttributeError there for a spectral
discriminator (the wrapped conv has no `weight` before its first forward, and 'SpectralNorm' matches the initialiser's 'Norm' branch),
so the reference's own trainer never initialised one.  spectral_init_ gives weight_bar ~ N(0, 0.02) and bias = 0 -- what the
initialiser gives every other conv -- and leaves u and v as constructed (normal, then l2normalize)."""
import torch
import torch.nn as nn
from torch.nn import Parameter

from .. import ops
from .base_networks import ChannelAttention, SpatialAttention
from .discriminators import _NORMS, NORM_TYPES
from .layers import HipConv2d


def _unit(x):
    return x / (x.norm() + 1e-12)


def _same_layers(table, layers):
    """False once the module holds other Parameter objects than the table was built from (load_state_dict(assign=True) replaces them):
    the table would go on reading the ones that have left."""
    return len(table.layers) == len(layers) and all(a is b for old, new in zip(table.layers, layers) for a, b in zip(old, new))


class SpectralNorm(nn.Module):
    def __init__(self, module, name='weight', power_iterations=1):
        super().__init__()
        if not isinstance(module, HipConv2d):
            raise NotImplementedError('SpectralNorm wraps a HipConv2d (the reference wraps nn.Conv2d only), got %s' % type(module).__name__)
        if name != 'weight':
            raise NotImplementedError("SpectralNorm: name must be 'weight'")
        if power_iterations != 1:
            raise NotImplementedError('SpectralNorm: power_iterations = 1 only (the reference never passes another value)')
        self.module, self.name, self.power_iterations = module, name, power_iterations
        # the conv's weight leaves its parameter list; u [Cout], v [K] (unit vectors, no gradient) and the weight itself as
        # weight_bar take its place, registered in the order of the reference's keys
        weight = module._parameters.pop(name)
        rows, cols = weight.shape[0], weight[0].numel()
        fresh = {'_u': _unit(torch.randn(rows, dtype=weight.dtype, device=weight.device)),
                 '_v': _unit(torch.randn(cols, dtype=weight.dtype, device=weight.device)), '_bar': weight.data}
        for suffix in ('_u', '_v', '_bar'):
            module.register_parameter(name + suffix, Parameter(fresh[suffix], requires_grad=suffix == '_bar'))
        self._table = None                       # a one-layer ops.SpectralTable, built when the wrapper is called on its own

    def layer(self):
        """(weight_bar, weight_u, weight_v): this wrapper's row of an ops.SpectralTable."""
        m = self.module
        return getattr(m, self.name + '_bar'), getattr(m, self.name + '_u'), getattr(m, self.name + '_v')

    def forward(self, x, act_slope=None, residual=None, weight=None):
        """weight: this pass's effective weight when the owner has already run the batched call for all its wrappers."""
        if weight is None:
            if self._table is None or not _same_layers(self._table, [self.layer()]):
                self._table = ops.SpectralTable([self.layer()])
            weight, = ops.spectral_weights(self._table)
        m = self.module
        return ops.conv2d(x, weight, m.bias, m.stride[0], m.padding[0], act_slope, residual)


def spectral_init_(net, std=0.02):
    """weights_init_normal for a network with SpectralNorm wrappers (module docstring): wrapped convs get weight_bar ~ N(0, std),
    bias = 0, u and v untouched; every other module is initialised as trainer.weights_init_normal initialises it."""
    from ..trainer import weights_init_normal
    wrapped = {id(m.module) for m in net.modules() if isinstance(m, SpectralNorm)}
    for m in net.modules():
        if isinstance(m, SpectralNorm):
            with torch.no_grad():                # on the parameters, not `.data`: the write must move their version
                m.module.weight_bar.normal_(0.0, std)
                if m.module.bias is not None:
                    m.module.bias.zero_()
        elif id(m) not in wrapped:
            weights_init_normal(m)
    return net


class SpectralPatchDiscriminator(nn.Module):
    """base_networks.Discriminator(in_channels, norm_type, use_spectralnorm=True, attention): the 8 block convs wrapped, norm and
    attention slots as in PatchDiscriminator (block 1 never has a norm; 'batch' is the train-mode HipBatchNorm2d)."""
    _PLAN = [(64, 1, False), (64, 2, True), (128, 1, True), (128, 2, True), (256, 1, True), (256, 2, True), (512, 1, True), (512, 2, True)]
    use_spectralnorm = True

    def __init__(self, in_channels=3, norm_type='', attention=False):
        super().__init__()
        if norm_type not in NORM_TYPES:
            raise ValueError('SpectralPatchDiscriminator: norm_type must be one of %r, got %r' % (NORM_TYPES, norm_type))
        self.norm_type, self.attention = norm_type, attention
        layers, cin = [], in_channels
        self._blocks = []                        # (conv idx, norm idx or None, [attention idxs])
        for idx, (cout, stride, norm) in enumerate(self._PLAN, start=1):
            entry = [len(layers), None, []]
            layers.append(SpectralNorm(HipConv2d(cin, cout, 3, stride, 1)))
            if norm and norm_type:
                entry[1] = len(layers)
                layers.append(_NORMS[norm_type](cout))
            layers.append(nn.Identity())         # slot of LeakyReLU(0.2): fused into the conv / the norm
            if attention and idx == 6:
                entry[2] = [len(layers), len(layers) + 1]
                layers += [ChannelAttention(256), SpatialAttention()]
            self._blocks.append(tuple(entry))
            cin = cout
        layers.append(HipConv2d(cin, 1, 3, 1, 1))
        self.model = nn.Sequential(*layers)
        self._table = None

    def spectral_layers(self):
        return [self.model[conv_i] for conv_i, _, _ in self._blocks]

    def forward(self, img):
        layers = [sn.layer() for sn in self.spectral_layers()]
        if self._table is None or not _same_layers(self._table, layers):
            self._table = ops.SpectralTable(layers)
        weights = ops.spectral_weights(self._table)          # one power iteration of all 8 layers: u and v advance here
        x = ops.nhwc(img)
        m = self.model
        for (conv_i, norm_i, extra), w in zip(self._blocks, weights):
            if norm_i is None:
                x = m[conv_i](x, act_slope=0.2, weight=w)
            else:
                x = m[norm_i](m[conv_i](x, weight=w), act_slope=0.2)
            for e in extra:
                x = m[e](x)
        return m[len(m) - 1](x)


def has_spectral_layers(net):
    return any(isinstance(m, SpectralNorm) for m in net.modules())
