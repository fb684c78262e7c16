"""NDSRGAN on the same HIP kernels.  Mirrors SRADSGAN/model/ndsrgan.py:57-239 (CL, DenseBlock, DCRDB, DRRDBnet, GeneratorResNet,
Discriminator) with the reference's constructor signatures and state_dict keys (weight-tied `upsampling.{1,4,7}` stages), and one
iteration of its training loop (:414-456) as `train_step`.

Execution differs from the reference's graph, exactly in fp32:
  * a dense block keeps its input and its four CL outputs in ONE [n, h, w, 192] buffer: each CL reads a channel prefix of it and
    writes its 32 channels into its own slice (row strides of the conv ABI), so the 276 torch.cat calls of a forward never happen;
    conv1 writes its output into the first buffer, and conv2 reads its skip input from there;
  * DCRDB and DRRDBnet's sums `x + .2 o1 + .2 o2 + ...` are evaluated left to right in the reference, i.e. as running sums
    S_k = S_{k-1} + .2 m_k: one pass per block forms the block result and the running sum together and writes it straight into
    channels 0:64 of the next dense block's buffer (ops.dcrdb_step);
  * the upsampler's LeakyReLU is fused into its conv, nn.UpsamplingNearest2d is one HIP pass (ops.upsample_nearest)."""
import math

import torch
import torch.nn as nn

from .. import ops
from .layers import HipBatchNorm2d, HipConv2d
from .sradsgan import FeatureExtractor  # noqa: F401  (re-exported: ndsrgan.py:44-55 is the same vgg19.features[:12] slice)
from .srgan import weights_init_normal  # noqa: F401  (ndsrgan.py:36-42 is srgan.py's)

SLOPE = 0.2


def _check_widths(nf, nc):
    if nf != ops.DENSE_NF or nc != ops.DENSE_NC:
        raise NotImplementedError('NDSRGAN: the HIP dense blocks run nf = 64, nc = 32 (the reference\'s configuration), got nf = %d, '
                                  'nc = %d' % (nf, nc))


def CL(in_channels, out_channels):
    """ndsrgan.py:57: conv 3x3 + LeakyReLU(.2); slot 1 is the activation, fused into the conv."""
    return nn.Sequential(HipConv2d(in_channels, out_channels, 3, 1, 1), nn.Identity())


class DenseBlock(nn.Module):
    """ndsrgan.py:60-76: x + 0.2 * conv(cat(x, CL1, ..., CL4)), the concatenation held in one buffer (ops.dense_block)."""

    def __init__(self, nf, nc, CL_num=4):
        super().__init__()
        _check_widths(nf, nc)
        if CL_num != 4:
            raise NotImplementedError('DenseBlock: the HIP dense buffer holds four CLs (CL_num = 4)')
        self.CL_blocks = nn.Sequential(*[CL(nc * j + nf, nc) for j in range(CL_num)])
        self.conv = HipConv2d(nc * CL_num + nf, nf, 3, 1, 1)

    def tensors(self):
        out = []
        for cl in self.CL_blocks:
            out += [cl[0].weight, cl[0].bias]
        return out + [self.conv.weight, self.conv.bias]

    def forward(self, x):
        return ops.dense_block(ops.nhwc(x), self.tensors())


class DCRDB(nn.Module):
    """ndsrgan.py:78-92.  Called on its own it returns o4 * .2 + x; inside DRRDBnet the running sum x + .2 DCRDB(x) comes out of the
    same pass (forward_sum)."""

    def __init__(self, nf, nc):
        super().__init__()
        _check_widths(nf, nc)
        self.RDB1 = DenseBlock(nf, nc)
        self.RDB2 = DenseBlock(nf, nc)
        self.RDB3 = DenseBlock(nf, nc)
        self.conv = HipConv2d(nf, nf, 3, 1, 1)

    def tensors(self):
        return self.RDB1.tensors() + self.RDB2.tensors() + self.RDB3.tensors() + [self.conv.weight, self.conv.bias]

    def forward_sum(self, x, chain=False):
        """x + 0.2 * self(x) (one step of DRRDBnet's running sum)."""
        return ops.dcrdb_step(x, self.tensors(), chain)

    def forward(self, x):
        x = ops.nhwc(x)
        o1 = self.RDB1(x)
        t = x + 0.2 * o1
        o2 = self.RDB2(t)
        t = t + 0.2 * o2
        o3 = self.RDB3(t)
        t = t + 0.2 * o3
        return self.conv(t) * 0.2 + x


class DRRDBnet(nn.Module):
    """ndsrgan.py:94-158: 23 DCRDBs, block k on x + .2 m1 + ... + .2 m(k-1), the net returns that sum through m23."""

    def __init__(self, nf, nc):
        super().__init__()
        _check_widths(nf, nc)
        for k in range(1, 24):
            setattr(self, 'DRRDB%d' % k, DCRDB(nf, nc))

    def forward(self, x):
        s = x                                            # (a dense-buffer slice stays one: dcrdb_step adopts its buffer)
        for k in range(1, 24):
            s = getattr(self, 'DRRDB%d' % k).forward_sum(s, chain=k < 23)
        return s


class _UpsamplingNearest2d(nn.Module):
    """The Sequential slot of nn.UpsamplingNearest2d(scale_factor = r) (ndsrgan.py:175-181)."""

    def __init__(self, scale_factor):
        super().__init__()
        self.scale_factor = scale_factor

    def forward(self, x):
        return ops.upsample_nearest(x, self.scale_factor)


class GeneratorResNet(nn.Module):
    """ndsrgan.py:160-211.  The upsampler stage (nearest x r, conv, LeakyReLU) is ONE set of module objects repeated per stage, so
    x4 / x8 / x9 share one conv and state_dict lists it under every stage index, as in the reference."""

    def __init__(self, in_channels=3, out_channels=3, nf=64, nc=32, upscale_factor=3):
        super().__init__()
        _check_widths(nf, nc)
        self.conv1 = nn.Sequential(HipConv2d(in_channels, nf, 3, 1, 1))
        self.DCRDB_block = DRRDBnet(nf=nf, nc=nc)
        self.conv2 = HipConv2d(nf, nf, 3, 1, 1)
        two = [_UpsamplingNearest2d(2), HipConv2d(nf, nf, 3, 1, 1), nn.Identity()]
        three = [_UpsamplingNearest2d(3), HipConv2d(nf, nf, 3, 1, 1), nn.Identity()]
        upsampling = []
        if (upscale_factor & (upscale_factor - 1)) == 0:
            for _ in range(int(math.log(upscale_factor, 2))):
                upsampling += two
        elif upscale_factor % 3 == 0:
            for _ in range(int(math.log(upscale_factor, 3))):
                upsampling += three
        self.upsampling = nn.Sequential(*upsampling)
        self.conv3 = nn.Sequential(HipConv2d(nf, nf, 3, 1, 1), nn.Identity(), HipConv2d(nf, out_channels, 3, 1, 1))

    def forward(self, x):
        c1, c2 = self.conv1[0], self.conv2
        out = ops.conv2d_into_dense(ops.nhwc(x), c1.weight, c1.bias)        # written into channels 0:64 of DRRDB1's first buffer
        out = ops.conv2d_residual_strided(self.DCRDB_block(out), c2.weight, c2.bias, out)   # out + conv2(trunk), in conv2's epilogue
        up = self.upsampling
        for i in range(0, len(up), 3):
            out = up[i + 1](up[i](out), act_slope=SLOPE)
        return self.conv3[2](self.conv3[0](out, act_slope=SLOPE))


class Discriminator(nn.Module):
    """ndsrgan.py:213-239: PatchGAN of 4x4 convs (3 -> 64 s2, 64 -> 128 s2 + BN, 128 -> 256 s2 + BN, 256 -> 512 s1 + BN, each with
    LeakyReLU(.2) fused into the conv or the BN pass; 512 -> 1 s1).  Output [B, 1, H/8 - 2, W/8 - 2]."""

    def __init__(self, in_channels=3):
        super().__init__()
        layers, self._blocks, cin = [], [], in_channels
        for cout, stride, norm in [(64, 2, False), (128, 2, True), (256, 2, True), (512, 1, True)]:
            entry = (len(layers), len(layers) + 1 if norm else None)
            layers.append(HipConv2d(cin, cout, 4, stride, 1))
            if norm:
                layers.append(HipBatchNorm2d(cout))
            layers.append(nn.Identity())                 # slot of LeakyReLU(0.2): fused into conv / BN
            self._blocks.append(entry)
            cin = cout
        layers.append(HipConv2d(cin, 1, 4, 1, 1))
        self.model = nn.Sequential(*layers)

    def forward(self, img):
        x, m = ops.nhwc(img), self.model
        for conv_i, bn_i in self._blocks:
            x = m[conv_i](x, act_slope=SLOPE) if bn_i is None else m[bn_i](m[conv_i](x), act_slope=SLOPE)
        return m[len(m) - 1](x)


def train_step(G, D, Fx, opt_G, opt_D, lr_img, hr_img):
    """One iteration of ndsrgan.py:414-456: loss_G = 1e-2 SmoothL1(gen, hr) + SmoothL1(F(gen), F(hr)) + 2.5e-3 SmoothL1(D(gen), 1),
    Adam(G); loss_D = (SmoothL1(D(hr), 1) + SmoothL1(D(gen.detach()), 0)) / 2, Adam(D).  The valid / fake targets are scalars of the
    loss kernel.  D's weight gradients of loss_G, which the reference zeroes before the D step, are not computed.  Returns the
    two logged scalars and the loss terms as 0-d device tensors (no host sync)."""
    opt_G.zero_grad(set_to_none=True)
    gen_hr = G(lr_img)
    gen_validity = D(gen_hr)
    loss_gan = ops.smooth_l1_mean(gen_validity, 1.0)
    with torch.no_grad():
        real_features = Fx(hr_img)
    content = ops.smooth_l1_mean(Fx(gen_hr), real_features)
    pixel = ops.smooth_l1_mean(gen_hr, hr_img)
    loss_G = 1e-2 * pixel + content + 2.5e-3 * loss_gan
    with ops.backward_scope(skip_params=list(D.parameters())):
        loss_G.backward()
    opt_G.step()
    ops.bump_weight_epoch()
    opt_D.zero_grad(set_to_none=True)
    loss_real = ops.smooth_l1_mean(D(hr_img), 1.0)
    loss_fake = ops.smooth_l1_mean(D(gen_hr.detach()), 0.0)
    loss_D = (loss_real + loss_fake) / 2
    loss_D.backward()
    opt_D.step()
    ops.bump_weight_epoch()
    return dict(loss_G=loss_G.detach(), loss_D=loss_D.detach(), pixel=pixel.detach(), content=content.detach(),
                loss_gan=loss_gan.detach(), loss_real=loss_real.detach(), loss_fake=loss_fake.detach())
