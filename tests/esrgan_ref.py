"""CPU restatement of ESRGAN (stock torch ops, any dtype: the fp64 referee of the ESRGAN tests).

Written from the architecture.  Generator: conv 3x3 in -> 64; nb residual-in-residual blocks, each three dense blocks (four conv 3x3 +
LeakyReLU(.2) layers growing 64 -> 96 -> 128 -> 160 -> 192 channels by concatenation, then conv 3x3 192 -> 64, result .2 conv + x)
applied one after the other, block result .2 t3 + x; conv 3x3 64 -> 64 and the skip from the head; per upsampling stage nearest x r,
conv 3x3 64 -> 64, LeakyReLU(.2) (or conv 64 -> 64 r r, pixel shuffle, LeakyReLU); conv 3x3 64 -> 64, LeakyReLU(.2), conv 3x3 64 -> out.
Discriminators: conv 3x3 in -> 64 + LeakyReLU, then alternating 4x4 stride-2 and 3x3 convs with BatchNorm and LeakyReLU(.2), widths
64, 64, 128, 128, 256, 256, 512, 512, 512, 512 (, 512, 512) down to S x S, flatten in NCHW order, Linear(512 S S -> 100), LeakyReLU(.2),
Linear(100 -> 1).  Perceptual extractor: (x - mean) / std, then the first 16 convs of VGG19 with ReLUs and four 2 x 2 max pools, the
last conv without its ReLU.  The criteria: binary cross entropy on logits and the squared error against a constant label, mean-reduced,
plain or on the logit minus the other batch's mean logit.  Module names follow the HIP model's state_dict."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

SLOPE = 0.2
VGG_WIDTHS = [64, 64, 'P', 128, 128, 'P', 256, 256, 256, 256, 'P', 512, 512, 512, 512, 'P', 512, 512, 512, 512]


def _conv(cin, cout, k=3, stride=1, pad=1):
    return nn.Conv2d(cin, cout, k, stride, pad)


class Dense5(nn.Module):
    def __init__(self, nf=64, gc=32):
        super().__init__()
        for j in range(4):
            setattr(self, 'conv%d' % (j + 1), nn.Sequential(_conv(nf + gc * j, gc), nn.LeakyReLU(SLOPE)))
        self.conv5 = nn.Sequential(_conv(nf + 4 * gc, nf))

    def forward(self, x):
        feats = x
        for j in range(4):
            feats = torch.cat((feats, getattr(self, 'conv%d' % (j + 1))(feats)), dim=1)
        return self.conv5(feats) * 0.2 + x


class Rrdb(nn.Module):
    def __init__(self):
        super().__init__()
        self.RDB1, self.RDB2, self.RDB3 = Dense5(), Dense5(), Dense5()

    def forward(self, x):
        return self.RDB3(self.RDB2(self.RDB1(x))) * 0.2 + x


class Shortcut(nn.Module):
    def __init__(self, sub):
        super().__init__()
        self.sub = sub

    def forward(self, x):
        return x + self.sub(x)


class Generator(nn.Module):
    def __init__(self, nb, scale=4, in_nc=3, out_nc=3, upsample_mode='upconv'):
        super().__init__()
        r, stages = (3, 1) if scale == 3 else (2, int(round(math.log2(scale))))
        layers = [_conv(in_nc, 64), Shortcut(nn.Sequential(*([Rrdb() for _ in range(nb)] + [_conv(64, 64)])))]
        for _ in range(stages):
            if upsample_mode == 'upconv':
                layers += [nn.Upsample(scale_factor=r, mode='nearest'), _conv(64, 64), nn.LeakyReLU(SLOPE)]
            else:
                layers += [_conv(64, 64 * r * r), nn.PixelShuffle(r), nn.LeakyReLU(SLOPE)]
        layers += [_conv(64, 64), nn.LeakyReLU(SLOPE), _conv(64, out_nc)]
        self.model = nn.Sequential(*layers)

    def forward(self, x):
        return self.model(x)


def head(x, w0, b0, w1, b1):
    """the dense head on an NCHW feature tensor: flatten in NCHW order, Linear, LeakyReLU(.2), Linear"""
    return F.linear(F.leaky_relu(F.linear(x.flatten(1), w0, b0), SLOPE), w1, b1)


class Discriminator(nn.Module):
    def __init__(self, size, in_nc=3):
        super().__init__()
        n_convs = {96: 10, 128: 10, 192: 12, 256: 12}[size]
        widths = [64, 64, 128, 128, 256, 256, 512, 512] + [512] * (n_convs - 8)
        layers, cin = [], in_nc
        for i, cout in enumerate(widths):
            layers.append(_conv(cin, cout, 4, 2, 1) if i % 2 else _conv(cin, cout, 3, 1, 1))
            if i > 0:
                layers.append(nn.BatchNorm2d(cout))
            layers.append(nn.LeakyReLU(SLOPE))
            cin = cout
        self.features = nn.Sequential(*layers)
        side = size >> (n_convs // 2)
        self.classifier = nn.Sequential(nn.Linear(512 * side * side, 100), nn.LeakyReLU(SLOPE), nn.Linear(100, 1))

    def forward(self, x):
        c = self.classifier
        return head(self.features(x), c[0].weight, c[0].bias, c[2].weight, c[2].bias)


class Vgg(nn.Module):
    """VGG19's first 16 convs, the last without its ReLU; keys features.{i}.*, buffers mean and std"""

    def __init__(self, use_input_norm=True):
        super().__init__()
        self.use_input_norm = use_input_norm
        if use_input_norm:
            self.register_buffer('mean', torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1))
            self.register_buffer('std', torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1))
        layers, cin = [], 3
        for item in VGG_WIDTHS:
            if item == 'P':
                layers.append(nn.MaxPool2d(2, 2))
            else:
                layers += [_conv(cin, item), nn.ReLU()]
                cin = item
        self.features = nn.Sequential(*layers[:-1])
        for p in self.features.parameters():
            p.requires_grad_(False)

    def forward(self, x):
        if self.use_input_norm:
            x = (x - self.mean) / self.std
        return self.features(x)


# ---- criteria ---------------------------------------------------------------------------------------------------------------- #

def criterion(x, target_is_real, gan_type, real_label_val=1.0, fake_label_val=0.0):
    if gan_type == 'wgan-gp':
        return -x.mean() if target_is_real else x.mean()
    y = real_label_val if target_is_real else fake_label_val
    if gan_type == 'vanilla':
        return (x.clamp(min=0) - x * y + torch.log1p(torch.exp(-x.abs()))).mean()
    if gan_type == 'lsgan':
        return ((x - y) ** 2).mean()
    raise ValueError(gan_type)


def ragan_d(pred_real, pred_fake, gan_type, real_label_val=1.0, fake_label_val=0.0):
    lab = (real_label_val, fake_label_val)
    return (criterion(pred_real - pred_fake.mean(), True, gan_type, *lab) + criterion(pred_fake - pred_real.mean(), False, gan_type, *lab)) / 2


def ragan_g(pred_real, pred_fake, gan_type, real_label_val=1.0, fake_label_val=0.0):
    lab = (real_label_val, fake_label_val)
    pred_real = pred_real.detach()
    return (criterion(pred_real - pred_fake.mean(), False, gan_type, *lab) + criterion(pred_fake - pred_real.mean(), True, gan_type, *lab)) / 2


def train_iteration(G, D, Fx, opt_G, opt_D, lr, hr, gan_type='vanilla', relative=True, weight_pixel=1e-2, weight_content=1.0,
                    weight_gan=5e-3, l2=False, clip_value=None):
    """one iteration: generator phase (D(gen) then D(hr)), Adam(G); discriminator phase (D(hr) then D(gen detached)), Adam(D), optional
    clamp.  Returns the five scalars as floats."""
    c = F.mse_loss if l2 else F.l1_loss
    opt_G.zero_grad()
    gen = G(lr)
    pixel = c(gen, hr)
    content = c(Fx(gen), Fx(hr).detach())
    if relative:
        pred_fake = D(gen)
        pred_real = D(hr).detach()
        gan = ragan_g(pred_real, pred_fake, gan_type)
    else:
        gan = criterion(D(gen), True, gan_type)
    loss_G = weight_pixel * pixel + weight_content * content + weight_gan * gan
    loss_G.backward()
    opt_G.step()
    opt_D.zero_grad()
    if relative:
        pred_real = D(hr)
        pred_fake = D(gen.detach())
        loss_D = ragan_d(pred_real, pred_fake, gan_type)
    else:
        loss_D = criterion(D(hr), True, gan_type) + criterion(D(gen.detach()), False, gan_type)
    loss_D.backward()
    opt_D.step()
    if clip_value:
        with torch.no_grad():
            for p in D.parameters():
                p.clamp_(-clip_value, clip_value)
    return {k: float(v.detach()) for k, v in (('loss_G', loss_G), ('loss_D', loss_D), ('pixel', pixel), ('content', content),
                                              ('loss_gan', gan))}


# ---- shared by the fixture generator and the tests ----------------------------------------------------------------------------- #

SCALES = (2, 3, 4, 8)
D_SIZES = (96, 128, 192, 256)
LR_SHAPE = (2, 3, 12, 10)           # the generator's recorded LR input (nb = 2)
DEEP_SHAPE = (1, 3, 8, 8)           # nb = 23, x4
STEP_LR, STEP_SCALE, STEP_D = (2, 3, 24, 24), 4, 96
STEP_CASES = [(g, r) for g in ('vanilla', 'lsgan') for r in (True, False)]
# Adam moves every weight by about lr whatever its gradient, a gradient whose sign is roundoff moves it the wrong way, and at B = 2 the
# discriminator's BatchNorms (18 samples per channel at 3 x 3) amplify that into the second iteration's losses.  Measured on the
# reference alone, its fp32 run against an fp64 run of the same loop: 1e-3 at lr 1e-4 (losses of 14 - 22), 6e-6 at lr 1e-5 -- faster
# than linear in lr.  torch's CPU kernels put the discriminator's output within 2.5e-6 of fp64; the component tests allow an
# implementation 1e-5 (fp32) / 5e-5 (split-bf16), 20 x that, and the number of roundoff-signed gradients grows with it: at lr 1e-5
# such an implementation would sit at the step tests' 1e-4 bar for the second iteration.  lr 2e-6 keeps the bar meaningful for every
# implementation the component bars admit, and a wrong-signed Adam step (4e-6) is still far above the 1e-6 the bulk must agree to
ADAM_LR = 2e-6
WEIGHTS = dict(weight_pixel=1e-2, weight_content=1.0, weight_gan=5e-3)


def fill_generator(G, tag=''):
    from oracle import sradsgan_ref as O
    return O.det_init_(G, prefix='esrgan.G%s.' % tag)


def fill_discriminator(D, size):
    from oracle import sradsgan_ref as O
    return O.det_init_(D, prefix='esrgan.D%d.' % size)


def fill_extractor(Fx):
    from oracle import sradsgan_ref as O
    return O.det_init_(Fx, prefix='esrgan.feature_extractor.')        # (the filler's He-style scale for VGG convs)


def gen_input(scale):
    from oracle import sradsgan_ref as O
    return O.det_fill('esrgan.x.%d' % scale, LR_SHAPE, 0.5, 0.5)


def gen_functional(scale, shape=LR_SHAPE):
    """weights of a fixed linear functional of the generator's output (no sign to flip)"""
    from oracle import sradsgan_ref as O
    return O.det_fill('esrgan.r.%d' % scale, (shape[0], 3, shape[2] * scale, shape[3] * scale), 1.0)


def d_input(size):
    from oracle import sradsgan_ref as O
    return O.det_fill('esrgan.d.%d' % size, (2, 3, size, size), 0.5, 0.5)


def step_inputs():
    from oracle import sradsgan_ref as O
    n, _, h, w = STEP_LR
    return (O.det_fill('esrgan.step.x', STEP_LR, 0.5, 0.5),
            O.det_fill('esrgan.step.t', (n, 3, h * STEP_SCALE, w * STEP_SCALE), 0.5, 0.5))


def small_digest(t):
    from oracle import sradsgan_ref as O
    return O.digest(t, full_max=16, nsample=8)


def out_digest(t):
    from oracle import sradsgan_ref as O
    return O.digest(t, full_max=4096, nsample=4096)


def bn_buffers(D):
    return [(k, b) for k, b in sorted(D.state_dict().items()) if 'running' in k]
