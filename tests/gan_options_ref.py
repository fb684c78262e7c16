"""CPU references of the four loss options of the reference's GAN trainers (--penalty_type, --grad_penalty_Lp_norm, --loss_Lp_norm,
--relativeGan; SRADSGAN/model/sradsgan.py:595-641, 829-892), in plain torch, for tests that compare the HIP step against them:

  * `train_step`: a restatement of one iteration (:829-892) with all four options and `alpha` injected, every discriminator pass run
    where the reference runs it (five with relativeGan);
  * `gp_ref` / `gp_autograd`: the six (norm, penalty) variants of the penalty reduction on a [npix][C] gradient image, in closed form
    in fp64 and as the reference's own autograd expressions (the fp32 yardstick);
  * `gp_inputs`: the kernel-test inputs with their planted pixels;
  * `scaled_discriminator_init_` and `pixel_norm_shares`: the discriminator of the option goldens, whose input-gradient norms straddle
    1 (with clip-sized weights they are far below 1 and hinge is identically zero), and the shares that show it;
  * `grad_digest` / `bn_buffers`: what tools/make_golden_gan_options.py records per case."""
import math

import numpy as np
import torch
import torch.nn as nn

from oracle import sradsgan_ref as O

NORMS = ('L2', 'L1', 'Linf')
PENALTIES = ('LS', 'hinge')
PAIRS = [(n, p) for n in NORMS for p in PENALTIES]
NON_DEFAULT_PAIRS = [q for q in PAIRS if q != ('L2', 'LS')]
BAND = 1e-3                 # the project's parity bar: pixels this close to a kink may take either side in fp32
BAND_CAP = 0.01             # at most this share of the pixels may sit inside a band

# the recorded training cases: name -> TrainStep / train_step options
CASES = {
    'hinge_linf': dict(penalty_type='hinge', grad_penalty_Lp_norm='Linf'),
    'ls_l1': dict(penalty_type='LS', grad_penalty_Lp_norm='L1'),
    'content_l2': dict(loss_Lp_norm='L2'),
    'relative': dict(relative=True),
}
TRAIN_SHAPE = dict(n_groups=2, n_blocks=1, batch=2, lr_side=8, scale=4)        # train_small's


# --------------------------------------------------------------------------------------------- #
# the penalty reduction on [npix][C]
# --------------------------------------------------------------------------------------------- #


def pixel_norm(g, norm):
    """g: [npix][C] -> [npix], in g's dtype."""
    if norm == 'L2':
        return g.pow(2).sum(1).sqrt()
    if norm == 'L1':
        return g.abs().sum(1)
    return g.abs().max(1)[0]


def gp_ref(g, gout, norm, penalty):
    """(value, dg) of gout * mean_p penalty(norm(g_p) - 1) in fp64, closed form.  L2: 0 where the norm is 0.  L1: sign(g), sign(0) = 0.
    Linf: sign(g) at the FIRST channel that attains max|g|, 0 elsewhere.  LS factor 2 (norm - 1); hinge factor 1 where norm > 1."""
    g = g.double()
    npix, c = g.shape
    nrm = pixel_norm(g, norm)
    d = nrm - 1
    value = (d * d).mean() if penalty == 'LS' else d.clamp_min(0).mean()
    fac = (2 * d if penalty == 'LS' else (d > 0).double()) * (gout / npix)
    if norm == 'L2':
        dn = torch.where(nrm[:, None] > 0, g / nrm.clamp_min(1e-300)[:, None], torch.zeros_like(g))
    elif norm == 'L1':
        dn = torch.sign(g)
    else:
        first = (g.abs() == nrm[:, None]).double().argmax(1)          # argmax of a 0/1 row: the first 1
        dn = torch.zeros_like(g)
        dn[torch.arange(npix), first] = torch.sign(g[torch.arange(npix), first])
    return value, fac[:, None] * dn


def gp_expression(grads, norm, penalty):
    """sradsgan.py:624-637 on a 4-d gradient tensor, verbatim in structure: the expression autograd differentiates."""
    if norm == 'Linf':
        nrm, _ = torch.max(torch.abs(grads), 1)
    elif norm == 'L1':
        nrm = grads.norm(1, 1)
    else:
        nrm = grads.norm(2, 1)
    cons = (nrm - 1).pow(2) if penalty == 'LS' else torch.nn.ReLU()(nrm - 1)
    return cons.mean()


def as4(x):
    """[npix][C] memory as the [1, C, 1, npix] NHWC tensor ops.gp_penalty takes."""
    return x.view(1, 1, x.shape[0], x.shape[1]).permute(0, 3, 1, 2)


def gp_autograd(g, gout, norm, penalty, dtype=torch.float32):
    """(value, dg) from stock torch autograd of gp_expression in `dtype` on the CPU."""
    x = g.to(dtype).clone().requires_grad_()
    v = gp_expression(as4(x), norm, penalty)
    (v * gout).backward()
    return v.detach(), x.grad


# Planted pixels (3 channels; C = 4 appends a zero channel, C = 1 keeps the first entry).  name -> values
PLANTED = (
    ('zero', (0.0, 0.0, 0.0)),                  # gradient 0 in every variant
    ('unit_first', (1.0, 0.0, 0.0)),            # norm exactly 1 in all three kinds: hinge factor 0, LS factor 0
    ('unit_second_neg', (0.0, -1.0, 0.0)),
    ('l1_one', (0.5, -0.25, 0.25)),             # L1 norm exactly 1
    ('tie_half', (0.5, -0.5, 0.25)),            # Linf tie between channels 0 and 1: the gradient goes to channel 0 only
    ('tie_two', (-2.0, 2.0, 2.0)),              # three-way Linf tie, negative first
)
ZERO_ENTRY_CHANNEL = 1      # the pixel behind the planted ones carries an exact 0 here (c > 1), non-zero elsewhere
MIN_PLANTED_NPIX = 16


def planted_pixels(c):
    rows = []
    for _, v in PLANTED:
        rows.append((list(v) + [0.0])[:c] if c != 3 else list(v))
    return torch.tensor(rows, dtype=torch.float32)


def planted_rows(npix, c):
    """Row indices of the planted pixels (spread over the blocks of the launch) and of the zero-entry pixel; empty for npix < 16."""
    if npix < MIN_PLANTED_NPIX:
        return [], None
    n = len(PLANTED)
    rows = [(i * (npix - 1)) // n for i in range(n)]               # 0, ..., strictly increasing for npix >= 16
    return rows, npix - 1


def gp_inputs(npix, c, seed=0):
    """[npix][C] fp32 gradient image whose three norms all straddle 1 (N(0, 1 / C) entries times a per-pixel factor in [0.3, 1.7]), the
    planted pixels at planted_rows,
    and -- apart from those -- no pixel whose fp64 L2, L1 or Linf norm lies within 1e-5 of 1 (such a pixel is scaled by 1.01 until it
    does not): away from the planted kinks fp32 and fp64 take the same side of every mask."""
    gen = torch.Generator().manual_seed(4242 + npix + 10 * c + 1000 * seed)
    t = torch.randn(npix, c, generator=gen) / math.sqrt(c) * (0.3 + 1.4 * torch.rand(npix, 1, generator=gen))
    rows, zrow = planted_rows(npix, c)
    if rows:
        t[rows] = planted_pixels(c)
        if c > 1:
            t[zrow, ZERO_ENTRY_CHANNEL] = 0.0
    for _ in range(8):
        near = torch.zeros(npix, dtype=torch.bool)
        for norm in NORMS:
            near |= (pixel_norm(t.double(), norm) - 1).abs() <= 1e-5
        if rows:
            near[rows] = False
        if not bool(near.any()):
            break
        t[near] = t[near] * 1.01
    return t


def gp_exact_planted(norm, c):
    """Names of the planted pixels whose dg the kernel's fp32 arithmetic yields without any rounding when gout / npix is a power of
    two: everything L1 and Linf (factor and sign only); for L2 the pixels whose factor is exactly 0."""
    if norm == 'L2':
        return ('zero', 'unit_first', 'unit_second_neg') if c >= 3 else ('zero', 'unit_first')
    return tuple(k for k, _ in PLANTED)


# --------------------------------------------------------------------------------------------- #
# the discriminator of the option goldens
# --------------------------------------------------------------------------------------------- #

GP_GAIN = 5.0               # std of the conv / linear weights = GP_GAIN x 0.02 (chosen once; the golden script asserts the shares)
TRAIN_GAIN = 3.0            # the same for the recorded training cases (their interpolates see larger gradients than the penalty inputs)
GP_CLIP = 0.2               # a clip_value that keeps every filled weight (|w| <= GP_GAIN * 0.02 * sqrt 3 = 0.173)


def scaled_discriminator_init_(D, prefix='D.', gain=GP_GAIN):
    """O.det_init_, then every weight with >= 2 dimensions refilled by the same deterministic filler with `gain` times the std."""
    O.det_init_(D, prefix=prefix)
    with torch.no_grad():
        for key, p in D.named_parameters():
            if p.dim() >= 2:
                p.copy_(O.det_fill(prefix + key, p.shape, gain * 0.02 * math.sqrt(3.0)))
    return D


def input_gradient(D, real, fake, alpha):
    """d sum(D(interp)) / d interp, [B, C, H, W], without touching D's running statistics' role in the value (train mode)."""
    interp = (alpha * real + (1 - alpha) * fake).requires_grad_(True)
    out = D(interp)
    return torch.autograd.grad(out, interp, torch.ones_like(out))[0]


def pixel_norm_shares(grads, norm):
    """For a [B, C, H, W] gradient: (share of pixels with norm > 1, share within BAND of 1, share whose two largest |g| lie within
    BAND of each other (Linf only, else 0), smallest |norm - 1|), all judged in fp64."""
    g = grads.detach().double().permute(0, 2, 3, 1).reshape(-1, grads.shape[1])
    nrm = pixel_norm(g, norm)
    above = float((nrm > 1).double().mean())
    band = float(((nrm - 1).abs() <= BAND).double().mean())
    tie = 0.0
    if norm == 'Linf' and g.shape[1] > 1:
        top = g.abs().sort(1, descending=True)[0]
        tie = float(((top[:, 0] - top[:, 1]) <= BAND).double().mean())
    return above, band, tie, float((nrm - 1).abs().min())


def shares_ok(above, band, tie):
    return 0.2 <= above <= 0.8 and band <= BAND_CAP and tie <= BAND_CAP


# --------------------------------------------------------------------------------------------- #
# one training iteration with the options (sradsgan.py:829-892)
# --------------------------------------------------------------------------------------------- #


def train_step(G, D, Fx, opt_G, opt_D, lr_img, hr_img, alpha, weight_content=1e-2, weight_gan=1e-3, lambda_gp=10.0, clip_value=0.01,
               use_gp=True, penalty_type='LS', grad_penalty_Lp_norm='L2', loss_Lp_norm='L1', relative=False):
    """One iteration as the reference writes it.  Afterwards G's .grad holds the G phase's gradients and D's the D phase's.  Returns
    the logged scalars, the three terms of loss_G, the penalty, and mean(D(real)) of the D phase."""
    crit = nn.L1Loss() if loss_Lp_norm == 'L1' else nn.MSELoss()                 # :685-688
    gan = O.GANLoss('wgan-gp')
    # ---- generator (:829-858) ----
    opt_G.zero_grad()
    gen_hr = G(lr_img)
    pixel = crit(gen_hr, hr_img)
    content = crit(Fx(gen_hr), Fx(hr_img).detach())
    if relative:                                                                 # :840-844
        pred_g_fake = D(gen_hr)
        pred_d_real = D(hr_img).detach()
        loss_gan = (gan(pred_d_real - torch.mean(pred_g_fake), False) + gan(pred_g_fake - torch.mean(pred_d_real), True)) / 2
    else:
        loss_gan = gan(D(gen_hr), True)
    loss_G = pixel + weight_content * content + weight_gan * loss_gan
    loss_G.backward()
    opt_G.step()
    # ---- discriminator (:865-892) ----
    opt_D.zero_grad()
    if relative:                                                                 # :868-873
        pred_d_real = D(hr_img)
        pred_d_fake = D(gen_hr.detach())
        loss_D = (gan(pred_d_real - torch.mean(pred_d_fake), True) + gan(pred_d_fake - torch.mean(pred_d_real), False)) / 2
    else:
        pred_d_real = D(hr_img)
        loss_D = gan(pred_d_real, True) + gan(D(gen_hr.detach()), False)
    gp = torch.zeros((), dtype=hr_img.dtype)
    if use_gp:
        gp = O.gradient_penalty(D, hr_img.detach(), gen_hr.detach(), alpha, grad_penalty_Lp_norm, penalty_type)
        loss_D = loss_D + lambda_gp * gp
    loss_D.backward()
    opt_D.step()
    with torch.no_grad():
        for p in D.parameters():
            p.clamp_(-clip_value, clip_value)
    return dict(loss_G=loss_G.item(), loss_D=loss_D.item(), pixel=pixel.item(), content=content.item(), loss_gan=loss_gan.item(),
                gp=float(gp.detach()), d_real_mean=float(pred_d_real.detach().mean()), gen_hr=gen_hr.detach())


SCALARS = ('loss_G', 'loss_D', 'pixel', 'content', 'loss_gan', 'gp')


def case_inputs(tag='train_small', it=0, batch=2, lr_side=8, scale=4):
    lr_img = O.det_fill('%s.lr.%d' % (tag, it), (batch, 3, lr_side, lr_side), 0.5, 0.5)
    hr_img = O.det_fill('%s.hr.%d' % (tag, it), (batch, 3, lr_side * scale, lr_side * scale), 0.5, 0.5)
    return lr_img, hr_img


def grad_digest(net, nsample=8):
    """Per parameter tensor in named_parameters() order: up to `nsample` evenly strided gradient entries and max|g|.  Returns
    (names, samples [sum of counts], counts, maxabs)."""
    names, samples, counts, maxabs = [], [], [], []
    for k, p in net.named_parameters():
        if p.grad is None:
            continue
        a = p.grad.detach().cpu().double().numpy().ravel()
        s = a[::max(1, a.size // nsample)][:nsample]
        names.append(k), samples.append(s), counts.append(s.size), maxabs.append(np.abs(a).max())
    return np.array(names), np.concatenate(samples), np.array(counts, dtype=np.int64), np.array(maxabs)


def digest_score(net, names, samples, counts, maxabs, skip=(), floor=1e-2):
    """parity_util.grad_score's measure on the recorded digest: max over tensors of max|dg| over the recorded entries /
    max(max|g_tensor|, floor * max|g_network|); returns (score, worst tensor)."""
    g_names, g_samples, g_counts, _ = grad_digest(net)
    assert list(g_names) == list(names) and list(g_counts) == list(counts)
    net_scale = float(np.max(maxabs))
    worst, worst_key, off = 0.0, '', 0
    for k, n, own in zip(names, counts, maxabs):
        d = float(np.abs(g_samples[off:off + n] - samples[off:off + n]).max())
        off += n
        if str(k).endswith(tuple(skip)):
            continue
        s = d / max(float(own), floor * net_scale, 1e-30)
        if s > worst:
            worst, worst_key = s, str(k)
    return worst, worst_key


def bn_buffers(D):
    """(names, running_mean and running_var values concatenated in state_dict order, num_batches_tracked per BatchNorm)."""
    names, vals, nbt = [], [], []
    for k, v in D.state_dict().items():
        if 'running_' in k:
            names.append(k)
            vals.append(v.detach().cpu().double().numpy().ravel())
        elif k.endswith('num_batches_tracked'):
            nbt.append(int(v))
    return np.array(names), np.concatenate(vals), np.array(nbt, dtype=np.int64)
