"""Plain-torch restatement of the reference HAT generator (SRADSGAN/model/hat.py:74-875), as a function of a state_dict with the
reference's keys.  Any dtype and device (the GPU tests run it in fp64); it follows the reference's tensor graph step by step: roll,
window partition, nn.Unfold, the rearrange, table[rpi.view(-1)] (which wraps the negative OCA indices), the -100 shift mask, and
drop path as x.div(keep) * floor(keep + U) (factors replayed from the HIP model: `factors` maps a HAB index to its (attention, MLP)
factor vectors, i.e. floor(keep + U) / keep)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

MEAN = (0.4488, 0.4371, 0.4040)


def config(upscale, window_size=9, depths=(6, 6, 6, 6, 6, 6), img_size=64):
    return dict(upscale=upscale, window_size=window_size, depths=tuple(depths), img_size=img_size, heads=6, dim=96,
                conv_scale=0.01, img_range=1.0)


def rpi_sa(ws):
    coords = torch.stack(torch.meshgrid([torch.arange(ws), torch.arange(ws)], indexing='ij')).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += ws - 1
    rel[:, :, 1] += ws - 1
    rel[:, :, 0] *= 2 * ws - 1
    return rel.sum(-1)


def rpi_oca(ws, overlap_ratio=0.5):
    wse = ws + int(overlap_ratio * ws)
    ori = torch.stack(torch.meshgrid([torch.arange(ws), torch.arange(ws)], indexing='ij')).flatten(1)
    ext = torch.stack(torch.meshgrid([torch.arange(wse), torch.arange(wse)], indexing='ij')).flatten(1)
    rel = (ext[:, None, :] - ori[:, :, None]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += ws - wse + 1
    rel[:, :, 1] += ws - wse + 1
    rel[:, :, 0] *= ws + wse - 1
    return rel.sum(-1)


def shift_mask(h, w, ws, shift):
    img = torch.zeros((1, h, w, 1))
    sl = (slice(0, -ws), slice(-ws, -shift), slice(-shift, None))
    cnt = 0
    for a in sl:
        for b in sl:
            img[:, a, b, :] = cnt
            cnt += 1
    mw = window_partition(img, ws).view(-1, ws * ws)
    m = mw.unsqueeze(1) - mw.unsqueeze(2)
    return m.masked_fill(m != 0, -100.0).masked_fill(m == 0, 0.0)


def window_partition(x, ws):
    b, h, w, c = x.shape
    x = x.view(b, h // ws, ws, w // ws, ws, c)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, ws, ws, c)


def window_reverse(windows, ws, h, w):
    b = int(windows.shape[0] / (h * w / ws / ws))
    x = windows.view(b, h // ws, w // ws, ws, ws, -1)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(b, h, w, -1)


def _ln(sd, p, x):
    return F.layer_norm(x, (x.shape[-1],), sd[p + '.weight'], sd[p + '.bias'], 1e-5)


def _lin(sd, p, x):
    return F.linear(x, sd[p + '.weight'], sd.get(p + '.bias'))


def _conv(sd, p, x):
    return F.conv2d(x, sd[p + '.weight'], sd[p + '.bias'], 1, sd[p + '.weight'].shape[-1] // 2)


def _mlp(sd, p, x):
    return _lin(sd, p + '.fc2', F.gelu(_lin(sd, p + '.fc1', x)))


def _drop(x, k):
    # drop_path: x.div(keep) * floor(keep + U); k = floor(keep + U) / keep per sample
    return x if k is None else x * k.to(x.dtype).view(-1, 1, 1)


def hab(sd, p, x, x_size, ws, shift, heads, conv_scale, mask, factors):
    h, w = x_size
    b, _, c = x.shape
    shortcut = x
    x = _ln(sd, p + '.norm1', x).view(b, h, w, c)
    t = x.permute(0, 3, 1, 2)
    t = _conv(sd, p + '.conv_block.cab.2', F.gelu(_conv(sd, p + '.conv_block.cab.0', t)))
    y = t.mean((2, 3), keepdim=True)
    y = torch.sigmoid(_conv(sd, p + '.conv_block.cab.3.attention.3', F.relu(_conv(sd, p + '.conv_block.cab.3.attention.1', y))))
    conv_x = (t * y).permute(0, 2, 3, 1).contiguous().view(b, h * w, c)
    sx = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2)) if shift > 0 else x
    xw = window_partition(sx, ws).view(-1, ws * ws, c)
    b_, n, _ = xw.shape
    qkv = _lin(sd, p + '.attn.qkv', xw).reshape(b_, n, 3, heads, c // heads).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0] * (c // heads) ** -0.5, qkv[1], qkv[2]
    attn = q @ k.transpose(-2, -1)
    table = sd[p + '.attn.relative_position_bias_table']
    bias = table[sd['relative_position_index_SA'].view(-1)].view(n, n, -1).permute(2, 0, 1).contiguous()
    attn = attn + bias.unsqueeze(0)
    if shift > 0:
        nw = mask.shape[0]
        attn = attn.view(b_ // nw, nw, heads, n, n) + mask.unsqueeze(1).unsqueeze(0).to(attn.dtype)
        attn = attn.view(-1, heads, n, n)
    attn = attn.softmax(-1)
    xo = _lin(sd, p + '.attn.proj', (attn @ v).transpose(1, 2).reshape(b_, n, c))
    sx = window_reverse(xo.view(-1, ws, ws, c), ws, h, w)
    attn_x = (torch.roll(sx, shifts=(shift, shift), dims=(1, 2)) if shift > 0 else sx).view(b, h * w, c)
    ka, km = factors if factors is not None else (None, None)
    x = shortcut + _drop(attn_x, ka) + conv_x * conv_scale
    return x + _drop(_mlp(sd, p + '.mlp', _ln(sd, p + '.norm2', x)), km)


def ocab(sd, p, x, x_size, ws, heads):
    h, w = x_size
    b, _, c = x.shape
    ows = ws + int(ws * 0.5)
    shortcut = x
    x = _ln(sd, p + '.norm1', x).view(b, h, w, c)
    qkv = _lin(sd, p + '.qkv', x).reshape(b, h, w, 3, c).permute(3, 0, 4, 1, 2)
    q = qkv[0].permute(0, 2, 3, 1)
    kv = torch.cat((qkv[1], qkv[2]), dim=1)
    qw = window_partition(q, ws).view(-1, ws * ws, c)
    kvw = F.unfold(kv, kernel_size=(ows, ows), stride=ws, padding=(ows - ws) // 2)       # b, 2c*ows*ows, nw
    nw = kvw.shape[-1]
    # rearrange 'b (nc ch owh oww) nw -> nc (b nw) (owh oww) ch'
    kvw = kvw.view(b, 2, c, ows * ows, nw).permute(1, 0, 4, 3, 2).reshape(2, b * nw, ows * ows, c)
    kw_, vw = kvw[0], kvw[1]
    b_, nq, _ = qw.shape
    n = kw_.shape[1]
    d = c // heads
    q = qw.reshape(b_, nq, heads, d).permute(0, 2, 1, 3) * d ** -0.5
    k = kw_.reshape(b_, n, heads, d).permute(0, 2, 1, 3)
    v = vw.reshape(b_, n, heads, d).permute(0, 2, 1, 3)
    attn = q @ k.transpose(-2, -1)
    table = sd[p + '.relative_position_bias_table']
    bias = table[sd['relative_position_index_OCA'].view(-1)].view(ws * ws, ows * ows, -1).permute(2, 0, 1).contiguous()
    attn = (attn + bias.unsqueeze(0)).softmax(-1)
    xo = (attn @ v).transpose(1, 2).reshape(b_, nq, c)
    x = window_reverse(xo.view(-1, ws, ws, c), ws, h, w).view(b, h * w, c)
    x = _lin(sd, p + '.proj', x) + shortcut
    return x + _mlp(sd, p + '.mlp', _ln(sd, p + '.norm2', x))


def forward(sd, x, cfg, factors=None):
    """GeneratorResNet.forward (hat.py:859-875).  factors: {HAB index in forward order: (ka, km)} (train-mode drop path)."""
    ws, heads = cfg['window_size'], cfg['heads']
    shift = ws // 2
    ir = cfg['img_range']
    img = cfg['img_size']
    img = img if isinstance(img, (tuple, list)) else (img, img)
    hab_ws_ok = min(img) > ws                      # HAB.__init__: min(input_resolution) <= ws forces shift 0
    h0, w0 = x.shape[2:]
    ph, pw = (ws - h0 % ws) % ws, (ws - w0 % ws) % ws
    if ph or pw:
        x = F.pad(x, (0, pw, 0, ph), 'reflect')
    mean = torch.tensor(MEAN, dtype=torch.float32).to(device=x.device, dtype=x.dtype).view(1, 3, 1, 1)   # torch.Tensor(rgb_mean).type_as(x)
    x = (x - mean) * ir
    x = _conv(sd, 'conv_first', x)
    b, c, h, w = x.shape
    mask = shift_mask(h, w, ws, shift).to(x.device)
    t = x.flatten(2).transpose(1, 2)
    t = _ln(sd, 'patch_embed.norm', t)
    idx = 0
    for i, depth in enumerate(cfg['depths']):
        p = 'layers.%d' % i
        r = t
        for j in range(depth):
            s = shift if (j % 2 == 1 and hab_ws_ok) else 0
            f = factors.get(idx) if factors else None
            r = hab(sd, '%s.residual_group.blocks.%d' % (p, j), r, (h, w), ws, s, heads, cfg['conv_scale'], mask, f)
            idx += 1
        r = ocab(sd, p + '.residual_group.overlap_attn', r, (h, w), ws, heads)
        r = r.transpose(1, 2).contiguous().view(b, c, h, w)
        t = _conv(sd, p + '.conv', r).flatten(2).transpose(1, 2) + t
    t = _ln(sd, 'norm', t)
    f = t.transpose(1, 2).contiguous().view(b, c, h, w)
    x = _conv(sd, 'conv_after_body', f) + x
    x = F.leaky_relu(_conv(sd, 'conv_before_upsample.0', x), 0.01)
    up = cfg['upscale']
    if (up & (up - 1)) == 0:
        stages, r = int(math.log(up, 2)), 2
    elif up % 3 == 0:
        stages, r = int(math.log(up, 3)), 3
    else:
        stages, r = 0, 1
    for _ in range(stages):
        x = F.pixel_shuffle(_conv(sd, 'upsample.upsampling.0', x), r)
    x = _conv(sd, 'conv_last', x)
    return x / ir + mean


def init_(G, prefix='H.'):
    """The fixtures' parameters, by state_dict key (tools/make_golden_hat.py applies it to the reference): det_init_'s filler for
    convs, Linears and the bias tables (std .02), biases U(+-0.01), LayerNorm weights 1 + U(+-0.05)."""
    from oracle import sradsgan_ref as O
    seen = set()
    with torch.no_grad():
        for key, p in G.named_parameters(remove_duplicate=False):
            if id(p) in seen:
                continue
            seen.add(id(p))
            full = prefix + key
            leaf = key.rsplit('.', 1)[-1]
            if ('norm' in key) and p.dim() == 1:
                p.copy_(O.det_fill(full, p.shape, 0.05, 1.0 if leaf == 'weight' else 0.0))
            elif leaf == 'bias':
                p.copy_(O.det_fill(full, p.shape, 0.01))
            else:
                p.copy_(O.det_fill(full, p.shape, 0.02 * math.sqrt(3.0)))
    return G


def state(G, dtype=torch.float64, device='cpu'):
    """state_dict of G as leaf tensors of `dtype` on `device` (index buffers kept int64) that require grad."""
    out = {}
    for k, v in G.state_dict().items():
        if v.dtype.is_floating_point:
            out[k] = v.detach().to(device=device, dtype=dtype).clone().requires_grad_(True)
        else:
            out[k] = v.detach().to(device)
    return out


def inputs(tag, shape, scale, ws):
    """input and an L1 target of the output's shape (the input reflect-padded to multiples of the window, times the scale)"""
    from oracle import sradsgan_ref as O
    x = O.det_fill('hat.x.%s' % tag, shape, 0.5, 0.5)
    h, w = shape[2] + (-shape[2]) % ws, shape[3] + (-shape[3]) % ws
    t = O.det_fill('hat.t.%s' % tag, (shape[0], 3, h * scale, w * scale), 0.5, 0.5)
    return x, t


def np_digest(t, full_max=16, nsample=8):
    a = t.detach().cpu().numpy().astype(np.float32).ravel()
    if a.size <= full_max:
        return a
    stride = a.size // nsample
    a64 = a.astype(np.float64)
    return np.concatenate([a[::stride][:nsample], np.array([a64.sum(), np.sqrt((a64 ** 2).sum())], dtype=np.float32)])
