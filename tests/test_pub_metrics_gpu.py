"""The papers' evaluation protocol on the device (sradsgan_amd/metrics.py, csrc/metrics_pub.hip) against the fp64 restatement of
tests/pub_metrics_ref.py (full 121-tap window, not the kernel's separable form), computed on the bytes copied back.

Tolerances.  RGB mse: equality with the int64 sum divided once.  psnr and luma mse: relative 1e-12 (the kernel's luma sum is an exact
integer, the restatement's an fp64 mean of rounded differences).  ssim: absolute 1e-9 -- moments of values <= 255 carry at most about
22 roundings of magnitude <= 65025 * 2^-53, about 2e-10, against C2 = 58.5 in the smallest denominator factor, while a wrong tap, crop
or normalisation moves SSIM by >= 1e-5.  Largest errors observed on an MI355X are recorded in DESIGN.md section 9."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import pub_metrics_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


T = 16      # the SSIM kernel's tile side; test_against_the_restatement holds the library to it

# (N, H, W, C, crop, y).  With tile side T the valid extents are: T x (T + 1) -- exactly one tile, one tile plus one --, (2T - 4) x
# (T - 5) after a crop of 2, 2T x (T - 1) -- two tiles, one tile less one --, and 282 x 502 = 18 x 32 = 576 tiles for the library's
# 512 blocks per image, so that the grid-stride loop takes a second round.
CASES = [(1, 11, 11, 3, 0, False), (1, 19, 19, 3, 4, True), (2, 23, 37, 3, 0, False), (2, 23, 37, 3, 0, True), (3, 40, 29, 3, 3, True),
         (1, T + 10, T + 11, 3, 0, False), (1, 2 * T + 10, T + 9, 3, 2, True), (1, 2 * T + 14, T + 13, 3, 2, True),
         (1, 300, 520, 3, 4, True), (2, 23, 37, 1, 0, False)]


_REF = {}


def _reference(case):
    """Images [contents * N, H, W, C] uint8 and their restated metrics, computed once per case and never modified."""
    if case not in _REF:
        n, h, w, c, crop, y = case
        imgs_a, imgs_b, want = [], [], []
        for k, kind in enumerate(R.CONTENTS):
            for i in range(n):
                a, b = R.pair(kind, h, w, c, 1000 * k + 10 * i + h)
                imgs_a.append(a)
                imgs_b.append(b)
                want.append((kind, R.metrics(a, b, crop, y)))
        a, b = np.stack(imgs_a), np.stack(imgs_b)
        a.setflags(write=False)
        b.setflags(write=False)
        _REF[case] = (a, b, want)
    return _REF[case]


def _rel(got, want):
    if want == got:
        return 0.0
    return abs(got - want) / abs(want)


def _compare(got, want, y, worst):
    """got: dict of python floats of one image; want: (kind, restated dict)."""
    kind, ref = want
    if y:
        worst['mse_rel'] = max(worst['mse_rel'], _rel(got['mse'], ref['mse']))
        assert _rel(got['mse'], ref['mse']) <= 1e-12, (kind, got['mse'], ref['mse'])
    else:
        assert got['mse'] == ref['mse'], (kind, got['mse'], ref['mse'])
    worst['psnr_rel'] = max(worst['psnr_rel'], _rel(got['psnr'], ref['psnr']))
    assert _rel(got['psnr'], ref['psnr']) <= 1e-12, (kind, got['psnr'], ref['psnr'])
    worst['ssim_abs'] = max(worst['ssim_abs'], abs(got['ssim'] - ref['ssim']))
    assert abs(got['ssim'] - ref['ssim']) <= 1e-9, (kind, got['ssim'], ref['ssim'])
    if kind == 'equal_constants':
        assert got['ssim'] == 1.0 and got['mse'] == 0.0 and got['psnr'] == float('inf')


def _host(m):
    cols = {k: v.cpu().tolist() for k, v in m.items()}
    return [dict((k, cols[k][i]) for k in cols) for i in range(len(cols['mse']))]


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'n%d_%dx%dx%d_crop%d_%s' % (c[:5] + ('y' if c[5] else 'rgb',)))
def test_against_the_restatement(case):
    from sradsgan_amd import metrics as M
    n, h, w, c, crop, y = case
    partials, tile = M.library_config()
    assert tile == T and partials < 18 * 32, 'the shapes above were chosen for this geometry'
    a, b, want = _reference(case)
    m = M.published_metrics_u8(torch.from_numpy(a.copy()).to(DEV), torch.from_numpy(b.copy()).to(DEV), crop, y)
    assert all(v.dtype == torch.float64 and tuple(v.shape) == (len(want),) for v in m.values()) and sorted(m) == ['mse', 'psnr', 'ssim']
    worst = dict(mse_rel=0.0, psnr_rel=0.0, ssim_abs=0.0)
    for got, ref in zip(_host(m), want):
        _compare(got, ref, y, worst)
    print('largest errors %r: luma mse rel %.3e, psnr rel %.3e, ssim abs %.3e' % (case, worst['mse_rel'], worst['psnr_rel'], worst['ssim_abs']))
    # the single-image names: the first image of the batch
    ps, ss = M.calculate_psnr(torch.from_numpy(a[0].copy()).to(DEV), torch.from_numpy(b[0].copy()).to(DEV), crop, y), \
        M.calculate_ssim(torch.from_numpy(a[0].copy()).to(DEV), torch.from_numpy(b[0].copy()).to(DEV), crop, y)
    assert torch.equal(ps, m['psnr'][0]) and torch.equal(ss, m['ssim'][0]) and ps.dim() == 0


def _half_way_floats():
    """float32 x in (0, 1) whose float32 product with 255 is exactly k + 0.5, one list for even k and one for odd k, found by search."""
    even, odd = [], []
    for k in range(255):
        x = np.float32((k + 0.5) / 255.0)
        for cand in (np.nextafter(x, np.float32(0)), x, np.nextafter(x, np.float32(1))):
            if np.float32(cand) * np.float32(255) == np.float32(k + 0.5):
                (odd if k % 2 else even).append(float(cand))
                break
    return even, odd


def _float_pair(n, h, w):
    g = torch.Generator().manual_seed(77)
    x, t = torch.rand(n, 3, h, w, generator=g) * 1.4 - 0.2, torch.rand(n, 3, h, w, generator=g)       # values below 0 and above 1
    even, odd = _half_way_floats()
    assert len(even) >= 4 and len(odd) >= 4, 'the search must find half-way products for even and odd k'
    ties = torch.tensor(even + odd)
    x.view(-1)[:ties.numel()] = ties
    x.view(-1)[ties.numel():ties.numel() + 4] = torch.tensor([float('inf'), float('-inf'), float('nan'), -0.0])
    t.view(-1)[-3:] = torch.tensor([float('nan'), float('inf'), float('-inf')])
    return x, t, ties.numel()


def test_float_front_end_equals_quantise_then_bytes():
    from sradsgan_amd import metrics as M
    from sradsgan_amd.model import gdp_kernels
    x, t, nties = _float_pair(2, 23, 37)
    q_nchw = R.quantise(x.numpy())
    flat = q_nchw.reshape(-1)                       # the order the special values were written in
    assert all(int(flat[i]) % 2 == 0 for i in range(nties)), 'half-way products round to the even byte'
    assert flat[nties:nties + 4].tolist() == [255, 0, 0, 0]                       # +inf, -inf, NaN, -0.0
    want_q = np.ascontiguousarray(q_nchw.transpose(0, 2, 3, 1))
    for fmt in (torch.contiguous_format, torch.channels_last):
        xd, td = x.to(DEV).contiguous(memory_format=fmt), t.to(DEV).contiguous(memory_format=fmt)
        qx, qt = M.quantise(xd), M.quantise(td)
        assert qx.dtype == torch.uint8 and tuple(qx.shape) == (2, 23, 37, 3) and qx.is_contiguous()
        assert np.array_equal(qx.cpu().numpy(), want_q)
        nhwc = xd.permute(0, 2, 3, 1).contiguous()
        assert torch.equal(qx, gdp_kernels.quantize_u8(nhwc, (0.0, 1.0)))
        for crop, y in ((0, False), (3, True), (2, False)):
            mf, mu = M.published_metrics(xd, td, crop, y), M.published_metrics_u8(qx, qt, crop, y)
            for k in ('mse', 'psnr', 'ssim'):
                assert torch.equal(mf[k], mu[k]), (fmt, crop, y, k)
            ref = R.metrics(want_q[1], R.quantise(t.permute(0, 2, 3, 1).numpy())[1], crop, y)
            assert abs(float(mf['ssim'][1]) - ref['ssim']) <= 1e-9 and _rel(float(mf['psnr'][1]), ref['psnr']) <= 1e-12


def test_an_image_has_the_same_bits_alone_and_in_any_batch():
    from sradsgan_amd import metrics as M
    a, b, _ = _reference((1, 300, 520, 3, 4, True))
    img_a, img_b = torch.from_numpy(a[0].copy()).to(DEV), torch.from_numpy(b[0].copy()).to(DEV)
    g = torch.Generator().manual_seed(3)
    fill = torch.randint(0, 256, (2,) + tuple(img_a.shape), generator=g, dtype=torch.uint8).to(DEV)
    for crop, y in ((4, True), (0, False)):
        alone = M.published_metrics_u8(img_a, img_b, crop, y)
        again = M.published_metrics_u8(img_a, img_b, crop, y)
        first = M.published_metrics_u8(torch.cat([img_a[None], fill]), torch.cat([img_b[None], fill.flip(0)]), crop, y)
        last = M.published_metrics_u8(torch.cat([fill, img_a[None]]), torch.cat([fill.flip(0), img_b[None]]), crop, y)
        for k in ('mse', 'psnr', 'ssim'):
            assert torch.equal(alone[k], again[k]), k
            assert torch.equal(alone[k][0], first[k][0]) and torch.equal(alone[k][0], last[k][2]), (crop, y, k)


class Replicate(torch.nn.Module):
    """Stub generator: pixel replication by `scale` (plus a parameter that contributes nothing, to carry the device)."""

    def __init__(self, scale):
        super().__init__()
        self.scale, self.p = scale, torch.nn.Parameter(torch.zeros(1))

    def forward(self, x):
        return x.repeat_interleave(self.scale, 2).repeat_interleave(self.scale, 3) * 0.9 + 0.03 + self.p


def test_evaluate_adds_the_published_keys_and_keeps_the_others():
    from sradsgan_amd import metrics as M, validate as V
    g = torch.Generator().manual_seed(11)
    hr = torch.rand(2, 3, 32, 32, generator=g).to(DEV)
    lr = torch.nn.functional.avg_pool2d(hr, 4)
    bc = torch.rand(2, 3, 32, 32, generator=g).to(DEV)
    gen = Replicate(4).to(DEV).eval()
    protocol = dict(crop_border=4, y_channel=True)
    plain = V.evaluate(gen, lr, hr, 4, bicubic=bc)
    both = V.evaluate(gen, lr, hr, 4, bicubic=bc, protocol=protocol)
    assert sorted(plain['sr']) == ['ergas', 'mse', 'psnr', 'ssim'] and sorted(plain) == sorted(both)
    assert torch.equal(plain['recon'], both['recon'])
    for key, img in (('sr', both['recon']), ('bicubic', bc)):
        assert sorted(both[key]) == ['ergas', 'mse', 'psnr', 'pub_mse', 'pub_psnr', 'pub_ssim', 'ssim']
        for k in plain[key]:
            assert torch.equal(plain[key][k], both[key][k]), (key, k)
        direct = M.published_metrics(img, hr, 4, True)
        for k in ('mse', 'psnr', 'ssim'):
            assert torch.equal(both[key]['pub_' + k], direct[k]), (key, k)
    assert 'pub_psnr' not in V.evaluate(gen, lr, hr, 4)['sr'] and 'bicubic' not in V.evaluate(gen, lr, hr, 4, protocol=protocol)
    # replayed from a captured graph: the eager bits, for two protocols held by two evaluators and for changed inputs
    for proto in (protocol, dict(crop_border=0, y_channel=False)):
        ev = V.GraphedEvaluator(gen, 4, protocol=proto)
        for shift in (0.0, 0.05):
            eager = V.evaluate(gen, lr + shift, hr, 4, bicubic=bc, protocol=proto)
            out = ev(lr + shift, hr, bc)
            for key in ('sr', 'bicubic'):
                for k in eager[key]:
                    assert torch.equal(out[key][k], eager[key][k]), (proto, shift, key, k)
    assert 'pub_psnr' not in V.GraphedEvaluator(gen, 4)(lr, hr, bc)['sr']


def _strip(line, label):
    """A val_log line without its time stamp and without the published keys."""
    import re
    line = re.sub(r'time:[0-9.]+', 'time:', line)
    return re.sub(r'(bicubic|%s)_pub_(psnr|ssim): \S+ ?' % label, '', line).rstrip()


def test_trainer_reports_the_published_averages(tmp_path):
    from sradsgan_amd import metrics as M, trainer as T
    g = torch.Generator().manual_seed(5)

    def loader(n_batches):
        out = []
        for _ in range(n_batches):
            hr = torch.rand(2, 3, 32, 32, generator=g)
            out.append((torch.nn.functional.avg_pool2d(hr, 4), hr, (hr * 0.8 + 0.1).clamp(0, 1), ['x', 'y']))
        return out
    test = loader(2)
    common = dict(scale_factor=4, crop_size=32, hr_height=32, hr_width=32, test_crop_size=12, n_residual_blocks=1, n_basic_blocks=1)
    ref_dir, pub_dir = str(tmp_path / 'ref'), str(tmp_path / 'pub')
    ref = T.SRADSGAN(T.default_args(save_dir=ref_dir, **common), test_loader=test)
    assert ref.eval_protocol is None
    torch.manual_seed(3)
    gen = ref._new_generator()
    gen.apply(T.weights_init_normal)
    path = os.path.join(str(tmp_path), 'g.pkl')
    torch.save(gen.state_dict(), path)
    ref.mfeNew_validate(epoch=1, modelpath=path)
    ref_line = open(os.path.join(ref_dir, 'val_log.txt')).read().strip().splitlines()[-1]
    assert 'pub_' not in ref_line
    avg_ref, _ = ref._evaluate_loader(ref.generator, 'sradsgan')
    assert not any('pub_' in k for k in avg_ref)

    pub = T.SRADSGAN(T.default_args(save_dir=pub_dir, eval_protocol='published', **common), test_loader=test)
    assert pub.eval_protocol == dict(crop_border=4, y_channel=True)
    pub.mfeNew_validate(epoch=1, modelpath=path)
    pub_line = open(os.path.join(pub_dir, 'val_log.txt')).read().strip().splitlines()[-1]
    assert _strip(pub_line, 'sradsgan') == _strip(ref_line, 'sradsgan') and pub_line != ref_line
    keys = [tok[:-1] for tok in pub_line.split() if tok.endswith(':') and ('bicubic_' in tok or 'sradsgan_' in tok)]
    assert keys == [p + k for p in ('bicubic_', 'sradsgan_') for k in ('mse', 'psnr', 'ssim', 'ergas', 'lpips', 'pub_psnr', 'pub_ssim')]
    avg, _ = pub._evaluate_loader(pub.generator, 'sradsgan')
    for k in avg_ref:
        assert avg[k] == pytest.approx(avg_ref[k], rel=1e-9), k            # the reference protocol's numbers are untouched
    # the four averages = the per-batch direct calls, summed and divided
    sums, num = dict.fromkeys(('bicubic_pub_psnr', 'bicubic_pub_ssim', 'sradsgan_pub_psnr', 'sradsgan_pub_ssim'), 0.0), 0
    pub.generator.eval()
    with torch.no_grad():
        for item in test:
            lr, hr, bc = pub._batch(item, test=True)
            for prefix, img in (('bicubic', bc), ('sradsgan', pub.generator(lr))):
                m = M.published_metrics(img, hr, 4, True)
                sums[prefix + '_pub_psnr'] += float(m['psnr'].sum())
                sums[prefix + '_pub_ssim'] += float(m['ssim'].sum())
            num += hr.size(0)
    for k, v in sums.items():
        assert avg[k] == pytest.approx(v / num, rel=1e-12, abs=0), k
        assert ('%s: %.4e ' % (k, avg[k])) in pub_line + ' '

    # the "+" path: the published numbers are those of the self-ensembled output
    from sradsgan_amd.ensemble import SelfEnsemble
    pub.self_ensemble = True
    avg_se, _ = pub._evaluate_loader(pub.generator, 'sradsgan')
    pub.self_ensemble = False
    total = 0.0
    with torch.no_grad():
        for item in test:
            lr, hr, bc = pub._batch(item, test=True)
            total += float(M.published_metrics(SelfEnsemble(pub.generator.eval())(lr), hr, 4, True)['ssim'].sum())
    assert avg_se['sradsgan_pub_ssim'] == pytest.approx(total / num, rel=1e-12, abs=0)
    assert avg_se['bicubic_pub_ssim'] == avg['bicubic_pub_ssim'] and avg_se['sradsgan_pub_ssim'] != avg['sradsgan_pub_ssim']

    # per class: one line per class and the image-weighted Total
    pub.class_loaders = OrderedDict([('airplane', loader(1)), ('beach', loader(2))])
    res = pub.mfeNew_validateByClass(7, modelpath=path)
    for k in sums:
        assert abs(res['Total'][k] - (2 * res['airplane'][k] + 4 * res['beach'][k]) / 6) < 1e-9, k
    lines = open(os.path.join(pub_dir, 'val_log.txt')).read().strip().splitlines()[-3:]
    assert all('sradsgan_pub_ssim:' in ln and 'bicubic_pub_psnr:' in ln for ln in lines) and 'dataset: Total' in lines[-1]
    with torch.no_grad():
        lr, hr, bc = pub._batch(pub.class_loaders['airplane'][0], test=True)
        m = M.published_metrics(pub.generator.eval()(lr), hr, 4, True)
    assert res['airplane']['sradsgan_pub_psnr'] == pytest.approx(float(m['psnr'].sum()) / 2, rel=1e-12, abs=0)
    ref.class_loaders = pub.class_loaders
    assert not any('pub_' in k for k in ref.mfeNew_validateByClass(7, modelpath=path)['Total'])


def test_evaluate_scene():
    from sradsgan_amd import data, scene as S
    g = torch.Generator().manual_seed(9)
    base = torch.rand(24, 32, 3, generator=g)
    hr = (torch.nn.functional.interpolate(base.permute(2, 0, 1)[None], size=(96, 128), mode='bilinear')[0].permute(1, 2, 0) * 255)
    hr = (hr + torch.rand(96, 128, 3, generator=g) * 12).clamp(0, 255).to(torch.uint8).contiguous()
    gen = Replicate(4).to(DEV)
    res = S.evaluate_scene(gen, hr, 4, 12, 3)
    assert sorted(res) == ['bicubic', 'out', 'sr']
    lr = data.resize_u8(hr.to(DEV)[None], 24, 32, 'bicubic')
    assert torch.equal(res['out'], S.super_resolve_scene(gen, lr[0], 4, 12, 3)) and tuple(res['out'].shape) == (96, 128, 3)
    up = data.resize_u8(lr, 96, 128, 'bicubic')[0]
    for key, img in (('sr', res['out']), ('bicubic', up)):
        ref = R.metrics(img.cpu().numpy(), hr.numpy(), 4, True)                 # crop_border None = scale; luma by default
        got = _host(res[key])[0]
        assert _rel(got['mse'], ref['mse']) <= 1e-12 and _rel(got['psnr'], ref['psnr']) <= 1e-12, (key, got, ref)
        assert abs(got['ssim'] - ref['ssim']) <= 1e-9, (key, got, ref)
    rgb = S.evaluate_scene(gen, hr.to(DEV), 4, 12, 3, crop_border=0, y_channel=False, tiles_per_batch=4)
    ref = R.metrics(res['out'].cpu().numpy(), hr.numpy(), 0, False)
    assert torch.equal(rgb['out'], res['out']) and float(rgb['sr']['mse'][0]) == ref['mse']
    assert abs(float(rgb['sr']['ssim'][0]) - ref['ssim']) <= 1e-9
