"""The dihedral kernels (csrc/augment.hip) and what is built on them -- data.Augment, ensemble.self_ensemble, the trainer's switches --
on the device.  Every kernel here is an exact permutation (the merge: a fixed-order fp32 sum), so every comparison is bit for bit:
against the numpy restatement tests/augment_ref.py and against the reference's recorded items (tests/golden/augment.npz)."""
import inspect
import itertools

import numpy as np
import pytest
import torch

from tests import augment_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _run_augment(src, params, cs, sigma=0.0, z=None, seed=0, step=0):
    from sradsgan_amd import data as D
    out = D.augment_u8(torch.from_numpy(src).to(DEV), torch.from_numpy(np.asarray(params, np.int32)).to(DEV), cs, sigma,
                       None if z is None else torch.from_numpy(z).to(DEV), seed, step)
    assert out.dtype == torch.uint8 and out.is_contiguous()
    return out.cpu().numpy()


# --------------------------------------------------------------------------------------------- #
# srhip_augment_u8
# --------------------------------------------------------------------------------------------- #

@pytest.mark.parametrize('c', [3, 4])
def test_augment_crop_and_every_op_per_sample(c):
    """13 x 11 source, crop 7: a row is 21 (C = 3) or 28 bytes, so with C = 3 the rows start at every byte phase and the scalar head
    and tail both run; three samples with three different ops and offsets per launch; the offsets cover both corners and an
    interior point; the eight launches rotate every op through every sample slot."""
    rng = np.random.RandomState(11 + c)
    src = rng.randint(0, 256, (3, 13, 11, c)).astype(np.uint8)
    offsets = [(0, 0), (13 - 7, 11 - 7), (2, 3)]
    for k in range(8):
        params = [[offsets[(n + k) % 3][0], offsets[(n + k) % 3][1], (k + 3 * n) % 8, 0] for n in range(3)]
        assert np.array_equal(_run_augment(src, params, 7), R.augment(src, params, 7)), params
    seen = {(k + 3 * n) % 8 for k in range(8) for n in range(3)}
    assert seen == set(range(8))


@pytest.mark.parametrize('c', [3, 4])
def test_augment_without_a_crop_and_past_one_wave_of_columns(c):
    rng = np.random.RandomState(5)
    src = rng.randint(0, 256, (3, 8, 8, c)).astype(np.uint8)                          # cs = H = W = 8: the op alone
    for k in range(0, 8, 3):
        params = [[0, 0, (k + n) % 8, 0] for n in range(3)]
        assert np.array_equal(_run_augment(src, params, 8), R.augment(src, params, 8))
    src = rng.randint(0, 256, (2, 70, 69, c)).astype(np.uint8)                        # cs = 67: past any 64-wide tiling, odd row bytes
    for params in ([[3, 2, 3, 0], [0, 0, 4, 0]], [[1, 0, 5, 0], [3, 2, 6, 0]], [[0, 2, 7, 0], [2, 1, 1, 0]], [[3, 0, 2, 0], [1, 1, 0, 0]]):
        assert np.array_equal(_run_augment(src, params, 67), R.augment(src, params, 67)), params


def test_augment_reproduces_the_recorded_reference_items(golden):
    g = golden('augment')
    cases, cs = g['cases'], g['hr'].shape[1]
    src = np.ascontiguousarray(g['src'][cases[:, 0]])                                 # one batch row per case
    params = [[y0, x0, R.OP_OF[(rv, lr, tb)], 0] for _, y0, x0, rv, lr, tb in cases.tolist()]
    assert np.array_equal(_run_augment(src[:-1], params[:-1], cs), g['hr'][:-1])
    z = np.zeros((len(cases), cs, cs, 3), np.float32)
    z[-1] = g['noise_z']                                                              # the noise case is the last row
    got = _run_augment(src, params, cs, float(g['noise_sigma']), z)
    assert np.array_equal(got[-1], g['hr'][-1]) and np.array_equal(got[:-1], g['hr'][:-1])     # z = 0 adds nothing


def test_out_of_range_table_rows_write_zeros_not_out_of_bounds():
    src = np.full((4, 9, 9, 3), 200, np.uint8)
    got = _run_augment(src, [[3, 0, 0, 0], [0, -1, 0, 0], [0, 0, 8, 0], [2, 2, 7, 0]], 7)
    assert not got[:3].any() and (got[3] == 200).all()


# --------------------------------------------------------------------------------------------- #
# noise
# --------------------------------------------------------------------------------------------- #

def test_supplied_noise_is_numpys_float64_result():
    """trunc(clip(double(byte) + sigma * z, 0, 255)).  Besides ordinary draws, z is set so that the sum lands within 1e-6 on either
    side of an integer (truncation, not rounding, and no fp32 shortcut: next to a byte of 16 or more an fp32 sum cannot hold 1e-6)
    and far beyond both ends.  sigma is a power of two and the crafted |z| < 1, so fp32 z moves the sum by at most 4 * 2^-25."""
    rng = np.random.RandomState(2)
    n, cs, sigma = 3, 7, 4.0
    src = rng.randint(0, 256, (n, 13, 11, 3)).astype(np.uint8)
    params = [[0, 0, 5, 0], [6, 4, 0, 0], [2, 3, 6, 0]]
    z = rng.standard_normal((n, cs, cs, 3)).astype(np.float32) * 8
    flat = z.reshape(n, -1)
    for s in range(n):
        for j, (off, d) in enumerate([(2, 5e-7), (2, -5e-7), (-1, 8e-7), (-1, -8e-7), (1, -3e-7), (0, 4e-7), (-2, -2e-7)]):
            flat[s, 5 * j] = np.float32((off + d) / sigma)
        flat[s, 40:44] = [1e4, -1e4, np.float32(3e38), np.float32(-3e38)]
    want = R.augment(src, params, cs, sigma, z)
    sums = src[0, :cs, :cs].reshape(-1).astype(np.float64) + sigma * flat[0].astype(np.float64)
    near = np.abs(sums - np.rint(sums))[[0, 5, 10, 15, 20, 25, 30]]
    assert (near < 1e-6).all() and (near > 0).all()                                   # the crafted sums are where they should be
    assert np.array_equal(_run_augment(src, params, cs, sigma, z), want)
    assert not np.array_equal(want, R.augment(src, params, cs))


@pytest.mark.parametrize('c', [3, 4])
def test_drawn_noise_is_the_supplied_path_fed_with_randn_rows(c):
    from sradsgan_amd.model import gdp_kernels as K
    rng = np.random.RandomState(9)
    n, cs, sigma, seed = 3, 7, 20.0, 1234567
    src = rng.randint(0, 256, (n, 13, 11, c)).astype(np.uint8)
    params = [[1, 2, 3, 0], [6, 4, 6, 0], [0, 0, 0, 0]]
    outs = []
    for step in (0, 5):
        z = K.randn_rows(torch.empty(n, cs, cs, c, device=DEV), seed, step).cpu().numpy()
        drawn = _run_augment(src, params, cs, sigma, None, seed, step)
        assert np.array_equal(drawn, _run_augment(src, params, cs, sigma, z))
        assert np.array_equal(drawn, R.augment(src, params, cs, sigma, z))
        outs.append(drawn)
    assert not np.array_equal(outs[0], outs[1])                                       # the step is part of the key


def test_augment_call_records_its_draws_and_advances_the_step():
    from sradsgan_amd import data as D
    from sradsgan_amd.model import gdp_kernels as K
    rng = np.random.RandomState(4)
    src = rng.randint(0, 256, (4, 16, 16, 3)).astype(np.uint8)
    aug = D.Augment(13, 2, random_crop=True, rotate=True, fliplr=True, fliptb=True, noise=['Gaussain', 6.0], seed=40, rank=2)
    twin = D.Augment(13, 2, random_crop=True, rotate=True, fliplr=True, fliptb=True, noise=['Gaussain', 6.0], seed=42)
    for call in range(2):
        out = aug(torch.from_numpy(src).to(DEV))
        assert aug.last_step == call and torch.equal(aug.last_params, twin.draw(4, 16, 16))
        z = K.randn_rows(torch.empty(4, 12, 12, 3, device=DEV), 42, call).cpu().numpy()
        assert np.array_equal(out.cpu().numpy(), R.augment(src, aug.last_params.numpy(), 12, 6.0, z))


@pytest.mark.parametrize('scale', [2, 3])
def test_augmented_training_batch_equals_the_recorded_items(golden, scale):
    from sradsgan_amd import data as D
    g = golden('augment')
    cases = g['cases']
    src = torch.from_numpy(np.ascontiguousarray(g['src'][cases[:, 0]])).to(DEV)
    table = torch.tensor([[y0, x0, R.OP_OF[(rv, lr, tb)], 0] for _, y0, x0, rv, lr, tb in cases.tolist()], dtype=torch.int32)
    aug = D.Augment(13, scale) if scale == 2 else D.Augment(14, scale)                # calculate_valid_crop_size -> 12 both times
    assert aug.crop_size == 12
    aug.draw = lambda n, h, w: table[:n]                                              # the recorded draws instead of random ones

    def planes(name, rows):
        return (torch.from_numpy(g[name][rows]).float() / 255.0).permute(0, 3, 1, 2)    # to_tensor

    lr, hr, bc = D.augmented_training_batch(src[:-1], scale, aug)
    rows = slice(0, len(cases) - 1)
    assert _same_bits(hr, planes('hr', rows)) and _same_bits(lr, planes('lr%d' % scale, rows)) and _same_bits(bc, planes('bc%d' % scale, rows))
    noisy = D.Augment(12, scale, noise=['Gaussain', float(g['noise_sigma'])])
    noisy.draw = lambda n, h, w: table[-1:]
    z = torch.from_numpy(g['noise_z'][None]).to(DEV)
    lr, hr, bc = D.training_batch(noisy(src[-1:], z=z), scale)
    rows = slice(len(cases) - 1, len(cases))
    assert _same_bits(hr, planes('hr', rows)) and _same_bits(lr, planes('lr%d' % scale, rows)) and _same_bits(bc, planes('bc%d' % scale, rows))


# --------------------------------------------------------------------------------------------- #
# srhip_dihedral_f32
# --------------------------------------------------------------------------------------------- #

def _torch_op(x, op):
    if op & 1:
        x = x.transpose(2, 3)
    if op & 2:
        x = x.flip(2)
    if op & 4:
        x = x.flip(3)
    return x.contiguous()


@pytest.mark.parametrize('shape', [(2, 3, 5, 7), (1, 64, 5, 7)])
@pytest.mark.parametrize('layout', ['nchw', 'channels_last', 'sliced'])
def test_dihedral_is_torch_flip_and_transpose_bit_for_bit(shape, layout):
    """C = 3: the scalar kernel in both thread orders; C = 64 channels_last: the float4 kernel; 'sliced': a view with gaps in every
    stride (and, for C = 64, a 16-byte-misaligned base that sends channels_last data down the scalar kernel)."""
    from sradsgan_amd import ensemble as E
    g = torch.Generator().manual_seed(shape[1])
    x = torch.randn(shape, generator=g)
    x[0, 0, 0, :3] = torch.tensor([-0.0, float('inf'), 1e-42])                          # a permutation keeps every bit pattern
    if layout == 'nchw':
        xd = x.to(DEV)
    elif layout == 'channels_last':
        xd = x.to(DEV).contiguous(memory_format=torch.channels_last)
    else:
        n, c, h, w = shape
        big = torch.zeros(n, h + 1, w + 2, c + 1, device=DEV)
        xd = big[:, 1:, 1:w + 1, 1:].permute(0, 3, 1, 2)
        xd.copy_(x)
    for op in range(8):
        y = E.dihedral(xd, op)
        assert _same_bits(y, _torch_op(x, op)), op
        if layout == 'channels_last':
            assert y.is_contiguous(memory_format=torch.channels_last)
    assert _same_bits(xd, x)                                                           # the input is only read


# --------------------------------------------------------------------------------------------- #
# srhip_ensemble_merge_f32
# --------------------------------------------------------------------------------------------- #

@pytest.mark.parametrize('ops', [[3], [5, 0, 6], [7, 2, 5, 0, 3, 6, 1, 4]])
def test_merge_is_the_fixed_order_fp32_sum(ops):
    from sradsgan_amd import ensemble as E
    g = torch.Generator().manual_seed(len(ops))
    views = []
    for k, op in enumerate(ops):
        v = torch.randn((2, 3, 14, 10) if op & 1 else (2, 3, 10, 14), generator=g) * (10.0 ** (k % 3))
        views.append(v)
    dev = [v.to(DEV).contiguous(memory_format=torch.channels_last) if k % 2 else v.to(DEV) for k, v in enumerate(views)]
    want = R.merge([v.numpy() for v in views], ops)
    got = E.merge(dev, ops)
    assert tuple(got.shape) == (2, 3, 10, 14) and _same_bits(got, torch.from_numpy(want))
    assert _same_bits(E.merge(dev, ops), got)                                          # two runs, the same bits
    if len(ops) > 1:                                                                   # the order is part of the contract
        again = R.merge([v.numpy() for v in views[::-1]], ops[::-1])
        assert _same_bits(E.merge(dev[::-1], ops[::-1]), torch.from_numpy(again))


# --------------------------------------------------------------------------------------------- #
# self_ensemble
# --------------------------------------------------------------------------------------------- #

def _upsample2(x):
    return x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def test_self_ensemble_of_an_equivariant_stub_returns_the_plain_upsample():
    """Pixel repetition commutes with every op, so every view maps back to the same tensor u and the merge is (m u) * fp32(1 / m).
    Inputs are k / 256 with few mantissa bits, so m u is exact; fp32(1 / m) * m = 1 + e with e = 0 (m = 1, 2, 4, 8), 2^-25 (3, 6),
    2^-26 (5), 3 * 2^-26 (7), and u (1 + e) rounds back to u whenever e times the mantissa f in [1, 2) of u stays under half an
    ulp = 2^-24: always for m != 7, and for m = 7 when f < 4/3.  The k below all have f < 4/3, so EVERY subset must return u bit
    for bit -- which pins the inverse addressing of all eight ops end to end (a wrong inverse moves pixels of an asymmetric image)."""
    from sradsgan_amd import ensemble as E
    allowed = [k for k in range(1, 256) if k / 2.0 ** int(np.floor(np.log2(k))) < 4.0 / 3.0]
    assert len(allowed) > 80
    idx = np.arange(2 * 3 * 6 * 10)
    lr = torch.tensor([allowed[(7 * i + i // 10) % len(allowed)] for i in idx], dtype=torch.float32).view(2, 3, 6, 10) / 256.0
    for op in range(1, 8):                                                             # asymmetric: no op leaves it alone
        assert op & 1 or not np.array_equal(R.apply_op(lr.numpy(), op, (2, 3)), lr.numpy())
    want = _upsample2(lr)
    lrd = lr.to(DEV)
    for m in range(1, 9):
        for ops in itertools.combinations(range(8), m):
            assert _same_bits(E.self_ensemble(_upsample2, lrd, ops), want), ops
    assert _same_bits(E.self_ensemble(_upsample2, lrd, [6, 1, 3, 0, 4], chunk=2), want)
    assert _same_bits(E.SelfEnsemble(torch.nn.Upsample(scale_factor=2, mode='nearest'))(lrd), want)
    assert _same_bits(E.self_ensemble(_upsample2, lrd.contiguous(memory_format=torch.channels_last), range(8)), want)


def test_self_ensemble_of_a_package_generator():
    """EDSR at the width the EDSR tests use (256; the reference hard-codes it), one residual block, x2, LR 6 x 10."""
    from sradsgan_amd import ensemble as E
    from sradsgan_amd.model.edsr import Net
    from tests.parity_util import rel_err, sibling_grad_check
    torch.manual_seed(4)
    net = Net(3, 256, 1, upscale_factor=2).to(DEV).eval()
    lr = torch.rand(2, 3, 6, 10, generator=torch.Generator().manual_seed(8))
    lrd = lr.to(DEV)
    with torch.no_grad():
        plain = net(lrd)
        assert _same_bits(E.self_ensemble(net, lrd, ops=[0]), plain)
        by_hand = [net(_torch_op(lrd, op)).cpu().numpy() for op in range(8)]          # eight separate calls on torch-made views
    want = torch.from_numpy(R.merge(by_hand, list(range(8))))
    one = E.self_ensemble(net, lrd, chunk=1)
    assert tuple(one.shape) == (2, 3, 12, 20) and _same_bits(one, want)
    assert not _same_bits(one, plain)
    stacked = E.self_ensemble(net, lrd)
    # stacking changes the batch the convolutions see: agreement at the module-output tolerance of tests/parity_util.py
    tol = inspect.signature(sibling_grad_check).parameters['rtol'].default
    err = rel_err(stacked, one)
    print('self_ensemble stacked vs view by view: rel err %.3e (bar %.0e)' % (err, tol))
    assert err < tol
    assert _same_bits(E.self_ensemble(net, lrd), stacked)


# --------------------------------------------------------------------------------------------- #
# trainer
# --------------------------------------------------------------------------------------------- #

def _trainer_run(tmp_path, tag, src):
    from sradsgan_amd import trainer as T

    class Recording(T.SRADSGAN):
        def _batch(self, item, test=False):
            out = super()._batch(item, test)
            if not test:
                self.seen.append((self.augment.last_params.clone(), self.augment.last_step, out[0].clone(), out[1].clone()))
            return out

    g = torch.Generator().manual_seed(6)
    hr = torch.rand(2, 3, 12, 12, generator=g)
    test = [(torch.nn.functional.avg_pool2d(hr, 2), hr, hr.clamp(0, 1), ['a', 'b'])]
    args = T.default_args(scale_factor=2, num_epochs=1, batch_size=2, save_dir=str(tmp_path / tag), crop_size=12, hr_height=12,
                          hr_width=12, sample_interval=1, n_residual_blocks=1, n_basic_blocks=1, augment_random_crop=True,
                          augment_rotate=True, augment_fliplr=True, augment_fliptb=True, augment_noise=['Gaussain', 5.0],
                          augment_seed=77, self_ensemble=True)
    torch.manual_seed(31)
    np.random.seed(31)
    net = Recording(args, train_loader=[torch.from_numpy(s) for s in src], test_loader=test)
    net.seen = []
    hist = net.train()
    return net, hist, test


def test_trainer_trains_on_augmented_batches_and_validates_with_self_ensemble(tmp_path):
    from sradsgan_amd import data as D
    from sradsgan_amd import ensemble as E
    from sradsgan_amd import validate as V
    from sradsgan_amd.model import gdp_kernels as K
    rng = np.random.RandomState(12)
    src = [rng.randint(0, 256, (2, 16, 16, 3)).astype(np.uint8) for _ in range(2)]      # two iterations of batch 2
    net, hist, test = _trainer_run(tmp_path, 'a', src)
    assert isinstance(net.augment, D.Augment) and len(net.seen) == 2 and len(hist) == 1
    tables = []
    for k, (params, step, lr, hr) in enumerate(net.seen):
        assert step == k and int(params[:, 0].max()) <= 4 and int(params[:, 1].max()) <= 4
        z = K.randn_rows(torch.empty(2, 12, 12, 3, device=DEV), 77, step).cpu().numpy()
        tile = R.augment(src[k], params.numpy(), 12, 5.0, z)                           # what Augment must have produced
        want_lr, want_hr, _ = D.training_batch(torch.from_numpy(tile).to(DEV), 2)
        assert _same_bits(hr, want_hr) and _same_bits(lr, want_lr)
        assert _same_bits(hr, (torch.from_numpy(tile).float() / 255.0).permute(0, 3, 1, 2))
        tables.append(params)
    # the validation inside train() and a fresh validate() both used the wrapped generator
    assert all(np.isfinite([hist[0][k] for k in ('loss_G', 'loss_D', 'psnr', 'ssim', 'ergas')]))
    psnr, ssim, ergas, lpips = net.validate(epoch=0, mode='train')
    assert np.isfinite([psnr, ssim, ergas]).all() and lpips != lpips
    assert (psnr, ssim, ergas) == (hist[0]['psnr'], hist[0]['ssim'], hist[0]['ergas'])
    lr_t, hr_t, _ = net._batch(test[0], test=True)
    net.generator.eval()
    with torch.no_grad():
        direct = V.quantized_metrics(E.self_ensemble(net.generator, lr_t), hr_t, 2)
        plain = V.quantized_metrics(net.generator(lr_t), hr_t, 2)
    net.generator.train()
    for name, value in (('psnr', psnr), ('ssim', ssim), ('ergas', ergas)):
        assert float(direct[name].sum()) / 2 == value, name
    assert float(plain['psnr'].sum()) / 2 != psnr                                      # and not the plain generator's numbers
    # the same seeds give the same run, bit for bit
    net2, hist2, _ = _trainer_run(tmp_path, 'b', src)
    assert (hist2[0]['loss_G'], hist2[0]['loss_D']) == (hist[0]['loss_G'], hist[0]['loss_D'])
    for a, b in zip(net.seen, net2.seen):
        assert torch.equal(a[0], b[0]) and _same_bits(a[3], b[3])
