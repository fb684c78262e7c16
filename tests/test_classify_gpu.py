"""The scene-classification evaluation on the device (sradsgan_amd/classify.py, csrc/classify.hip) against the fp64 restatement of
tests/classify_ref.py.  Bars are derived, not measured: integer and bit-exact equality where the arithmetic is exact, the fp32
dot-product bound gamma_L * sum |a b| (any order, u = 2^-24) for the dense kernels, an operation-count bound for softmax-CE, the conv
route bars of tests/test_conv_routes_gpu.py for the VGG19 layers, and tests/reduction_ref.py's yardstick (8 x stock fp32 torch, FLOOR)
for the composed training steps.  Every test prints its worst err / bound (run with -s)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import classify_ref as C
from tests import conv_emulation as E
from tests import reduction_ref as R
from tests.test_conv_routes_gpu import TAU

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _S():
    from sradsgan_amd import classify
    return classify


def _ops():
    from sradsgan_amd import ops
    return ops


# ---- channel sums, preprocess --------------------------------------------------------------------------------------------------- #
def _u8(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
    t[0] = 255                                                    # an all-255 tile: the largest sums the size allows
    return t


@pytest.mark.parametrize('size', [(32, 32), (31, 33)])
@pytest.mark.parametrize('n', [1, 5])
def test_channel_sums_are_numpy_integers(n, size):
    S = _S()
    img = _u8(n, size[0], size[1], 10 * n + size[0])
    got = S.channel_sums(img.to(DEV)).cpu().numpy()
    want = img.numpy().astype(np.int64).sum(axis=(1, 2))
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert want[0, 0] == 255 * size[0] * size[1]
    means = S.channel_means([img.to(DEV)[:1], img.to(DEV)[1:]] if n > 1 else img.to(DEV))
    assert float(np.abs(means - C.channel_means_ref(img.numpy())).max()) <= 1e-10
    if n > 1:                                                     # independent of the order of the images, bit for bit
        assert np.array_equal(means, S.channel_means(img.flip(0).to(DEV)))


@pytest.mark.parametrize('width', [32, 33])
def test_preprocess_is_the_fp32_expression_bit_for_bit(width):
    S = _S()
    img = _u8(3, 31, width, width)
    means = np.array([123.68, 116.779, 103.939], np.float64) + 0.013
    got = S.preprocess(img.to(DEV), means).cpu().numpy()
    want = C.preprocess_ref32(img.numpy(), means)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


# ---- the dense kernels ---------------------------------------------------------------------------------------------------------- #
DENSE_SHAPES = [(512, 256), (2048, 256), (32768, 256), (256, 21), (256, 3)]


def _dense_inputs(family, m, k, n, seed):
    g = torch.Generator().manual_seed(seed)
    if family == 'normal':
        x, w = torch.randn(m, k, generator=g), torch.randn(k, n, generator=g) / k ** 0.5
        b, dy = torch.randn(n, generator=g), torch.randn(m, n, generator=g)
    else:                        # all-positive operands: a dropped, doubled or mis-strided chunk moves the result far beyond gamma_L
        x, w = 0.5 + torch.rand(m, k, generator=g), (0.5 + torch.rand(k, n, generator=g)) / k
        b, dy = 0.5 + torch.rand(n, generator=g), 0.5 + torch.rand(m, n, generator=g)
        if family == 'rows':     # every row on its own scale: an aliased row is off by at least 1 / 64 of its value
            x = x * (1.0 + torch.arange(m, dtype=torch.float32)[:, None] / 64.0)
            dy = dy * (1.0 + torch.arange(m, dtype=torch.float32)[:, None] / 64.0)
    return x.to(DEV), w.to(DEV), b.to(DEV), dy.to(DEV)


def _ratio(got, ref, bound):
    r = (got.double() - ref).abs() / bound
    return float(torch.nan_to_num(r, nan=float('inf')).max())


@pytest.mark.parametrize('family', ['normal', 'positive', 'rows'])
@pytest.mark.parametrize('shape', DENSE_SHAPES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('m', [1, 21, 64])
def test_dense_kernels_against_fp64(m, shape, family):
    S, ops = _S(), _ops()
    k, n = shape
    x, w, b, dy = _dense_inputs(family, m, k, n, 100 * m + k + n)
    # forward
    y = S.dense_fwd(x, w, b)
    ref = x.double() @ w.double() + b.double()
    worst = {'fwd': _ratio(y, ref, C.dense_bound(x, w, b))}
    assert torch.equal(y, S.dense_fwd(x, w, b))                              # two calls, identical bits
    with ops.conv_math('fp32'):
        y32 = S.dense_fwd(x, w, b)
    with ops.conv_math('bf16x3'):
        assert torch.equal(y32, S.dense_fwd(x, w, b)) and torch.equal(y, y32)  # the conv arithmetic mode does not reach it
    yr = S.dense_fwd(x, w, b, relu=True)
    assert torch.equal(yr, y.clamp_min(0))
    # weight gradient
    dw, db = S.dense_wgrad(x, dy)
    worst['wgrad'] = _ratio(dw, x.double().t() @ dy.double(), C.dense_bound(x.t(), dy))
    worst['bgrad'] = _ratio(db, dy.double().sum(0), C.gamma(m) * dy.double().abs().sum(0) + 1e-45)
    dw2, db2 = S.dense_wgrad(x, dy)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    # data gradient: layer 2 into layer 1 only
    if k == 256:
        dx = S.dense_dgrad(dy, w)
        worst['dgrad'] = _ratio(dx, dy.double() @ w.double().t(), C.dense_bound(dy, w.t()))
        assert torch.equal(dx, S.dense_dgrad(dy, w))
    print('dense m=%d k=%d n=%d %s: worst err / bound %s' % (m, k, n, family, ', '.join('%s %.3g' % kv for kv in worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize('m', [21, 64])
def test_dropout_is_the_host_function_forward_and_backward(m):
    S = _S()
    k, n, c = 512, 256, 21
    x, w, b, _ = _dense_inputs('normal', m, k, n, 5)
    g = torch.Generator().manual_seed(6)
    w2, dz = torch.randn(n, c, generator=g).to(DEV), torch.randn(m, c, generator=g).to(DEV)
    y0 = S.dense_fwd(x, w, b, relu=True)                                      # eval mode: no mask, no scaling
    plain = S.dense_dgrad(dz, w2)
    masks = []
    for seed in (1, (1 << 40) + 5):
        for step in (0, 7):
            keep = torch.from_numpy(C.dropout_keep(seed, step, m, n)).to(DEV)
            masks.append(keep)
            yd = S.dense_fwd(x, w, b, relu=True, dropout=(seed, step))
            assert torch.equal(yd, torch.where(keep, 2.0 * y0, torch.zeros_like(y0)))
            dh = S.dense_dgrad(dz, w2, act=yd, dropout=(seed, step))
            assert torch.equal(dh, torch.where(keep & (y0 > 0), 2.0 * plain, torch.zeros_like(plain)))
    assert not torch.equal(masks[0], masks[1]) and not torch.equal(masks[0], masks[2])
    assert torch.equal(S.dense_dgrad(dz, w2, act=y0), torch.where(y0 > 0, plain, torch.zeros_like(plain)))


# ---- softmax cross-entropy ------------------------------------------------------------------------------------------------------ #
def _logits(family, m, c, seed):
    g = torch.Generator().manual_seed(seed)
    z = 3.0 * torch.randn(m, c, generator=g)
    if family == 'pm80':                                           # exp overflows without the max subtraction
        z = torch.where(torch.rand(m, c, generator=g) < 0.5, torch.full_like(z, 80.0), torch.full_like(z, -80.0))
        z[:, 0] = 80.0
    elif family == 'equal':
        z = torch.full((m, c), 1.25)
    elif family == 'tie':
        z[:, 0] = z[:, c - 1] = z.max(1).values + 0.5              # two equal maxima
    y = torch.randint(0, c, (m,), generator=g, dtype=torch.int32)
    return z, y


@pytest.mark.parametrize('family', ['normal', 'pm80', 'equal', 'tie'])
@pytest.mark.parametrize('c', [3, 21, 64])
@pytest.mark.parametrize('m', [1, 21, 64])
def test_softmax_ce_against_fp64(m, c, family):
    S = _S()
    z, y = _logits(family, m, c, 1000 * m + 10 * c)
    row, total, dz = S.softmax_ce(z.to(DEV), y.to(DEV))
    row, total, dz = row.cpu().double(), float(total.cpu()[0]), dz.cpu().double()
    logp = torch.log_softmax(z.double(), 1)
    onehot = F.one_hot(y.long(), c).double()
    ref_row = -(logp * onehot).sum(1)
    ref_dz = (logp.exp() - onehot) / m
    loss_b, dz_b = C.ce_bounds(z, y, 1.0 / m)
    assert bool(torch.isfinite(row).all()) and bool(torch.isfinite(dz).all())
    r_loss = float(((row - ref_row).abs() / loss_b).max())
    r_sum = abs(total - float(ref_row.sum())) / float(loss_b.sum())
    r_dz = float(((dz - ref_dz).abs() / dz_b).max())
    r_zero = float((dz.sum(1).abs() / dz_b.sum(1)).max())
    print('softmax-ce m=%d c=%d %s: err / bound loss %.3g, batch sum %.3g, dlogits %.3g, row sums %.3g' % (m, c, family, r_loss, r_sum, r_dz, r_zero))
    assert r_loss <= 1.0 and r_sum <= 1.0 and r_dz <= 1.0 and r_zero <= 1.0
    assert abs(total - float(row.sum())) <= 1e-12 * max(1.0, abs(total))      # the batch sum is the fp64 sum of the fp32 rows


def test_confusion_counts_and_first_index_ties():
    S = _S()
    m, c = 300, 21
    g = torch.Generator().manual_seed(3)
    z = torch.randn(m, c, generator=g)
    z[:, 20] = -10.0                                               # class 20 is never predicted
    z[:, 19] = -11.0                                               # neither is class 19, which also never occurs
    for r in range(0, m, 7):                                       # tied maxima at two or three places
        a, b = int(torch.randint(0, 19, (1,), generator=g)), int(torch.randint(0, 19, (1,), generator=g))
        z[r, a] = z[r, b] = 5.0
        if r % 14 == 0:
            z[r, 18] = 5.0
    z[1] = 0.5                                                     # all equal: class 0
    y = torch.randint(0, 19, (m,), generator=g, dtype=torch.int32)
    y[::11] = 20
    table = torch.zeros(c, c, dtype=torch.int32, device=DEV)
    pred = torch.cat([S.argmax_confusion(z[a:a + 64].to(DEV), y[a:a + 64].to(DEV), table) for a in range(0, m, 64)]).cpu().numpy()
    want = np.argmax(z.numpy(), axis=1)                            # numpy: the first index of the maximum
    assert np.array_equal(pred, want) and pred[1] == 0
    cm = np.zeros((c, c), np.int64)
    np.add.at(cm, (y.numpy().astype(np.int64), want), 1)
    assert np.array_equal(table.cpu().numpy().astype(np.int64), cm)
    assert cm[:, 20].sum() == 0 and cm[20].sum() > 0 and cm[19].sum() == 0
    metrics = pytest.importorskip('sklearn.metrics')
    assert np.array_equal(cm, metrics.confusion_matrix(y.numpy(), want, labels=list(range(c))))


# ---- VGG19 ---------------------------------------------------------------------------------------------------------------------- #
@pytest.fixture(scope='module')
def vgg():
    return _S().VGG19Features().to(DEV)


@pytest.fixture(scope='module')
def dataset(vgg):
    """The CPU-checked synthetic tiles, their means and their device features (default conv arithmetic), computed once."""
    S = _S()
    imgs, labels = C.synthetic_tiles()
    u8 = torch.from_numpy(imgs).to(DEV)
    means = S.channel_means(u8)
    assert float(np.abs(means - C.channel_means_ref(imgs)).max()) <= 1e-10
    feats = S.features_of(u8, vgg, means)
    return dict(imgs=imgs, labels=labels, u8=u8, means=means, feats=feats)


@pytest.fixture(scope='module')
def gains(vgg):
    """C.conv_gain of every conv of the trunk, by torchvision index, computed once (144 singular-value problems on the host)."""
    state = vgg.state_dict()
    return {i: C.conv_gain(state['features.%d.weight' % i]) for block in C.BLOCKS for i in block}


VGG_CASES = [(n, size, mode) for n in (1, 3) for size in (32, 64) for mode in ('fp32', 'bf16x3')] + [(2, 128, 'bf16x3')]


@pytest.mark.parametrize('n,size,mode', VGG_CASES)
def test_vgg19_layers_under_the_conv_route_bars(vgg, gains, n, size, mode):
    """The trunk against tests/classify_ref.py, whose BLOCKS -- not the model's own tables -- say which layer comes where.
    (1) The taps carry the torchvision indices of C.tap_sequence(), in that order.
    (2) Every conv + ReLU against the operand-rounded fp64 emulation of the layer C.BLOCKS names, with the weights the state dict
        holds under that name, on the layer's own (device) input, under the bars of tests/test_conv_routes_gpu.py; every pool
        exactly.  In the default mode a layer may run the split-bf16 route or an exact-fp32 one (short planes): it has to lie
        within the bar of one of the two emulations.  A layer's arithmetic counts as proved ('!' in the printed line) the way that
        file proves it for the close pair: the result is more than 2x nearer, in the 2-norm, to that emulation than to the other.
        The 128 x 128 case is large enough for the split-bf16 kernels to take wide layers: at least one has to be proved so.
    (3) Every pooled block output against C.vgg19_block_ref (the block of C.vgg19_ref) fed the device's previous block output, in the
        2-norm, under the per-layer bars of (2) composed over the block: a layer's own share is the norm of its element-wise bar
        (plus, where split-bf16 is allowed, the norm of the distance of that emulation from the exact fp64 layer on the same
        input), and the layers after it can lengthen it by no more than C.conv_gain of their weights.  The bar comes to 2e-4 and
        5e-4 of the output's norm for the two-conv blocks and to 0.06 - 0.18 for the four-conv ones (printed; the measured
        distance is 1e-6 - 5e-6); two layers of a block swapped move its output by 0.7 - 0.9 of its norm
        (stock fp32 torch on the host standing in for the device).
    The distance of all five outputs to C.vgg19_ref end to end is printed, not asserted: composed over 16 layers the bar says
    nothing."""
    S, ops = _S(), _ops()
    imgs, _ = C.synthetic_tiles(classes=3, per_class=1, size=size, seed=size + n)
    u8 = torch.from_numpy(imgs[:n]).to(DEV)
    x = S.preprocess(u8, [120.0, 115.0, 110.0])
    with ops.conv_math(mode):
        out, taps = vgg(x, taps=True)
    assert tuple(out.shape) == (n, size // 32, size // 32, 512) and out.is_contiguous()
    assert [i for i, _ in taps] == [i for i, _ in C.tap_sequence()]
    state = {k: v.detach() for k, v in vgg.state_dict().items()}
    ariths = ('fp32',) if mode == 'fp32' else ('bf16x3', 'fp32')
    prev, worst, routes, blocks, pooled = x.permute(0, 3, 1, 2), 0.0, [], [], []
    block_in, tap = prev, iter(taps)
    for b, block in enumerate(C.BLOCKS):
        bar = 0.0
        for i in block:
            t = next(tap)[1]
            weight, bias = state['features.%d.weight' % i], state['features.%d.bias' % i]
            ratios, refs, own = {}, {}, {}
            for arith in reversed(ariths):                          # fp32 first: its emulation is the exact fp64 layer
                ref, absref = E.conv_fwd(prev.contiguous(), weight, 1, 1, arith)
                refs[arith], absref = E.epilogue(ref, absref, bias=bias, slope=0.0)
                ratios[arith] = E.worst(t, refs[arith], absref, TAU[arith])[0]
                own[arith] = float(E.bound(refs[arith], absref, TAU[arith]).norm()) + float((refs[arith] - refs['fp32']).norm())
            bar = gains[i] * bar + max(own.values())
            arith = min(ratios, key=ratios.get)
            assert ratios[arith] <= 1.0, 'features.%d (%s): err / bound %s' % (i, tuple(t.shape), ratios)
            proved = ''
            if len(ariths) == 2:
                dist = {a: E.l2_dist(t, refs[a]) for a in ariths}
                mine = min(dist, key=dist.get)
                other = 'fp32' if mine == 'bf16x3' else 'bf16x3'
                if ratios[mine] <= 1.0 and dist[other] > 2 * max(dist[mine], 1e-300):
                    arith, proved = mine, '!'
            routes.append('%d:%s%s %.2f' % (i, arith, proved, ratios[arith]))
            worst = max(worst, ratios[arith])
            prev = t
        t = next(tap)[1]
        assert torch.equal(t, F.max_pool2d(prev, 2, 2)), 'pool after features.%d' % block[-1]
        ref = C.vgg19_block_ref(block_in, state, b)
        assert tuple(t.shape) == tuple(ref.shape) and bool(torch.isfinite(t).all())
        dist, scale = E.l2_dist(t, ref), float(ref.norm())
        assert dist <= bar, 'block %d pooled output: |diff| %.3e, bar %.3e (|ref| %.3e)' % (b + 1, dist, bar, scale)
        blocks.append('%d: %.2g (err %.1e, bar %.1e of |ref|)' % (b + 1, dist / bar, dist / scale, bar / scale))
        pooled.append(t)
        prev = block_in = t
    print('vgg19 n=%d %dx%d %s: worst err / bound %.3f  [%s]' % (n, size, size, mode, worst, ' '.join(routes)))
    print('   pooled block outputs against the restatement fed the previous device output, err / bound  ' + '; '.join(blocks))
    if size >= 128:
        assert any(':bf16x3!' in r for r in routes), routes
    last = taps[-1][1]                                              # Flatten order is (h, w, c)
    assert torch.equal(out.reshape(n, -1), last.permute(0, 2, 3, 1).reshape(n, -1))
    flat = out.reshape(n, -1)
    hh = size // 32
    assert float(flat[n - 1, ((hh - 1) * hh + 0) * 512 + 7]) == float(last[n - 1, 7, hh - 1, 0])
    whole = C.vgg19_ref(x.cpu().numpy(), {k: v.cpu() for k, v in state.items()})
    print('   all five against the fp64 restatement end to end, max |diff| / max |ref|: '
          + ' '.join('%.1e' % C.err(t.permute(0, 2, 3, 1), w) for t, w in zip(pooled, whole)))


# ---- training ------------------------------------------------------------------------------------------------------------------- #
def test_head_training_steps_against_fp64(dataset):
    """8 optimiser steps at m = 20 on device-extracted features: the loss and w1, b1, w2, b2 after every step against the fp64
    restatement fed the same batches and the same masks.  Bar per tensor and step: reduction_ref.bound of the error the same
    restatement makes in stock fp32 torch on the CPU (dense and Adam roundings composed step by step), as the Adam test does."""
    S = _S()
    X, y = dataset['feats'], torch.from_numpy(dataset['labels'])
    seed = 21
    head = S.SceneClassifier(3, (1, 1, 512), DEV, seed=seed)
    ref64 = C.HeadRef(S.initial_kernels(512, 3, seed), 3, torch.float64)
    ref32 = C.HeadRef(S.initial_kernels(512, 3, seed), 3, torch.float32)
    Xc = X.cpu()
    order = np.random.RandomState(2).permutation(60)
    worst, dist = 0.0, 0.0
    for step in range(8):
        idx = torch.from_numpy(order[20 * (step % 3):20 * (step % 3) + 20])
        xb, yb = Xc[idx], y[idx]
        total, _ = head.train_batch(xb.to(DEV).contiguous(), yb.to(torch.int32).to(DEV), seed)
        l64, _ = ref64.train_batch(xb, yb, seed)
        l32, _ = ref32.train_batch(xb, yb, seed)
        loss = float(total.cpu()[0]) / 20
        bar = R.bound(abs(l32 - l64) / abs(l64))
        r = abs(loss - l64) / abs(l64) / bar
        assert r <= 1.0, 'step %d loss %.9g vs %.9g: err / bound %.3g' % (step + 1, loss, l64, r)
        worst = max(worst, r)
        for name, got in head.parameters().items():
            e, bar = C.err(got, ref64.p[name]), R.bound(C.err(ref32.p[name], ref64.p[name]))
            assert e <= bar, 'step %d %s: err %.3e, bar %.3e' % (step + 1, name, e, bar)
            worst, dist = max(worst, e / bar), max(dist, e)
    print('head training, 8 steps at m = 20: worst err / bound %.3f, largest parameter distance max|d| / max|ref| %.3e' % (worst, dist))


def _fit_run(S, dataset, seed):
    X, labels = dataset['feats'], dataset['labels']
    tr, va, te = S.split_indices(labels, C.SPLIT_SEED)
    head = S.SceneClassifier(3, (1, 1, 512), DEV)
    hist, best = head.fit(X[tr], labels[tr], X[va], labels[va], epochs=C.FIT_EPOCHS, batch_size=C.FIT_BATCH, seed=seed)
    head.refit(torch.cat([X[tr], X[va]]), np.concatenate([labels[tr], labels[va]]), best, batch_size=C.FIT_BATCH, seed=seed)
    return head, hist, best, head.evaluate(X[te], labels[te]), te


def test_fit_refit_evaluate_end_to_end(dataset):
    S = _S()
    head, hist, best, res, te = _fit_run(S, dataset, C.FIT_SEED)
    print('end to end: best epoch %d, val_loss %.4f -> %.4f, accuracy %.3f' % (best, hist['val_loss'][0], hist['val_loss'][-1], res['accuracy']))
    assert len(hist['loss']) == C.FIT_EPOCHS == len(hist['val_loss']) and best == int(np.argmin(hist['val_loss'])) + 1
    assert res['accuracy'] == 1.0
    assert res['confusion'].dtype == np.int64 and np.array_equal(res['confusion'], np.diag([5, 5, 5]))
    assert np.array_equal(res['pred'], dataset['labels'][te])
    assert all(row['f1'] == 1.0 and row['support'] == 5 for row in res['report']['classes'])
    assert np.array_equal(head.predict(dataset['feats'][te]).cpu().numpy(), res['pred'])
    head2, hist2, best2, res2, _ = _fit_run(S, dataset, C.FIT_SEED)                    # the same seed: the same bits
    assert hist2 == hist and best2 == best
    assert torch.equal(head2.flat_p, head.flat_p) and np.array_equal(res2['confusion'], res['confusion'])


# ---- classify_sr ---------------------------------------------------------------------------------------------------------------- #
def _generators(tmp_path):
    from sradsgan_amd import trainer as T
    from sradsgan_amd.model.edsr import Net
    args = T.default_args(scale_factor=2, save_dir=str(tmp_path / 'out'), crop_size=64, hr_height=64, hr_width=64, test_crop_size=32,
                          n_residual_blocks=1, n_basic_blocks=1)
    net = T.SRADSGAN(args)
    torch.manual_seed(3)
    g = net._new_generator()
    g.apply(T.weights_init_normal)
    path = os.path.join(str(tmp_path), 'g.pkl')
    torch.save(g.state_dict(), path)
    torch.manual_seed(4)
    edsr = Net(3, 256, 1, upscale_factor=2)
    return net, g.to(DEV), path, edsr.to(DEV)


def test_classify_sr_equals_the_separate_steps(vgg, tmp_path):
    from sradsgan_amd import data as sdata
    S = _S()
    imgs, labels = C.synthetic_tiles(classes=3, per_class=2, size=64, seed=9)
    hr = torch.from_numpy(imgs).to(DEV)
    means = S.channel_means(hr)
    head = S.SceneClassifier(3, (2, 2, 512), DEV, seed=2)
    net, sradsgan, path, edsr = _generators(tmp_path)
    for name, gen in (('sradsgan', sradsgan), ('edsr', edsr)):
        batches = [hr[:4], hr[4:]]
        res = S.classify_sr(gen, 2, batches, labels, vgg, head, means, mode='sr', return_tiles=True)
        gen.eval()
        parts = []
        for b in batches:                                           # the same steps with the existing pieces, batch by batch
            lr = sdata.resize_u8(b, 32, 32, 'bicubic')
            with torch.no_grad():
                sr = gen(sdata.to_tensor(lr))
            parts.append((sr * 255.0).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous())      # save_img1
        u8 = torch.cat(parts)
        assert tuple(u8.shape) == (6, 64, 64, 3)
        assert torch.equal(torch.cat(res['tiles']), u8), name
        direct = head.predict(S.features_of(u8, vgg, means)).cpu().numpy()
        assert np.array_equal(res['pred'], direct), name
        assert res['confusion'].sum() == 6 and res['confusion'].dtype == np.int64
        assert abs(res['accuracy'] - float((direct == labels).mean())) <= 1e-15
    bic = S.classify_sr(sradsgan, 2, hr, labels, vgg, head, means, mode='bicubic', return_tiles=True)
    assert torch.equal(bic['tiles'][0], sdata.resize_u8(sdata.resize_u8(hr, 32, 32, 'bicubic'), 64, 64, 'bicubic'))
    low = S.classify_sr(sradsgan, 2, hr, labels, vgg, head, means, mode='lr', return_tiles=True)
    assert tuple(low['tiles'][0].shape) == (6, 32, 32, 3) and low['confusion'].sum() == 6     # resized to 64 x 64 (nearest) for the head
    with pytest.raises(ValueError):
        S.classify_sr(sradsgan, 2, hr, labels, vgg, head, means, mode='nearest')
    from PIL import Image                                           # the folder form: class sub-directories of image files
    for k, im in enumerate(imgs):
        os.makedirs(str(tmp_path / 'set' / ('class%d' % labels[k])), exist_ok=True)
        Image.fromarray(im).save(str(tmp_path / 'set' / ('class%d' % labels[k]) / ('tile%02d.png' % k)))
    folder = S.classify_folder(str(tmp_path / 'set'), vgg, head, means)
    assert folder['class_names'] == ['class0', 'class1', 'class2']
    assert np.array_equal(folder['pred'], head.predict(S.features_of(hr, vgg, means)).cpu().numpy())
    assert np.array_equal(folder['confusion'], head.evaluate(S.features_of(hr, vgg, means), labels)['confusion'])
    want = S.classify_sr(sradsgan, 2, hr, labels, vgg, head, means)
    got = net.mfe_classify_scenes(hr, labels, vgg, head, means, modelpath=path)
    assert sorted(got) == sorted(want) == ['accuracy', 'confusion', 'pred', 'report']
    assert got['accuracy'] == want['accuracy'] and got['report'] == want['report']
    assert np.array_equal(got['confusion'], want['confusion']) and np.array_equal(got['pred'], want['pred'])
