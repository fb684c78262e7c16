"""CPU checks of the scene-classification evaluation: the fp64 restatement the GPU tests compare against (tests/classify_ref.py) is
checked against autograd, the host dropout function against its published test vector and its statistics, the split and the report
against their definitions / sklearn, and the synthetic data set of the GPU tests is fixed here so the GPU accuracy test cannot pass
or fail by a coin flip."""
import numpy as np
import pytest
import torch

from tests import classify_ref as C


def _head(k, c, seed):
    from sradsgan_amd import classify as S
    return S.initial_kernels(k, c, seed)


def test_closed_form_gradients_agree_with_fp64_autograd():
    g = torch.Generator().manual_seed(4)
    m, k, c = 7, 24, 5
    x = torch.randn(m, k, generator=g, dtype=torch.float64)
    y = torch.randint(0, c, (m,), generator=g)
    p = {'w1': 0.3 * torch.randn(k, C.HIDDEN, generator=g, dtype=torch.float64), 'b1': 0.1 * torch.randn(C.HIDDEN, generator=g, dtype=torch.float64),
         'w2': 0.3 * torch.randn(C.HIDDEN, c, generator=g, dtype=torch.float64), 'b2': 0.1 * torch.randn(c, generator=g, dtype=torch.float64)}
    keep = torch.from_numpy(C.dropout_keep(3, 9, m, C.HIDDEN))
    for mask in (None, keep):
        q = {n: t.clone().requires_grad_() for n, t in p.items()}
        pre, h, z = C.head_forward(x, q, mask)
        loss = torch.nn.functional.cross_entropy(z, y)
        auto = torch.autograd.grad(loss, [q[n] for n in ('w1', 'b1', 'w2', 'b2')])
        pre, h, z = C.head_forward(x, p, mask)
        mine, dz = C.ce_ref(z, y)
        grads = C.head_backward(x, p, pre, h, dz, mask)
        assert abs(float(mine) - float(loss.detach())) <= 1e-14 * max(1.0, abs(float(loss.detach())))
        for n, a in zip(('w1', 'b1', 'w2', 'b2'), auto):
            assert float((grads[n] - a).abs().max()) <= 1e-13 * max(1.0, float(a.abs().max())), n


def test_adam_restatement_is_torch_adam():
    g = torch.Generator().manual_seed(8)
    p0 = torch.randn(50, generator=g, dtype=torch.float64)
    grads = [torch.randn(50, generator=g, dtype=torch.float64) * s for s in (1.0, 1e-3, 1.0)]
    q = p0.clone().requires_grad_()
    opt = torch.optim.Adam([q], lr=C.LR, betas=(C.B1, C.B2), eps=C.EPS)
    p, st = {'a': p0.clone()}, {'m': {'a': torch.zeros(50, dtype=torch.float64)}, 'v': {'a': torch.zeros(50, dtype=torch.float64)}}
    for t, gr in enumerate(grads, 1):
        q.grad = gr.clone()
        opt.step()
        C.adam_update(p, {'a': gr}, st, t)
        assert float((p['a'] - q.detach()).abs().max()) <= 1e-15


def test_host_dropout_function():
    # Random123's known-answer vector for philox4x32-10 with a zero counter and a zero key
    assert int(C.philox_first(np.zeros(1, np.uint64), 0, 0)[0]) == 0x6627E8D5
    a = C.dropout_keep(7, 3, 64, 256)
    assert a.dtype == np.bool_ and a.shape == (64, 256)
    assert np.array_equal(a, C.dropout_keep(7, 3, 64, 256))                           # a pure function
    kept = int(a.sum())
    assert abs(kept - 8192) <= 384, kept                                              # 6 binomial sigma of 16384 fair draws
    for other in (C.dropout_keep(7, 4, 64, 256), C.dropout_keep(8, 3, 64, 256)):      # step and seed both matter
        assert 0.4 < float((other != a).mean()) < 0.6
    assert np.array_equal(C.dropout_keep(7, 3, 21, 256), a[:21])                      # the element index is row * 256 + column


def test_split_indices_are_65_10_25_per_class_and_disjoint():
    from sradsgan_amd import classify as S
    labels = np.repeat(np.arange(21), 100)
    np.random.RandomState(0).shuffle(labels)
    tr, va, te = S.split_indices(labels, seed=3)
    for part, count in ((tr, 65), (va, 10), (te, 25)):
        assert np.array_equal(np.bincount(labels[part], minlength=21), np.full(21, count))
    allidx = np.concatenate([tr, va, te])
    assert len(np.unique(allidx)) == 2100 == len(allidx)
    again = S.split_indices(labels, seed=3)
    assert all(np.array_equal(a, b) for a, b in zip((tr, va, te), again))
    assert not np.array_equal(S.split_indices(labels, seed=4)[0], tr)


def test_report_equals_sklearn():
    metrics = pytest.importorskip('sklearn.metrics')
    from sradsgan_amd import classify as S
    rng = np.random.RandomState(1)
    c = 6
    y_true = rng.randint(0, c, 400)
    y_pred = np.where(rng.rand(400) < 0.7, y_true, rng.randint(0, c, 400))
    y_pred[y_pred == 4] = 1                                                           # class 4 is never predicted
    y_true[y_true == 5] = 0                                                           # class 5 never occurs ...
    y_pred[y_pred == 5] = 2                                                           # ... and is never predicted
    cm = np.zeros((c, c), np.int64)
    np.add.at(cm, (y_true, y_pred), 1)
    assert np.array_equal(cm, metrics.confusion_matrix(y_true, y_pred, labels=list(range(c))))
    rep = S.report_from_confusion(cm)
    pr, rc, f1, sup = metrics.precision_recall_fscore_support(y_true, y_pred, labels=list(range(c)), zero_division=0)
    for i in range(c):
        row = rep['classes'][i]
        assert row['support'] == sup[i]
        assert abs(row['precision'] - pr[i]) <= 1e-15 and abs(row['recall'] - rc[i]) <= 1e-15 and abs(row['f1'] - f1[i]) <= 1e-15
    assert rep['classes'][4]['precision'] == 0.0 and rep['classes'][4]['support'] > 0
    assert abs(rep['accuracy'] - metrics.accuracy_score(y_true, y_pred)) <= 1e-15
    for avg in ('macro', 'weighted'):
        want = metrics.precision_recall_fscore_support(y_true, y_pred, labels=list(range(c)), average=avg, zero_division=0)
        got = rep[avg + ' avg']
        assert abs(got['precision'] - want[0]) <= 1e-15 and abs(got['recall'] - want[1]) <= 1e-15 and abs(got['f1'] - want[2]) <= 1e-15


def test_channel_means_and_preprocess_restatements():
    imgs, _ = C.synthetic_tiles()
    means = C.channel_means_ref(imgs)
    assert means.shape == (3,) and np.allclose(means, imgs.reshape(-1, 3).astype(np.float64).mean(0), rtol=0, atol=1e-9)
    x = C.preprocess_ref32(imgs[:2], means)
    assert x.dtype == np.float32 and float(np.abs(x - (imgs[:2] - means) / 255.0).max()) < 1e-6


def test_synthetic_data_set_is_separable_with_margin():
    """The data set of the GPU end-to-end test, fixed here: on the deterministic-init VGG19 the fp64 restatement of fit + refit
    reaches accuracy 1.0 on the held-out quarter, and the smallest gap between the top two logits exceeds 1e-2 -- five orders of
    magnitude above what fp32 arithmetic moves a logit by."""
    from sradsgan_amd import classify as S
    imgs, labels = C.synthetic_tiles()
    assert imgs.shape == (60, 32, 32, 3) and imgs.dtype == np.uint8
    assert np.array_equal(imgs, C.synthetic_tiles()[0])
    means = C.channel_means_ref(imgs)
    state = {k: v.detach() for k, v in S.VGG19Features().state_dict().items()}
    feats = C.vgg19_ref(C.preprocess_ref32(imgs, means), state)[-1].reshape(60, -1)
    assert feats.shape == (60, 512)
    tr, va, te = S.split_indices(labels, C.SPLIT_SEED)
    assert (len(tr), len(va), len(te)) == (39, 6, 15)
    y = torch.from_numpy(labels)
    ref = C.HeadRef(_head(512, 3, C.FIT_SEED), 3)
    best = ref.fit_refit(_head(512, 3, C.FIT_SEED), _head(512, 3, C.FIT_SEED + 1), feats[tr], y[tr], feats[va], y[va], C.FIT_EPOCHS,
                         C.FIT_BATCH, C.FIT_SEED)
    z = ref.logits(feats[te])
    top = z.topk(2, dim=1).values
    gap = float((top[:, 0] - top[:, 1]).min())
    acc = float((z.argmax(1) == y[te]).double().mean())
    print('synthetic set: best epoch %d, held-out accuracy %.3f, smallest top-2 logit gap %.4f' % (best, acc, gap))
    assert acc == 1.0
    assert gap > 1e-2


def test_entry_points_refuse_bad_arguments_and_there_is_no_cpu_fallback():
    import __graft_entry__ as ge
    from sradsgan_amd import _hip, classify as S
    import os
    if not os.path.exists(_hip.LIB_PATH):
        ge.build()
    lib = _hip.lib()
    assert lib.srhip_cls_dense_chunks(32768) == 64 and lib.srhip_cls_dense_chunks(256) == 1 and lib.srhip_cls_dense_chunks(0) == 0
    assert lib.srhip_cls_channel_sums_workspace(5, 31, 33) >= 5 * 4 * 8 and lib.srhip_cls_channel_sums_workspace(0, 1, 1) == 0
    assert lib.srhip_cls_dense_fwd(None, None, None, None, None, 0, 1, 8, 1, 0, 0, 0, 0, None) == -1
    assert b'null tensor' in lib.srhip_last_error()
    assert lib.srhip_cls_softmax_ce_fwd_bwd(None, None, None, None, None, 1, 3, 1.0, None) == -1
    assert lib.srhip_cls_confusion(None, None, None, None, 1, 3, None) == -1
    u8 = torch.zeros(1, 32, 32, 3, dtype=torch.uint8)
    for call in (lambda: S.preprocess(u8, [0.0, 0.0, 0.0]), lambda: S.channel_means(u8),
                 lambda: S.SceneClassifier(3, (1, 1, 512), device='cpu'), lambda: S.VGG19Features()(torch.zeros(1, 32, 32, 3)),
                 lambda: S.dense_fwd(torch.zeros(2, 8), torch.zeros(8, 4))):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()
    with pytest.raises(ValueError):
        S.VGG19Features()(torch.zeros(1, 33, 32, 3))
    with pytest.raises(KeyError):
        S.VGG19Features().load_torchvision_vgg19({})
    sd = {'features.%d.%s' % (i, leaf): torch.full(shape, float(i)) for i, (cin, cout) in S.CONVS.items()
          for leaf, shape in (('weight', (cout, cin, 3, 3)), ('bias', (cout,)))}
    net = S.VGG19Features()
    assert len(net.load_torchvision_vgg19(dict(sd, **{'classifier.0.weight': torch.zeros(1)}))) == 32
    assert float(net.features[34].weight[0, 0, 0, 0]) == 34.0 and float(net.features[0].bias[5]) == 0.0
