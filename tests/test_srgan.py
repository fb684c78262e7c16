"""SRGAN: the oracle against vectors recorded from the reference's model/srgan.py classes (CPU),
and the HIP mirror against the oracle and the same vectors (GPU)."""
import os

import numpy as np
import pytest
import torch

from oracle import sradsgan_ref as O
from oracle import srgan_ref as S
from tests.parity_util import sibling_grad_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['loss_G', 'loss_D', 'pixel', 'content', 'loss_gan', 'loss_real', 'loss_fake']


def _golden(name):
    return np.load(os.path.join(ROOT, 'tests', 'golden', name + '.npz'))


def _gen_case(net, scale, device='cpu', dtype=torch.float32):
    x = O.det_fill('srgan.x.%d' % scale, (2, 3, 12, 10), 0.5, 0.5).to(device, dtype)
    tgt = O.det_fill('srgan.t.%d' % scale, (2, 3, 12 * scale, 10 * scale), 0.5, 0.5).to(device, dtype)
    net.zero_grad()
    y = net(x)
    loss = torch.nn.functional.mse_loss(y, tgt)
    loss.backward()
    return y, loss


def _check_grads_and_buffers(net, g, rtol):
    seen = 0
    for k, p in net.named_parameters():
        key = 'grad__' + k.replace('.', '__')
        if key in g:
            d = O.digest(p.grad)
            assert np.abs(d - g[key]).max() <= rtol * max(1.0, np.abs(g[key]).max()), k
            seen += 1
    assert seen >= 20
    for k, b in net.named_buffers():
        ref = g['buf__' + k.replace('.', '__')]
        assert np.abs(O.digest(b.float()) - ref).max() <= rtol * max(1.0, np.abs(ref).max()), k


@pytest.mark.parametrize('scale', [2, 3, 4])
def test_oracle_generator_matches_reference_vectors(scale):
    g = _golden('srgan_x%d' % scale)
    net = S.GeneratorResNet(3, 3, n_residual_blocks=2, upscale_factor=scale)
    O.det_init_(net, prefix='S.')
    assert sorted(net.state_dict().keys()) == list(g['keys'])
    y, loss = _gen_case(net, scale)
    assert np.abs(y.detach().numpy() - g['y']).max() < 2e-6 and abs(float(loss.detach()) - float(g["loss"])) < 1e-6
    _check_grads_and_buffers(net, g, 1e-5)


def _step_models(mod_g, mod_d, fx):
    G = mod_g(3, 3, n_residual_blocks=2, upscale_factor=4)
    D = mod_d()
    return G, D, fx()


def _run_steps(G, D, Fx, step, device='cpu'):
    for p in Fx.parameters():
        p.requires_grad_(False)
    opt_G = torch.optim.Adam(G.parameters(), lr=2e-4, betas=(0.9, 0.999))
    opt_D = torch.optim.Adam(D.parameters(), lr=2e-4, betas=(0.9, 0.999))
    rows = []
    for it in range(2):
        lr_img = O.det_fill('srgan.step.lr.%d' % it, (4, 3, 16, 16), 0.5, 0.5).to(device)
        hr_img = O.det_fill('srgan.step.hr.%d' % it, (4, 3, 64, 64), 0.5, 0.5).to(device)
        out = step(G, D, Fx, opt_G, opt_D, lr_img, hr_img)
        rows.append([float(out[n]) for n in NAMES])
    return np.array(rows)


def _check_step_weights(G, D, g, rtol, adam_bound=None):
    """adam_bound=None: element-wise at rtol (oracle vs reference: same arithmetic).  Otherwise the criterion of
    tests/parity_util.py: Adam turns a gradient whose sign differs by roundoff into a full +-lr step, so weights after
    k iterations are only bounded by 2*lr*k element-wise; the bulk (median) must still agree closely."""
    gs, ds = G.state_dict(), D.state_dict()
    for key in g.files:
        if key.startswith('G__') or (key.startswith('D__') and key != 'D__bn_running_var'):
            sd = gs if key[0] == 'G' else ds
            t = sd[key[3:].replace('__', '.')].float().cpu()
            d = O.digest(t)
            if adam_bound is None:
                n = d.size - 2 if t.numel() > 4096 else d.size
                tol = rtol * max(1.0, np.abs(g[key]).max())
                assert np.abs(d[:n] - g[key][:n]).max() <= tol, key
                # the digest's [sum, l2] tail adds up every element, those whose gradient sign is roundoff included: Adam moves
                # each of them by +-lr per step on any two CPUs, so the tail is held to one such element's 2 * lr * iterations
                assert np.abs(d[n:] - g[key][n:]).max(initial=0.0) <= max(tol, 2 * 2e-4 * 2), key
            else:
                n = d.size - 2 if t.numel() > 4096 else d.size            # drop the digest's [sum, l2] tail
                dev = np.abs(d[:n] - g[key][:n])
                assert dev.max() <= adam_bound and np.median(dev) <= 2e-5, (key, dev.max(), np.median(dev))
    d = O.digest(ds['model.3.running_var'].cpu())
    assert np.abs(d - g['D__bn_running_var']).max() <= rtol * max(1.0, np.abs(g['D__bn_running_var']).max())


def test_oracle_training_iterations_match_reference_vectors():
    g = _golden('srgan_step')
    assert list(g['names']) == NAMES
    G, D, Fx = _step_models(S.GeneratorResNet, S.Discriminator, O.FeatureExtractor)
    assert sorted(D.state_dict().keys()) == list(g['keys_D'])
    O.det_init_(G, prefix='S.')
    O.det_init_(D, prefix='SD.')
    O.det_init_(Fx, prefix='V.')
    rows = _run_steps(G, D, Fx, S.train_step)
    dev = np.abs(rows - g['scalars'])
    # iteration 1 runs on the recorded initial weights: the reference's arithmetic to roundoff.  Iteration 2 runs on weights
    # after one Adam step, which turns every gradient whose sign is roundoff into a +-lr step whose direction follows the CPU's
    # summation order (thread count, the vendor's BLAS / oneDNN kernels): measured up to 7e-7 across 1-16 threads on the
    # recording CPU, 2.3e-6 on an AMD EPYC host.
    assert dev[0].max() < 2e-6, dev
    assert dev[1].max() < 5e-6, dev
    _check_step_weights(G, D, g, 1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize('scale', [2, 3, 4])
def test_hip_generator_matches_oracle_and_reference_vectors(scale):
    from sradsgan_amd.model import srgan as H
    dev = torch.device('cuda:0')
    g = _golden('srgan_x%d' % scale)
    ref = S.GeneratorResNet(3, 3, n_residual_blocks=2, upscale_factor=scale)
    O.det_init_(ref, prefix='S.')
    net = H.GeneratorResNet(3, 3, n_residual_blocks=2, upscale_factor=scale)
    assert sorted(net.state_dict().keys()) == list(g['keys'])
    net.load_state_dict(ref.state_dict(), strict=True)
    net = net.to(dev)
    y, loss = _gen_case(net, scale, dev)
    assert float((y.cpu() - torch.from_numpy(g['y'])).abs().max()) < 1e-4          # vs the reference itself
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-4
    # gradients: tests/parity_util.sibling_grad_check (reference vectors OR an fp64 oracle run at 1e-3; the wiring
    # bound only where the fp32 oracle itself shows a pre-activation within roundoff of a ReLU kink -- x3 has one at
    # 2e-6 and the device takes the other branch there: one flipped element of ~1e5 moves every upstream gradient by
    # ~1/sqrt(#elements) = 3e-3, the tied upsampler weight by 3e-2).
    ref64 = S.GeneratorResNet(3, 3, n_residual_blocks=2, upscale_factor=scale)
    O.det_init_(ref64, prefix='S.')
    rep = sibling_grad_check(net, g, ref, ref64.double(), lambda m, d, dt: _gen_case(m, scale, d, dt), tie_eps=5e-6)
    print('x%d gradient report: %s' % (scale, rep))
    for k, b in net.named_buffers():                                     # BatchNorm running statistics
        want = g['buf__' + k.replace('.', '__')]
        assert np.abs(O.digest(b.float()) - want).max() <= 1e-3 * max(1.0, np.abs(want).max()), k
    # eval(): running statistics, against the oracle in eval()
    ref.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()})
    ref.eval(), net.eval()
    x = O.det_fill('srgan.x.%d' % scale, (2, 3, 12, 10), 0.5, 0.5)
    with torch.no_grad():
        assert float((net(x.to(dev)).cpu() - ref(x)).abs().max()) < 1e-4


@pytest.mark.gpu
def test_hip_training_iterations_match_reference_vectors():
    from sradsgan_amd.model import srgan as H
    dev = torch.device('cuda:0')
    g = _golden('srgan_step')
    refs = _step_models(S.GeneratorResNet, S.Discriminator, O.FeatureExtractor)
    O.det_init_(refs[0], prefix='S.')
    O.det_init_(refs[1], prefix='SD.')
    O.det_init_(refs[2], prefix='V.')
    G, D, Fx = _step_models(H.GeneratorResNet, H.Discriminator, H.FeatureExtractor)
    assert sorted(D.state_dict().keys()) == list(g['keys_D'])
    for m, r in zip((G, D, Fx), refs):
        m.load_state_dict(r.state_dict(), strict=True)
        m.to(dev)
    rows = _run_steps(G, D, Fx, H.train_step, dev)
    err = np.abs(rows - g['scalars']) / np.maximum(1.0, np.abs(g['scalars']))
    assert err.max() < 1e-3, (err.max(), rows, g['scalars'])
    _check_step_weights(G, D, g, 2e-3, adam_bound=2 * 2e-4 * 2)
