"""CPU-side checks behind tests/test_reductions_gpu.py: the closed-form fp64 BatchNorm references against fp64 autograd, the input
generators against the properties the GPU tests rely on, and the argument refusals of the reduction entry points (SRHIP_REQUIRE
fires before any launch, so they need no device)."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from tests import reduction_ref as R

EPS = 1e-5


@pytest.mark.parametrize('slope', [0.2, None])
@pytest.mark.parametrize('family,rows,c', [('normal', 65, 12), ('corner10', 130, 8), ('constant_channel', 63, 4), ('gamma_signs', 75, 16),
                                           ('normal', 1, 4), ('normal', 2, 4)])
def test_closed_form_batch_norm_references_match_fp64_autograd(family, rows, c, slope):
    """mean / invstd / y / running statistics, (dx, dgamma, dbeta) with an addend, and (g_dy, g_x, g_gamma) of the penalty pattern
    of test_conv_gpu.py (first-order backward with create_graph, then the backward of a functional of dx) against fp64 autograd of
    F.leaky_relu(batch_norm(...)); the mask is the fp64 forward's."""
    t = R.bn_inputs(family, rows, c)
    a = R.bn_autograd(t['x'], t['gamma'], t['beta'], t['dy'], t['u'], EPS, slope, torch.float64, addend=t['addend'],
                      running_mean=t['running_mean'], running_var=t['running_var'])
    f = R.bn_fwd_ref(t['x'], t['gamma'], t['beta'], t['running_mean'], t['running_var'], EPS, 0.1, slope)
    keys = ['y', 'mean', 'invstd', 'running_mean'] + (['running_var'] if rows > 1 else [])   # rows = 1: torch's unbiased variance is NaN
    for k in keys:
        assert R.err(f[k], a[k]) < 1e-12, k
    if rows == 1:
        assert R.err(f['running_var'], 0.9 * t['running_var'].double()) < 1e-12     # biased variance of one row: 0
        return                                       # (torch refuses / NaNs the rest at one value per channel)
    mask = a['mask']
    for k, v in zip(('dx', 'dgamma', 'dbeta'), R.bn_bwd_ref(t['dy'], t['x'], t['gamma'], mask, EPS, slope, t['addend'])):
        assert R.err(v, a[k]) < 1e-11, k
    for k, v in zip(('g_dy', 'g_x', 'g_gamma'), R.bn_bwd2_ref(t['u'], t['dy'], t['x'], t['gamma'], mask, EPS, slope)):
        assert R.err(v, a[k]) < 1e-11, k


def test_second_order_reference_matches_the_gradient_penalty_graph():
    """The pattern itself: pen = mean((||gx||_2 over channels - 1)^2) with gx = d<y, dy>/dx under create_graph; its gradient at x
    through the first-order node is bn_bwd2_ref's g_x for the cotangent u = d pen / d gx."""
    n, c, h, w = 2, 8, 5, 3
    t = R.bn_inputs('normal', n * h * w, c, seed=3)
    x4 = t['x'].double().view(n, h, w, c).permute(0, 3, 1, 2).requires_grad_()
    dy4 = t['dy'].double().view(n, h, w, c).permute(0, 3, 1, 2)
    gamma = t['gamma'].double().requires_grad_()
    y = F.leaky_relu(F.batch_norm(x4, None, None, gamma, t['beta'].double(), True, 0.1, EPS), 0.2)
    (gx,) = torch.autograd.grad(y, x4, dy4, create_graph=True)
    pen = ((gx.norm(2, 1) - 1) ** 2).mean()
    u4, = torch.autograd.grad(pen, gx, retain_graph=True)
    want_x, want_gamma = torch.autograd.grad(pen, [x4, gamma])
    flat = lambda v: v.permute(0, 2, 3, 1).reshape(-1, c)
    _, g_x, g_gamma = R.bn_bwd2_ref(flat(u4), t['dy'], t['x'], t['gamma'], flat(y) > 0, EPS, 0.2)
    assert R.err(g_x, flat(want_x)) < 1e-11 and R.err(g_gamma, want_gamma) < 1e-11


@pytest.mark.parametrize('rows,c', [(4097, 64), (65, 192)])
def test_batch_norm_input_families_have_their_stated_property(rows, c):
    x = R.bn_inputs('constant_channel', rows, c)['x']
    assert float(x[:, R.CONSTANT_CHANNEL].double().var(unbiased=False)) == 0.0
    assert float(x[:, 0].var()) > 0.5
    for fam, level in (('corner3', 3.0), ('corner10', 10.0)):
        x = R.bn_inputs(fam, rows, c)['x']
        assert float(x[0].abs().max()) == 0.0
        assert float((x[1:] - level).abs().max()) <= 0.05 + 1e-6 and float(x[1:].std()) > 0.02
    x = R.bn_inputs('mean100', rows, c)['x'].double()
    assert abs(float(x.mean()) - 100) < 1e-3 and 0.008 < float(x.std()) < 0.012
    g = R.bn_inputs('gamma_signs', rows, c)['gamma']
    assert float(g[R.GAMMA_NEGATIVE]) < 0 and float(g[R.GAMMA_ZERO]) == 0.0


@pytest.mark.parametrize('count', [5, 1023, 1048581])
def test_loss_inputs_hit_the_kinks_exactly(count):
    a, b = R.loss_inputs(count)
    d = a - b                                       # fp32, as the kernel forms it
    assert int((d == 0).sum()) >= 1 and int((d == 1).sum()) >= 1 and int((d == -1).sum()) >= 1
    assert float(d[count - 1]) == -1.0              # ... one of them in the scalar tail
    assert int((d.abs() < 1).sum()) >= 1 and (count < 100 or int((d.abs() > 1).sum()) > count // 10)
    s = R.scalar_target_inputs(count, 1.0) - 1.0
    assert int((s == 0).sum()) >= 1 and int((s == 1).sum()) >= 1 and int((s == -1).sum()) >= 1


@pytest.mark.parametrize('npix', [255, 262147])
@pytest.mark.parametrize('c', [1, 3, 4])
def test_gradient_penalty_inputs_contain_a_zero_norm_pixel(npix, c):
    g = R.gp_inputs(npix, c)
    nrm = g.pow(2).sum(1).sqrt()
    assert float(nrm[npix - 1]) == 0.0 and int((nrm == 0).sum()) == 1
    assert float(nrm.min()) == 0.0 and float(nrm.max()) > 1.0 > float(nrm[:-1].min())
    _, dg = R.gp_ref(g, 1.0)
    assert bool(torch.isfinite(dg).all()) and float(dg[npix - 1].abs().max()) == 0.0


def test_adam_inputs_and_reference_agree_with_torch_in_fp64():
    """adam_ref against torch.optim.Adam + clamp_ run in fp64 on the same gradients (pre-multiplied by grad_scale), and the frozen
    head of the arena: no gradient ever, so m = v = 0 and the update is 0 / eps = 0."""
    lr, b1, b2, eps = 2.0 ** -12, 0.875, 1 - 2.0 ** -8, 2.0 ** -27
    p0, grads = R.adam_inputs(4096)
    assert all(float(g[:R.ADAM_FROZEN].abs().max()) == 0.0 for g in grads) and float(grads[3].abs().max()) == 0.0
    for gs, clip in ((1.0, 0.0), (0.125, 0.05)):
        q = p0.double().clone().requires_grad_()
        opt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps)
        ref = R.adam_ref(p0, grads, lr, b1, b2, eps, gs, clip)
        for it, g in enumerate(grads):
            q.grad = g.double() * gs
            opt.step()
            if clip > 0:
                with torch.no_grad():
                    q.clamp_(-clip, clip)
            st = opt.state[q]
            assert R.err(ref[it][0], q) < 1e-13 and R.err(ref[it][1], st['exp_avg']) < 1e-13 and R.err(ref[it][2], st['exp_avg_sq']) < 1e-13
        want = p0[:R.ADAM_FROZEN].double().clamp(-clip, clip) if clip > 0 else p0[:R.ADAM_FROZEN].double()
        assert torch.equal(ref[-1][0][:R.ADAM_FROZEN], want)


# ---- argument refusals: a non-zero code and a message, before any launch ---------------------------------------------------


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    from sradsgan_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        ge.build()
    return _hip.lib()


@pytest.fixture(scope='module')
def host():
    """A host buffer whose address stands for every tensor argument: a refused call never reads it."""
    buf = (ctypes.c_float * 4096)()
    return buf, ctypes.addressof(buf)


def _refused(lib, rc, *words):
    msg = lib.srhip_last_error()
    assert rc != 0, 'accepted'
    assert msg and all(w.encode() in msg for w in words), msg


@pytest.mark.parametrize('c', [6, 1028])
def test_batch_norm_refuses_unsupported_channel_counts(lib, host, c):
    _, p = host
    rows, big = 8, 1 << 24
    _refused(lib, lib.srhip_bn_train_fwd(p, p, p, None, None, p, p, p, p, big, rows, c, 1e-5, 0.1, 0.2, 1, None), 'bn_train_fwd', 'multiple of 4')
    _refused(lib, lib.srhip_bn_train_bwd(p, p, p, p, p, p, p, p, p, p, big, rows, c, 0.2, 1, None), 'bn_train_bwd', 'multiple of 4')
    _refused(lib, lib.srhip_bn_train_bwd_acc_x(p, p, p, p, p, p, p, p, p, None, None, p, big, rows, c, 0.2, 1, None), 'bn_train_bwd')
    _refused(lib, lib.srhip_bn_train_bwd_acc_xa(p, p, p, p, p, p, p, p, p, p, None, None, p, big, rows, c, 0.2, 1, None), 'bn_train_bwd')
    _refused(lib, lib.srhip_bn_train_bwd_bwd(p, p, p, p, p, p, p, p, p, p, p, big, rows, c, 0.2, 1, None), 'bn_train_bwd_bwd', 'multiple of 4')
    _refused(lib, lib.srhip_bn_train_bwd_bwd_acc_x(p, p, p, p, p, p, p, p, p, p, None, p, big, rows, c, 0.2, 1, None), 'bn_train_bwd_bwd')


def test_batch_norm_forward_refuses_half_a_running_pair_and_a_short_workspace(lib, host):
    _, p = host
    _refused(lib, lib.srhip_bn_train_fwd(p, p, p, p, None, p, p, p, p, 1 << 24, 8, 8, 1e-5, 0.1, 0.2, 1, None), 'pairs')
    need = lib.srhip_bn_workspace(4097, 64)
    assert need >= 65 * 2 * 64 * 4
    _refused(lib, lib.srhip_bn_train_fwd(p, p, p, None, None, p, p, p, p, need - 1, 4097, 64, 1e-5, 0.1, 0.2, 1, None), 'workspace')


def test_adam_and_gradient_penalty_refuse_what_their_kernels_cannot_index(lib, host):
    _, p = host
    _refused(lib, lib.srhip_adam_step(p, p, p, p, p, 6, 1e-3, 0.9, 0.999, 1e-8, 1.0, 0.0, None), 'adam_step', 'multiple of 4')
    _refused(lib, lib.srhip_adam_step(p + 4, p, p, p, p, 8, 1e-3, 0.9, 0.999, 1e-8, 1.0, 0.0, None), 'adam_step', 'aligned')
    _refused(lib, lib.srhip_gp_norm_penalty_fwd(p, p, p, 4096, 10, 5, None), 'gp_norm_penalty_fwd')
    _refused(lib, lib.srhip_gp_norm_penalty_bwd(p, p, p, 10, 5, None), 'gp_norm_penalty_bwd')
    _refused(lib, lib.srhip_l1_mean_fwd(p + 4, p, p, p, 4096, 8, None), 'l1_mean_fwd', 'aligned')


@pytest.mark.parametrize('c,ld', [(257, 257), (258, 260), (1028, 1028), (2048, 2048), (64, 63), (0, 4)])
def test_colsum_refuses_what_it_cannot_serve(lib, host, c, ld):
    """The limits of srhip_colsum: C <= 1024 in multiples of 4, any other C <= 256, ld >= C.  Inside them every (ld, alignment) is
    SERVED (the scalar form walks the column groups of a C > 256 matrix; tests/test_reductions_gpu.py checks the sums), so nothing
    else is refused."""
    _, p = host
    _refused(lib, lib.srhip_colsum(p, p, p, 1 << 24, 100, c, ld, None), 'colsum')
