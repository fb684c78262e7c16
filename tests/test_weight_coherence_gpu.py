"""Cached weight images follow every way a weight can change.

Convolutions never read a Parameter: they read a packed image that ops.packed_weight keeps on the parameter object and refreshes when
the parameter's `_version` or `data_ptr()` moves, when the fused optimiser calls ops.bump_weight_epoch(), or when the caller says so
(ops.weights_changed).  Two captured graphs (TrainStep(use_graph=True), validate.GraphedEvaluator) read those images at replay time.

The oracle is the kernel itself on a fresh image: ops.packed_weight packs on the fly for anything that is no nn.Parameter, so the same
raw op fed `w.detach().clone()` -- for a module, a copy.deepcopy of it, whose Parameters are new objects without a cache -- runs the
same kernel on an image of the weights as they are now.  Every comparison is torch.equal; there are no tolerances.  Every row first
asserts that the fresh result after the change differs from the fresh result before it: a change that did nothing cannot pass, and a
stale image (which reproduces the "before" result) is always told apart.

What these rows found when they were written (each is fixed in the package): the initialisers of trainer, model/srgan and model/spectral
wrote through `.data` (rows j); nothing refreshed an image after a silent write (rows k); a fused Adam step on a static net left its
images stale (row e, static); a SpectralNorm kept the Parameter objects load_state_dict(assign=True) had replaced (row c-assign,
spectral); the eval attention tail refused a bias at an unaligned offset (row h, generator); GraphedEvaluator replayed old images after
load_state_dict and old storage after a re-homing (c, f, g); a Parameter that had run could not be pickled.

tests/test_weight_coherence_cpu.py records which of the channels below torch reports (version / pointer) and which are silent."""
import copy
import gc
import io
import pickle

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
MATHS = ('fp32', 'bf16x3', 'half')
# cout, cin, k: the 64 -> 64 trunk conv, the head, the narrow (64 -> 3) kernel, the 1x1
SHAPES = {'trunk': (64, 64, 3), 'head': (64, 3, 3), 'narrow': (3, 64, 3), 'pointwise': (64, 64, 1)}


def _cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


@pytest.fixture(autouse=True)
def _registry_as_found():
    """The registry is global: models of a test are dropped with it, and their entries leave at the next repack_all."""
    from sradsgan_amd import ops
    yield
    gc.collect()
    ops.repack_all()
    torch.cuda.synchronize()


# ---- consumers ------------------------------------------------------------------------------------------------------------------------ #
class Consumer:
    """`net`, inputs, and run(net) -> list of result tensors.  cached(): on the net itself (its cached images); fresh(): on images
    packed now from the weights as they are."""
    def cached(self):
        return [t.detach().clone() for t in self.run(self.net)]

    def fresh(self):
        return [t.detach().clone() for t in self.run(copy.deepcopy(self.net))]


class RawConvs(Consumer):
    """ops.conv2d_fwd_raw (image 0) and ops.conv2d_dgrad_raw (image 1) of four weight shapes on x of 2 x Cin x 9 x 7, under each
    conv math.  fresh(): the same calls fed w.detach().clone()."""

    def __init__(self):
        from sradsgan_amd.model.layers import HipConv2d
        g = torch.Generator().manual_seed(11)
        self.net = nn.ModuleDict({k: HipConv2d(cin, cout, kk, 1, kk // 2) for k, (cout, cin, kk) in SHAPES.items()})
        with torch.no_grad():
            for p in self.net.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
        self.net.to(DEV)
        self.x = {k: _cl(torch.randn(2, cin, 9, 7, generator=g)) for k, (cout, cin, kk) in SHAPES.items()}
        self.dy = {k: _cl(torch.randn(2, cout, 9, 7, generator=g)) for k, (cout, cin, kk) in SHAPES.items()}

    def run(self, net, clone=False):
        from sradsgan_amd import ops
        outs = []
        for k, (cout, cin, kk) in SHAPES.items():
            w = net[k].weight
            if clone:
                w = w.detach().clone()
            for math in MATHS:
                with ops.conv_math(math):
                    outs.append(ops.conv2d_fwd_raw(self.x[k], w, None, 1, kk // 2))
                    outs.append(ops.conv2d_dgrad_raw(self.dy[k], w, (2, cin, 9, 7), 1, kk // 2))
        return outs

    def fresh(self):
        return [t.detach().clone() for t in self.run(self.net, clone=True)]


class Generator(Consumer):
    """A one-block ResGroup generator: training-mode forward and input gradient (the fused RAB, padded planes), and the no_grad / eval
    forward (_tail_forward_eval and the plane routes of inference), under bf16x3 -- the arithmetic the planes exist in."""

    def __init__(self):
        from sradsgan_amd import model as M
        torch.manual_seed(12)
        self.net = M.GeneratorResNet(M.ResGroup, n_residual_blocks=1, n_basic_blocks=1, upscale_factor=2).to(DEV)
        g = torch.Generator().manual_seed(13)
        self.x = torch.rand(2, 3, 9, 7, generator=g).to(DEV)
        self.dy = torch.randn(2, 3, 18, 14, generator=g).to(DEV)

    def run(self, net):
        from sradsgan_amd import ops
        with ops.conv_math('bf16x3'):
            net.train()
            x = self.x.clone().requires_grad_(True)
            y = net(x)
            gx, = torch.autograd.grad(y, x, self.dy)
            net.eval()
            with torch.no_grad():
                ye = net(self.x)
        return [y, gx, ye]


class _Wrap(nn.Module):
    def __init__(self, inner, call):
        super().__init__()
        self.inner, self._call = inner, call

    def forward(self, x):
        return self._call(self.inner, x)


def _call_module(m, x):
    return m(x)


def _call_linear(m, x):
    from sradsgan_amd import ops
    return ops.linear(x, m.weight, m.bias)


class OneLayer(Consumer):
    """One layer that packs by its own route: forward and input gradient."""

    def __init__(self, kind):
        from sradsgan_amd.model.layers import HipConv2d, HipDilatedConv2d
        torch.manual_seed(14)
        c = 64
        if kind == 'dilated':                                    # ops.conv2d_dil
            self.net = _Wrap(HipDilatedConv2d(64, 64, 3, padding=2, dilation=2), _call_module)
        elif kind == 'linear':                                   # ops.linear at a published HAT width
            c = 180
            self.net = _Wrap(nn.Linear(180, 180), _call_linear)
        else:                                                    # weight_bar is the leaf, the effective weight of each pass is not
            from sradsgan_amd.model.spectral import SpectralNorm
            self.net = _Wrap(SpectralNorm(HipConv2d(64, 64, 3, 1, 1)), _call_module)
        self.net.to(DEV)
        g = torch.Generator().manual_seed(15)
        self.x = _cl(torch.randn(2, c, 9, 7, generator=g))
        self.dy = _cl(torch.randn(2, c, 9, 7, generator=g))

    def run(self, net):
        from sradsgan_amd import ops
        with ops.conv_math('bf16x3'):
            x = self.x.clone().requires_grad_(True)
            y = net(x)
            gx, = torch.autograd.grad(y, x, self.dy)
        return [y, gx]


CONSUMERS = {'raw': RawConvs, 'generator': Generator, 'dilated': lambda: OneLayer('dilated'), 'linear': lambda: OneLayer('linear'),
             'spectral': lambda: OneLayer('spectral')}


# ---- change channels ------------------------------------------------------------------------------------------------------------------ #
def _new_values(net, seed=21):
    g = torch.Generator().manual_seed(seed)
    return {k: (torch.randn(v.shape, generator=g) * 0.07).to(v.device) for k, v in net.state_dict().items()}


def ch_copy_(c):
    new = _new_values(c.net)
    with torch.no_grad():
        for k, p in c.net.named_parameters():
            p.copy_(new[k])


def ch_init_normal(c):
    for p in c.net.parameters():
        nn.init.normal_(p, 0.0, 0.05)


def ch_load_state_dict(c):
    c.net.load_state_dict(_new_values(c.net), strict=True)


def ch_load_state_dict_assign(c):
    c.net.load_state_dict(_new_values(c.net), strict=True, assign=True)


def _torch_optimizer(cls, **kw):
    def change(c):
        params = [p for p in c.net.parameters() if p.requires_grad]
        for p in params:
            p.grad = torch.full_like(p, 0.5)
        cls(params, lr=0.01, **kw).step()
        for p in params:
            p.grad = None
    return change


def ch_arena_adam(c):
    from sradsgan_amd import ops
    c.arena.flat_g.fill_(0.5)
    c.arena.adam_step(0.01, 0.9, 0.999, 1e-8)
    ops.bump_weight_epoch()


def ch_data_assign(c):
    for p in c.net.parameters():
        p.data = p.data * 1.5 + 0.01


def ch_arena_after_run(c):
    """dp.ParamArena adopts a net that has run (every parameter is re-homed), then the weights are written in a way torch reports."""
    from sradsgan_amd.dp import ParamArena
    c.arena = ParamArena(c.net)
    ch_copy_(c)


def ch_arena_after_run_then_epoch(c):
    """...then one fused Adam step and the batched re-pack BEFORE the next use: the batched table still names the storage the
    parameters have left."""
    from sradsgan_amd.dp import ParamArena
    c.arena = ParamArena(c.net)
    ch_arena_adam(c)


def ch_vector_to_parameters(c):
    params = list(c.net.parameters())
    vec = torch.nn.utils.parameters_to_vector(params)
    torch.nn.utils.vector_to_parameters(vec * 1.5 + 0.01, params)


def ch_load_epoch_network(c):
    from sradsgan_amd import checkpoint as C
    path = str(c.tmp_path / 'net_param_epoch_1.pkl')
    torch.save({k: v.cpu() for k, v in _new_values(c.net).items()}, path)
    C.load_epoch_network(path, c.net)
    assert c.arena.check_views()


def ch_trainer_init(c):
    from sradsgan_amd.trainer import weights_init_normal
    c.net.apply(lambda m: weights_init_normal(m, 0.0, 0.05))


def ch_srgan_init(c):
    from sradsgan_amd.model.srgan import weights_init_normal
    c.net.apply(lambda m: weights_init_normal(m) if isinstance(getattr(m, 'weight', None), torch.Tensor) else None)


def ch_spectral_init(c):
    from sradsgan_amd.model.spectral import spectral_init_
    spectral_init_(c.net, std=0.05)


# the silent writes (tests/test_weight_coherence_cpu.py): torch cannot see them, one ops.weights_changed call must
def ch_data_normal_(c):
    for p in c.net.parameters():
        p.data.normal_(0.0, 0.05)


def ch_data_clamp_(c):
    for p in c.net.parameters():
        p.data.clamp_(-0.01, 0.01)                               # the reference's clip, sradsgan.py:891-892


def ch_ema_through_data(c):
    new = _new_values(c.net)
    for k, p in c.net.named_parameters():
        p.data.mul_(0.5).add_(new[k], alpha=0.5)


def ch_foreach_on_data(c):
    torch._foreach_mul_([p.data for p in c.net.parameters()], 1.5)


# name -> (change, needs an arena built before the first use, consumers the change cannot walk or does not touch)
REPORTED = {
    'a-copy_': (ch_copy_, False, ()),
    'b-init.normal_': (ch_init_normal, False, ()),
    'c-load_state_dict': (ch_load_state_dict, False, ()),
    'c-load_state_dict-assign': (ch_load_state_dict_assign, False, ()),
    'd-Adam-foreach': (_torch_optimizer(torch.optim.Adam, foreach=True), False, ()),
    'd-Adam-single': (_torch_optimizer(torch.optim.Adam, foreach=False), False, ()),
    'd-SGD-foreach': (_torch_optimizer(torch.optim.SGD, foreach=True), False, ()),
    'd-SGD-single': (_torch_optimizer(torch.optim.SGD, foreach=False), False, ()),
    'e-arena-adam-epoch': (ch_arena_adam, True, ()),
    'f-data-assign': (ch_data_assign, False, ()),
    'g-arena-after-run': (ch_arena_after_run, False, ()),
    'g2-arena-after-run-then-epoch': (ch_arena_after_run_then_epoch, False, ()),
    'h-vector_to_parameters': (ch_vector_to_parameters, False, ()),
    'i-load_epoch_network': (ch_load_epoch_network, True, ()),
    'j-trainer-init': (ch_trainer_init, False, ('spectral',)),
    'j-srgan-init': (ch_srgan_init, False, ('spectral', 'linear')),
    'j-spectral-init': (ch_spectral_init, False, ()),
}
SILENT = {
    'k-data.normal_': ch_data_normal_,
    'k-data.clamp_': ch_data_clamp_,
    'k-ema-through-data': ch_ema_through_data,
    'k-foreach-on-data': ch_foreach_on_data,
}


def _build(consumer, static, arena_first, tmp_path):
    from sradsgan_amd import ops
    from sradsgan_amd.dp import ParamArena
    c = CONSUMERS[consumer]()
    c.tmp_path, c.arena = tmp_path, None
    if static:
        ops.mark_static(c.net)
    if arena_first:
        c.arena = ParamArena(c.net)
    ref = c.fresh()                                              # (before the net's own run: a spectral conv advances u and v per pass)
    for a, b in zip(c.cached(), ref):                            # the net has run: both image kinds exist
        assert torch.equal(a, b)
    return c


def _assert_follows(c, change, what, then=None):
    before = c.fresh()
    change(c)
    if then is not None:
        then(c)
    after = c.fresh()
    got = c.cached()
    assert len(got) == len(after) == len(before)
    for i, (b, a) in enumerate(zip(before, after)):
        assert not torch.equal(b, a), '%s: result %d did not move with the weights -- the row proves nothing' % (what, i)
    stale = [i for i, (g, a) in enumerate(zip(got, after)) if not torch.equal(g, a)]
    assert not stale, '%s: results %s were computed from images of other weights (equal to the old ones: %s)' % (
        what, stale, [torch.equal(got[i], before[i]) for i in stale])


_REPORTED_CASES = [(cons, name) for cons in CONSUMERS for name, (_, _, excluded) in REPORTED.items() if cons not in excluded]


@pytest.mark.parametrize('static', [False, True], ids=['trainable', 'static'])
@pytest.mark.parametrize('consumer,channel', _REPORTED_CASES, ids=['%s-%s' % c for c in _REPORTED_CASES])
def test_images_follow_a_write_torch_reports_without_help(consumer, channel, static, tmp_path):
    change, arena_first, _ = REPORTED[channel]
    c = _build(consumer, static, arena_first, tmp_path)
    _assert_follows(c, change, '%s / %s' % (consumer, channel))


_SILENT_CASES = [(cons, name) for cons in CONSUMERS for name in SILENT]


@pytest.mark.parametrize('static', [False, True], ids=['trainable', 'static'])
@pytest.mark.parametrize('consumer,channel', _SILENT_CASES, ids=['%s-%s' % c for c in _SILENT_CASES])
def test_images_follow_a_silent_write_after_weights_changed(consumer, channel, static, tmp_path):
    from sradsgan_amd import ops
    c = _build(consumer, static, False, tmp_path)
    _assert_follows(c, SILENT[channel], '%s / %s' % (consumer, channel), then=lambda c: ops.weights_changed(c.net))


def test_weights_changed_takes_parameters_as_well_as_modules():
    from sradsgan_amd import ops
    c = _build('raw', True, False, None)
    _assert_follows(c, ch_data_normal_, 'raw / parameters named one by one', then=lambda c: ops.weights_changed(*c.net.parameters()))
    with pytest.raises(TypeError):
        ops.weights_changed('net')


def test_static_then_trainable_follows_each_change(tmp_path):
    """mark_static -> change -> mark_trainable -> change, with the batched re-pack as the only refresh of the last one."""
    from sradsgan_amd import ops
    from sradsgan_amd.dp import ParamArena
    c = _build('raw', True, False, tmp_path)
    _assert_follows(c, ch_init_normal, 'static')
    assert not any(ent[0]() is p for ent in ops._registry.entries for p in c.net.parameters())
    ops.mark_trainable(c.net)
    _assert_follows(c, ch_load_state_dict, 'trainable again')
    weights = [m.weight for m in c.net.values()]
    assert all(sum(ent[0]() is w for ent in ops._registry.entries) == 2 for w in weights)       # both kinds are in the batched re-pack
    c.arena = ParamArena(c.net)
    c.cached()
    _assert_follows(c, ch_arena_adam, 'trainable again, fused Adam + epoch')


# ---- the LPIPS stem copy ---------------------------------------------------------------------------------------------------------------- #
class Stem(Consumer):
    """lpips.LPIPS keeps an HWIO copy of its stem weight; the oracle is ops.lpips_stem_raw fed a fresh permutation.  The deterministic
    init of the constructor stands for the AlexNet file."""

    def __init__(self):
        from sradsgan_amd.lpips import LPIPS
        self.model = LPIPS().to(DEV)
        self.net = self.model.features[0]
        self.x = torch.rand(2, 3, 31, 31, generator=torch.Generator().manual_seed(16)).to(DEV)

    def cached(self):
        with torch.no_grad():
            return [self.model.feature_taps(self.x)[0].detach().clone()]

    def fresh(self):
        from sradsgan_amd import ops
        w = self.net.weight.detach().clone().permute(2, 3, 1, 0).contiguous()
        return [ops.lpips_stem_raw(self.x, w, self.net.bias.detach().clone()).detach().clone()]


@pytest.mark.parametrize('channel', ['a-copy_', 'c-load_state_dict', 'c-load_state_dict-assign'] + sorted(SILENT))
def test_lpips_stem_copy_follows_the_weights(channel):
    from sradsgan_amd import ops
    c = Stem()
    c.tmp_path = c.arena = None
    assert torch.equal(c.cached()[0], c.fresh()[0])
    if channel in SILENT:
        _assert_follows(c, SILENT[channel], 'lpips stem / ' + channel, then=lambda c: ops.weights_changed(c.model))
    else:
        _assert_follows(c, REPORTED[channel][0], 'lpips stem / ' + channel)


# ---- captured graphs ------------------------------------------------------------------------------------------------------------------- #
def _evaluator(arena_first):
    from sradsgan_amd import model as M, validate
    from sradsgan_amd.dp import ParamArena
    torch.manual_seed(17)
    c = Consumer()
    c.net = M.GeneratorResNet(M.ResGroup, n_residual_blocks=1, n_basic_blocks=1, upscale_factor=4).to(DEV).eval()
    c.arena = ParamArena(c.net) if arena_first else None
    g = torch.Generator().manual_seed(18)
    c.lr, c.hr = torch.rand(2, 3, 12, 10, generator=g).to(DEV), torch.rand(2, 3, 48, 40, generator=g).to(DEV)
    c.ev = validate.GraphedEvaluator(c.net, 4)
    return c


def _replay(c):
    out = c.ev(c.lr, c.hr)
    return [out['recon'].clone()] + [out['sr'][k].clone() for k in ('mse', 'psnr', 'ssim', 'ergas')]


def _eager(c):
    from sradsgan_amd import validate
    out = validate.evaluate(c.net, c.lr, c.hr, 4)
    return [out['recon'].clone()] + [out['sr'][k].clone() for k in ('mse', 'psnr', 'ssim', 'ergas')]


@pytest.mark.parametrize('channel', ['c-load_state_dict', 'e-arena-adam-epoch', 'i-load_epoch_network', 'f-data-assign', 'g-arena-after-run'])
def test_graphed_evaluator_never_replays_old_weights(channel, tmp_path):
    """After a write in place (c, e, i) the replay reads refreshed images; after the storage moved under the live capture (f, g) the
    call captures again (the class docstring states the choice).  The replay runs BEFORE any eager pass could refresh the images."""
    change, arena_first, _ = REPORTED[channel]
    c = _evaluator(arena_first)
    c.tmp_path = tmp_path
    before = _replay(c)
    for a, b in zip(before, _eager(c)):
        assert torch.equal(a, b)
    _replay(c)                                                   # a second replay: the capture is live and warm
    change(c)
    got = _replay(c)
    want = _eager(c)
    assert not torch.equal(want[0], before[0])
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), (channel, i, 'stale' if torch.equal(a, before[i]) else 'neither old nor new')
    for a, b in zip(_replay(c), want):                           # and the next replay stays there
        assert torch.equal(a, b)


def _train(use_graph, heal):
    """5 steps at the size of tests/test_graph_gpu.py, the initial weights loaded back between steps 3 and 4."""
    from oracle import sradsgan_ref as O
    from sradsgan_amd import ops
    from sradsgan_amd.train_step import TrainStep
    from tests.parity_util import build_pair
    (hg, hd, hf), _ = build_pair(2, 1, 4, DEV)
    initial = [{k: v.detach().clone() for k, v in net.state_dict().items()} for net in (hg, hd)]
    step = TrainStep(hg, hd, hf, use_graph=use_graph, overlap_wgrad=False, overlap_d_step=False)
    batches = [(O.det_fill('graph.lr.%d' % i, (4, 3, 24, 24), 0.5, 0.5).to(DEV), O.det_fill('graph.hr.%d' % i, (4, 3, 96, 96), 0.5, 0.5).to(DEV),
                O.det_fill('graph.alpha.%d' % i, (4, 1, 1, 1), 0.5, 0.5).to(DEV)) for i in range(3)]
    names = ('loss_G', 'loss_D', 'pixel', 'content', 'loss_gan', 'gp')
    scal = []
    for it in range(5):
        if it == 3:
            hg.load_state_dict(initial[0])
            hd.load_state_dict(initial[1])
            if heal == 'epoch':
                ops.bump_weight_epoch()
            else:
                ops.weights_changed(hg, hd)
        out = step(*batches[it % 3])
        scal.append(torch.stack([out[k].double() for k in names]).clone())
    torch.cuda.synchronize()
    return torch.stack(scal).cpu(), [p.detach().clone() for p in list(hg.parameters()) + list(hd.parameters())]


@pytest.fixture(scope='module')
def eager_training():
    return _train(False, 'epoch')


@pytest.mark.parametrize('heal', ['epoch', 'weights_changed'])
def test_train_step_graph_follows_a_load_between_replays(eager_training, heal):
    want_s, want_w = eager_training
    got_s, got_w = _train(True, heal)
    assert torch.isfinite(want_s).all()
    assert not torch.equal(want_s[3], want_s[2])
    bad = (got_s != want_s).any(dim=1).nonzero().flatten().tolist()
    assert not bad, ('the replayed step differs from the eager one at iterations', bad)
    for a, b in zip(got_w, want_w):
        assert torch.equal(a, b)


# ---- activation caches ----------------------------------------------------------------------------------------------------------------- #
def _two_rabs():
    from sradsgan_amd import model as M
    torch.manual_seed(19)
    blocks = nn.ModuleList([M.RAB(64, 64) for _ in range(2)]).to(DEV)
    x = _cl(torch.randn(2, 64, 9, 7, generator=torch.Generator().manual_seed(20)))
    return blocks, x


def _first_rab(blocks, x):
    blocks[0]._next_is_rab = True
    return blocks[0](x.clone().requires_grad_(True))


def _first_tail(blocks, x):
    from sradsgan_amd import ops
    b = blocks[0]
    u = x.clone().requires_grad_(True)
    return ops.attention_tail(u, (x * 0.5).requires_grad_(True), b.ca.fc1.weight, b.ca.fc2.weight, b.sa.conv1.weight, b.conv.weight,
                              b.conv.bias, emit_pp=True)


@pytest.mark.parametrize('producer', [_first_rab, _first_tail], ids=['rab_block', 'attention_tail'])
def test_an_in_place_edit_voids_handed_over_planes(producer):
    """A fused RAB (or the attention tail with emit_pp) hands its output over as padded planes too, tagged with the output's version.
    x.mul_(2) on the tagged tensor must void them: the next RAB equals the run in which nothing is handed over."""
    from sradsgan_amd import ops
    blocks, x = _two_rabs()
    outs = {}
    with ops.conv_math('bf16x3'):
        for hand_over in (True, False):
            old, ops._X_PP = ops._X_PP, hand_over
            try:
                mid = producer(blocks, x)
                tag = getattr(mid, '_srhip_pp', None)
                if hand_over:
                    assert tag is not None and tag[1] == mid._version, 'nothing was handed over: the test would prove nothing'
                    unedited = blocks[1](mid).detach().clone()
                else:
                    assert tag is None
                mid.mul_(2.0)
                outs[hand_over] = blocks[1](mid).detach().clone()
            finally:
                ops._X_PP = old
    assert not torch.equal(outs[False], unedited)
    assert torch.equal(outs[True], outs[False])


def test_an_in_place_edit_reaches_the_adopted_dense_buffer():
    """dcrdb_step(chain=True) writes its result into the next step's dense buffer and tags it; the next step adopts the buffer.  An edit
    of the handed-over tensor in between must be what the next step computes from: equal to the unchained run on the edited tensor."""
    from sradsgan_amd import ops
    from sradsgan_amd.model.ndsrgan import DCRDB
    torch.manual_seed(22)
    blocks = nn.ModuleList([DCRDB(64, 32) for _ in range(2)]).to(DEV)
    x = _cl(torch.randn(2, 64, 9, 7, generator=torch.Generator().manual_seed(23)))
    outs = {}
    with torch.no_grad(), ops.conv_math('bf16x3'):
        for chain in (True, False):
            mid = blocks[0].forward_sum(x, chain=chain)
            assert (getattr(mid, '_srhip_dense_buf', None) is not None) == chain
            if chain:
                unedited = blocks[1].forward_sum(mid).clone()
            mid.mul_(2.0)
            fills = ops.dense_stats.fills
            outs[chain] = blocks[1].forward_sum(mid).clone()
            assert ops.dense_stats.fills == fills + (0 if chain else 1)          # adopted, not copied
    assert not torch.equal(outs[False], unedited)
    assert torch.equal(outs[True], outs[False])


# ---- pickling and copies ---------------------------------------------------------------------------------------------------------------- #
class TwoConvs(nn.Module):
    def __init__(self):
        from sradsgan_amd.model.layers import HipConv2d
        super().__init__()
        self.conv = HipConv2d(64, 64, 3, 1, 1)
        self.out = HipConv2d(64, 3, 3, 1, 1)

    def forward(self, x):
        return self.out(self.conv(x, act_slope=0.2))


def _ran_net():
    torch.manual_seed(24)
    net = TwoConvs().to(DEV)
    x = _cl(torch.randn(2, 64, 9, 7, generator=torch.Generator().manual_seed(25)))
    net(x.clone().requires_grad_(True)).square().mean().backward()          # forward and backward: both image kinds exist
    return net, x


def _via_torch_save(net):
    buf = io.BytesIO()
    torch.save(net, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=False)


def _via_pickle(net):
    return pickle.loads(pickle.dumps(net))


@pytest.mark.parametrize('how', [_via_torch_save, _via_pickle, copy.deepcopy], ids=['torch.save', 'pickle', 'deepcopy'])
def test_a_net_that_has_run_can_be_pickled_and_copied(how):
    from sradsgan_amd import ops
    entries = len(ops._registry.entries)
    net, x = _ran_net()
    assert len(ops._registry.entries) > entries
    pickle.loads(pickle.dumps(net.conv.weight))
    twin = how(net)
    assert not getattr(twin.conv.weight, '_srhip_packed', None)                 # no cache entry travels into a copy
    with torch.no_grad():
        want = net(x).clone()
        assert torch.equal(twin(x), want)

        def rewrite(m, seed):
            g = torch.Generator().manual_seed(seed)
            for p in m.parameters():
                p.copy_((torch.randn(p.shape, generator=g) * 0.1).to(DEV))
        rewrite(twin, 26)
        changed = twin(x).clone()
        assert not torch.equal(changed, want)
        assert torch.equal(net(x), want)                                        # the original still reads its own images
        rewrite(net, 27)
        moved = net(x).clone()
        assert not torch.equal(moved, want) and not torch.equal(moved, changed)
        assert torch.equal(twin(x), changed)                                    # and the other way round
    mine = [ent for p in net.parameters() for ent in getattr(p, '_srhip_packed', {}).values()]
    theirs = [ent for p in twin.parameters() for ent in getattr(p, '_srhip_packed', {}).values()]
    assert mine and theirs and not any(a is b or a[2].data_ptr() == b[2].data_ptr() for a in mine for b in theirs)
    del net, twin, mine, theirs
    gc.collect()
    ops.repack_all()
    assert len(ops._registry.entries) == entries
