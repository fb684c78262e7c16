"""Generator inference + validation metrics on the device: the arithmetic of the reference's
mfeNew_validate / validate loops (SRADSGAN/model/sradsgan.py:1258-1391, 1058-1194) without the per-image
device->host->PIL->numpy round trip.  Metrics follow the reference bit for bit where it is integer work
(uint8 quantisation with wrap, MSE, PSNR, ERGAS of utils/utils.py:923-962) and to fp64 roundoff for SSIM
(scikit-image 0.15 algorithm, parity unpinned: skimage is not vendored by the reference).  LPIPS (sradsgan.py:561,
1125-1132, 1326-1332) is computed when the caller passes a loaded sradsgan_amd.lpips.LPIPS model; the pretrained AlexNet
file it needs is the user's to supply, and without a model the metric is simply absent from the results."""
import ctypes

import torch

from . import _hip, ops
from . import metrics as pub


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def quantized_metrics(sr, hr, scale):
    """sr, hr: [N,3,H,W] float tensors on the HIP device (any memory format).  Returns a dict of float64
    tensors [N]: mse, psnr, ssim, ergas -- per image, exactly what the reference computes after ToPILImage."""
    ops._require_gpu(sr, 'quantized_metrics')
    ops._require_gpu(hr, 'quantized_metrics')
    if sr.shape != hr.shape:
        raise ValueError('quantized_metrics: shape mismatch %s vs %s' % (tuple(sr.shape), tuple(hr.shape)))
    sr, hr = ops.nhwc(sr.detach()), ops.nhwc(hr.detach())
    n, c, h, w = sr.shape
    lib = _hip.lib()
    nb = lib.srhip_metric_blocks()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    part = torch.empty(n, nb, 2, device=sr.device, dtype=torch.int64)
    _hip.check(lib.srhip_quant_sse(_p(sr), _p(hr), _p(part), n, c * h * w, st), 'quant_sse')
    spart = torch.empty(n, nb, device=sr.device, dtype=torch.float64)
    _hip.check(lib.srhip_ssim_u8(_p(sr), _p(hr), _p(spart), n, h, w, c, st), 'ssim_u8')
    out = torch.empty(4, n, device=sr.device, dtype=torch.float64)          # rows: mse, psnr, ssim, ergas (one launch for the scalar tail)
    _hip.check(lib.srhip_metric_finish(_p(part), _p(spart), _p(out), n, h, w, c, float(scale), st), 'metric_finish')
    return dict(mse=out[0], psnr=out[1], ssim=out[2], ergas=out[3])


@torch.no_grad()
def evaluate(generator, lr, hr, scale, bicubic=None, lpips=None, protocol=None):
    """One validation batch: recon = G(lr) (sradsgan.py:1305), metrics of recon vs hr and -- when the
    bicubic-upsampled input is given -- of bicubic vs hr (:1328-1331).  Returns per-image metric dicts.
    lpips: an lpips.LPIPS model; then out['sr']['lpips'] (and out['bicubic']['lpips']) are float64 [N] of the unquantised
    images (:1326-1332), the backbone running once over [recon; hr; bicubic].
    protocol: None, or dict(crop_border=k, y_channel=bool): then out['sr'] (and out['bicubic']) also carry pub_mse, pub_psnr and
    pub_ssim, metrics.published_metrics of the same images -- the papers' protocol beside the reference trainer's, whose keys are
    computed exactly as without it."""
    recon = generator(lr)
    out = {'recon': recon, 'sr': quantized_metrics(recon, hr, scale)}
    if bicubic is not None:
        out['bicubic'] = quantized_metrics(bicubic, hr, scale)
    if lpips is not None:
        n = hr.shape[0]
        images = [hr, recon] + ([] if bicubic is None else [bicubic])
        d = lpips.pairs(images, [(i, n + i) for i in range(n)] + ([] if bicubic is None else [(i, 2 * n + i) for i in range(n)]))
        out['sr']['lpips'] = d[:n]
        if bicubic is not None:
            out['bicubic']['lpips'] = d[n:]
    if protocol is not None:
        for key, img in (('sr', recon),) + (() if bicubic is None else (('bicubic', bicubic),)):
            m = pub.published_metrics(img, hr, protocol['crop_border'], protocol['y_channel'])
            out[key].update(pub_mse=m['mse'], pub_psnr=m['psnr'], pub_ssim=m['ssim'])
    return out


class GraphedEvaluator:
    """evaluate() replayed from a captured hipGraph.  Generator inference at validation batch sizes is launch-bound
    (about 500 kernels of ~10 us for a batch of 16: the GPU waits for the Python launch loop), so the whole
    forward + metric pass is captured once per input shape and replayed; inputs are copied into the capture's static
    buffers, results live in static buffers that the next call overwrites (clone what must survive).
    Weights are read at replay time -- the parameters themselves and the packed images ops.packed_weight keeps of them --, and a replay
    runs none of the Python that keeps those images fresh.  So every call first compares, on the host, what the capture recorded with
    what the parameters (generator and LPIPS model) say now:
      * a `_version` that moved since the image was packed (load_state_dict, a torch optimiser, an initialiser): the images of that
        parameter are packed again in place (ops.weights_changed), then the graph is replayed;
      * a `data_ptr()` that moved (dp.ParamArena built after the capture, `p.data = ...`): the capture reads storage the parameter has
        left, so the captures are dropped and the call captures again -- it never returns numbers of the old weights.
    Writes torch cannot see (the fused Adam, `.data` writes) need what they need everywhere: ops.bump_weight_epoch() /
    ops.weights_changed() after them.  In the steady state the comparison launches nothing."""

    def __init__(self, generator, scale, warmup=2, lpips=None, protocol=None):
        self.generator, self.scale, self.warmup, self.lpips = generator, scale, warmup, lpips
        self.protocol = None if protocol is None else dict(crop_border=protocol['crop_border'], y_channel=bool(protocol['y_channel']))
        self._graphs = {}

    def _capture(self, key, lr, hr, bicubic):
        static = dict(lr=lr.clone(), hr=hr.clone(), bicubic=None if bicubic is None else bicubic.clone())
        side = torch.cuda.Stream(device=lr.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                 # library / allocator / packed-weight warm-up outside the capture
            for _ in range(self.warmup):
                evaluate(self.generator, static['lr'], static['hr'], self.scale, static['bicubic'], self.lpips, self.protocol)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = evaluate(self.generator, static['lr'], static['hr'], self.scale, static['bicubic'], self.lpips, self.protocol)
        self._graphs[key] = (graph, static, out)
        self._params = self._parameters()
        self._ptrs = [p.data_ptr() for p in self._params]

    def _parameters(self):
        nets = [self.generator] + ([] if self.lpips is None else [self.lpips])
        return [p for net in nets for p in net.parameters()]

    def _follow_weights(self):
        """Host only unless something has changed (class docstring).  False: the captures were dropped."""
        params = self._parameters()
        if len(params) != len(self._params) or any(a is not b for a, b in zip(params, self._params)) \
                or any(p.data_ptr() != ptr for p, ptr in zip(params, self._ptrs)):
            self._graphs.clear()
            return False
        stale = [p for p in params
                 if any(ent[4] != p._version for ent in getattr(p, '_srhip_packed', {}).values())
                 or any(got[0] != p._version for got in getattr(p, '_srhip_derived', {}).values())]
        if stale:
            ops.weights_changed(*stale)
        return True

    def __call__(self, lr, hr, bicubic=None):
        ops._require_gpu(lr, 'GraphedEvaluator')
        key = (tuple(lr.shape), tuple(hr.shape), bicubic is not None, ops.get_conv_math())
        if self.protocol is not None:                 # `protocol` may be reassigned between calls: one capture per value
            key += (self.protocol['crop_border'], bool(self.protocol['y_channel']))
        if self._graphs:
            self._follow_weights()
        if key not in self._graphs:
            self._capture(key, lr, hr, bicubic)
        graph, static, out = self._graphs[key]
        static['lr'].copy_(lr)
        static['hr'].copy_(hr)
        if bicubic is not None:
            static['bicubic'].copy_(bicubic)
        graph.replay()
        return out


def format_results(mode, rlt):
    """The log line of the reference's PrintLogger.print_format_results (SRADSGAN/utils/logger.py:117-147), as a
    string: '<epoch:  3, iter:   1,200, time:1.25, lr:2.0e-04> dataset: AID key: 1.23e-04 ...' -- '{:.2e}' per value
    in 'train' mode, '{:.4e}' in 'val' mode.  `rlt` must carry epoch, iters, time, model (and optionally lr); it is
    not modified."""
    rlt = dict(rlt)
    epoch, iters, time_, model = rlt.pop('epoch'), rlt.pop('iters'), rlt.pop('time'), rlt.pop('model')
    if 'lr' in rlt:
        message = '<epoch:{:3d}, iter:{:8,d}, time:{:.2f}, lr:{:.1e}> '.format(epoch, iters, time_, rlt.pop('lr'))
    else:
        message = '<epoch:{:3d}, iter:{:8,d}, time:{:.2f}> '.format(epoch, iters, time_)
    message += '{:s}: {:s} '.format('dataset', model)
    for label, value in rlt.items():
        if mode == 'train':
            message += '{:s}: {:.2e} '.format(label, value)
        elif mode == 'val':
            message += '{:s}: {:.4e} '.format(label, value)
    return message


def append_log(path, mode, rlt):
    """Appends format_results(mode, rlt) to loss_log.txt / val_log.txt like the reference (logger.py:142-147)."""
    line = format_results(mode, rlt)
    with open(path, 'a') as f:
        f.write(line + '\n')
    return line
