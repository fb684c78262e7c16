"""Generate tests/golden/gdp_*.npz by running the REFERENCE GDP_x0/model/gdp_modules (unet.py, diffusion.py) on the CPU (build
container only: tqdm, torchvision and PIL are stubbed, the two files are loaded by path so that GDP_x0/model/__init__.py's trainer
imports stay out).  Parameters come from tests/gdp_ref.init_ (the deterministic filler keyed by state-dict name).

  gdp_small.npz     the small net (gdp_ref.SMALL) on gdp_ref.small_input() at t in {0, 1, 7, 999} and with two different t in a batch
  gdp_loop.npz      the same net through p_sample_loop on a 6-step linear schedule: the seven tensors torch.randn returned under
                    torch.manual_seed(gdp_ref.LOOP_SEED), the final image and the continous=True stack
  gdp_schedule.npz  the schedule buffers of linear/1000 and cosine/50 as float32
  gdp_full.npz      sorted state-dict keys, shapes and the parameter count of define_G(gdp_test_54_216.json), built on the meta device
  gdp_test_54_216.json   the reference's configuration file itself (settings only)

Prints the distance of the float64 restatement (tests/gdp_ref.py) from the reference's float32 vectors: the CPU test's bar is ten
times that."""
import importlib.util
import json
import os
import re
import shutil
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import sradsgan_ref as O  # noqa: E402
from oracle.make_golden import REF  # noqa: E402
from tests import gdp_ref as R  # noqa: E402

GDP = os.path.join(REF, 'GDP_x0')
GOLD = os.path.join(ROOT, 'tests', 'golden')


def import_gdp():
    for name in ('tqdm', 'torchvision', 'torchvision.transforms', 'torchvision.transforms.functional', 'PIL', 'PIL.Image'):
        try:
            importlib.import_module(name)
        except ImportError:
            m = types.ModuleType(name)
            m.__path__ = []
            sys.modules[name] = m
    sys.modules['tqdm'].tqdm = getattr(sys.modules['tqdm'], 'tqdm', lambda it, **kw: it)
    tv = sys.modules['torchvision.transforms']
    if not hasattr(tv, 'functional'):
        tv.functional = sys.modules['torchvision.transforms.functional']
    if not hasattr(sys.modules['PIL'], 'Image'):
        sys.modules['PIL'].Image = sys.modules['PIL.Image']
    mods = []
    for leaf in ('unet', 'diffusion'):
        spec = importlib.util.spec_from_file_location('gdp_ref_modules_' + leaf, os.path.join(GDP, 'model', 'gdp_modules', leaf + '.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mods.append(mod)
    return mods


def load_config(path):
    return json.loads(re.sub(r'//.*', '', open(path).read()))


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max())


def main():
    torch.set_num_threads(8)
    unet, diffusion = import_gdp()
    net = R.init_(unet.UNet(**R.SMALL)).eval()
    sd64, sd32 = R.state(net, torch.float64), R.state(net, torch.float32)
    x = R.small_input()
    out, worst, floor = {}, 0.0, 0.0
    with torch.no_grad():
        for name, ts in R.SMALL_T.items():
            t = torch.tensor(ts, dtype=torch.long)
            y = net(x, t)
            out[name] = O.digest(y)
            worst = max(worst, rel(R.unet_forward(sd64, x.double(), t, R.SMALL), y))
            floor = max(floor, rel(R.unet_forward(sd32, x, t, R.SMALL), R.unet_forward(sd64, x.double(), t, R.SMALL)))
    out['shape'] = np.array(y.shape)
    np.savez_compressed(os.path.join(GOLD, 'gdp_small.npz'), **out)
    print('small net: fp64 restatement vs reference fp32 %.3e, restatement fp32 vs fp64 %.3e' % (worst, floor))

    G = diffusion.GaussianDiffusion(net, image_size=12, channels=3, conditional=True)
    G.set_new_noise_schedule(R.LOOP_SCHEDULE, 'cpu')
    cond = x[:, 3:].contiguous()
    drawn, randn = [], torch.randn

    def recording(*a, **k):
        z = randn(*a, **k)
        drawn.append(z.clone())
        return z

    stacks = {}
    for cont in (False, True):
        torch.manual_seed(R.LOOP_SEED)
        del drawn[:]
        torch.randn = recording
        try:
            stacks[cont] = G.super_resolution(cond, continous=cont)
        finally:
            torch.randn = randn
    noise = torch.stack(drawn)
    sdg = {'denoise_fn.' + k: v for k, v in sd64.items()}
    betas = R.betas64(**{'schedule': R.LOOP_SCHEDULE['schedule'], 'n': R.LOOP_SCHEDULE['n_timestep'],
                         'start': R.LOOP_SCHEDULE['linear_start'], 'end': R.LOOP_SCHEDULE['linear_end']})
    kept = R.sample(sdg, cond.double(), noise, betas, R.SMALL, keep=True)
    e_loop = rel(torch.cat(kept, dim=0), stacks[True])
    assert torch.equal(stacks[True][-1], stacks[False])
    np.savez_compressed(os.path.join(GOLD, 'gdp_loop.npz'), noise=noise.numpy(), final=stacks[False].numpy(),
                        stack=stacks[True].numpy())
    print('6-step loop: %d draws, fp64 restatement vs reference stack %.3e; final %s, stack %s' % (
        len(drawn), e_loop, tuple(stacks[False].shape), tuple(stacks[True].shape)))

    sched = {}
    for tag, opt in (('linear1000', dict(schedule='linear', n_timestep=1000, linear_start=1e-4, linear_end=2e-2)),
                     ('cosine50', dict(schedule='cosine', n_timestep=50, linear_start=1e-4, linear_end=2e-2))):
        D = diffusion.GaussianDiffusion(None, image_size=12)
        D.set_new_noise_schedule(opt, 'cpu')
        for k, v in D.state_dict().items():
            sched['%s.%s' % (tag, k)] = v.numpy()
    np.savez_compressed(os.path.join(GOLD, 'gdp_schedule.npz'), **sched)

    cfg_path = os.path.join(GDP, 'config', 'gdp_test_54_216.json')
    shutil.copyfile(cfg_path, os.path.join(GOLD, 'gdp_test_54_216.json'))
    u = load_config(cfg_path)['model']['unet']
    with torch.device('meta'):
        full = unet.UNet(in_channel=u['in_channel'], out_channel=u['out_channel'], norm_groups=32, inner_channel=u['inner_channel'],
                         channel_mults=u['channel_multiplier'], attn_res=u['attn_res'], res_blocks=u['res_blocks'],
                         dropout=u['dropout'], image_size=216)
    fsd = full.state_dict()
    keys = sorted(fsd)
    width = max(len(fsd[k].shape) for k in keys)
    shapes = np.array([list(fsd[k].shape) + [0] * (width - len(fsd[k].shape)) for k in keys], dtype=np.int32)
    count = sum(p.numel() for p in full.parameters())
    np.savez_compressed(os.path.join(GOLD, 'gdp_full.npz'), keys=np.array(keys), shapes=shapes, params=np.int64(count))
    print('full configuration: %d keys, %d parameters' % (len(keys), count))
    for f in ('gdp_small.npz', 'gdp_loop.npz', 'gdp_schedule.npz', 'gdp_full.npz', 'gdp_test_54_216.json'):
        print('%s: %.1f KB' % (f, os.path.getsize(os.path.join(GOLD, f)) / 1024.0))


if __name__ == '__main__':
    main()
