"""Generate tests/golden/gen_ablation.npz by running the REFERENCE model/sradsgan.py GeneratorResNet (build container only; the stub
import of oracle/make_golden.py) for the attention ablations of tests/attn_variants_ref.GEN_CONFIGS: 2 groups x 1 block, x2, a
(2, 3, 12, 12) input, det_init_ weights.

Per configuration: the state_dict keys (in order) and shapes, the digest of the output, and a digest of every parameter gradient for
the cotangent det_fill(tag + '.dy') (attn_variants_ref.small_digest).  Digests only.  tests/test_attn_variants_ref_cpu.py holds the
oracle (oracle/sradsgan_ref.py) and the HIP modules' state_dict layout to these records."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import make_golden as MG  # noqa: E402
from oracle import sradsgan_ref as O  # noqa: E402
from tests import attn_variants_ref as V  # noqa: E402


def main():
    torch.set_num_threads(8)
    ref = MG.import_reference()
    out = {'configs': np.array([V.gen_tag(c) for c in V.GEN_CONFIGS])}
    for cfg in V.GEN_CONFIGS:
        tag = V.gen_tag(cfg)
        y, g = V.gen_run(ref.GeneratorResNet(ref.ResGroup, **V.gen_kwargs(cfg)), cfg)
        sd = g.state_dict()
        out[tag + '/keys'] = np.array(list(sd.keys()))
        out[tag + '/shapes'] = np.array([','.join(map(str, v.shape)) for v in sd.values()])
        out[tag + '/y'] = O.digest(y)
        for k, p in g.named_parameters():
            out[tag + '/grad/' + k] = V.small_digest(p.grad)
        print('%-44s %3d keys  |y| max %.4f' % (tag, len(sd), float(y.abs().max())))
    path = os.path.join(ROOT, 'tests', 'golden', 'gen_ablation.npz')
    np.savez_compressed(path, **out)
    print('%s %.1f KB' % (path, os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
