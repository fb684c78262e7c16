"""The reference's trainer surface on the HIP path: `SRADSGAN(args)` with `.train()`, `.validate()`,
`.mfeNew_validate()` and the save/load helpers of SRADSGAN/model/sradsgan.py:511-1391, so `main_sradsgan.py`'s
    net = SRADSGAN(args); net.train(); net.mfeNew_validate(epoch=.., modelpath=..)
keeps working with the import changed.  Same argparse field names and defaults
(main_sradsgan.py:16-61, `default_args`), same loss weights / optimiser settings / step order (TrainStep), same
checkpoint names and log lines, same epoch control (PlateauRollback).

The data side: like the reference (`load_dataset`, sradsgan.py:643-656) the trainer builds its loaders from
`args.data_dir / train_dataset / test_dataset` when none are injected -- the same directory walk and file order
(data/data.py:295-346), but as `data.TileFolder` + `data.DevicePrefetcher`: uint8 HR tiles decoded by worker threads,
copied on their own HIP stream, and turned into (lr, hr, bc) on the device (sradsgan_amd.data.training_batch /
test_batch, bit-exact with the reference's PIL transforms) instead of 16 PIL worker processes.  An injected iterable
(`train_loader`, `test_loader`: the reference's own DataLoader tuples `(lr, hr, bc, paths)` or uint8 HR tiles
`[N, H, W, 3]`) takes precedence.  Metrics are computed on the device (validate.py).  LPIPS (sradsgan.py:561) is computed when it is
configured: `args.lpips_alexnet` (a torchvision AlexNet state-dict file, the user's to supply) together with `args.lpips_lin` (the
reference's utils/PerceptualSimilarity/weights/v0.1/alex.pth), or `set_lpips(model)` with a loaded sradsgan_amd.lpips.LPIPS.  Not
configured, the lpips slots of the returned tuples and log lines carry NaN and the epoch control sees 10000.  PNG panels are not
written."""
import argparse
import math
import os
import time
from collections import OrderedDict

import numpy as np
import torch

from . import checkpoint as ckpt
from . import data as sdata
from . import degrade as sdegrade
from . import dp
from . import contrast as scontrast
from . import lpips as slpips
from . import ops
from . import validate as sval
from .ensemble import SelfEnsemble
from .model import Discriminator, FeatureExtractor, GeneratorResNet, PatchDiscriminator, ResGroup
from .model.discriminators import NORM_TYPES
from .model.spectral import SpectralPatchDiscriminator, spectral_init_
from .train_step import TrainStep


def default_args(**overrides):
    """argparse.Namespace with the reference's flag names and defaults (main_sradsgan.py:16-61)."""
    d = dict(model_name='SRADSGAN', root_dir='.', data_dir='.', train_dataset=['AID', 'DOTA', 'LoveDA', 'RSSCN7_2800', 'SECOND'],
             test_dataset=['UCMerced_LandUse'], crop_size=216, num_threads=16, num_channels=3, scale_factor=8, epoch=0,
             num_epochs=100, save_epochs=1, batch_size=16, test_batch_size=1, save_dir='Result', lr=0.0002, b1=0.9, b2=0.999,
             gpu_mode=True, test_crop_size=216, n_cpu=16, hr_height=216, hr_width=216, sample_interval=1000, clip_value=0.01,
             lambda_gp=10, gp=True, penalty_type='LS', grad_penalty_Lp_norm='L2', relativeGan=False, loss_Lp_norm='L1',
             weight_content=1e-2, weight_gan=1e-3, max_train_samples=40000, is_train=True,
             # not in main_sradsgan.py: the augmentation Dataset.__getitem__ offers (data.Augment; all off = no Augment is built)
             # and x8 geometric self-ensemble at validation (ensemble.SelfEnsemble)
             augment_random_crop=False, augment_rotate=False, augment_fliplr=False, augment_fliptb=False, augment_noise=None,
             augment_seed=None, self_ensemble=False,
             # not in main_sradsgan.py either: the blur-and-noise degradation of model/util.py (degrade.SRMDPreprocessing) in place
             # of plain bicubic LR; degrade_blur off = nothing is built.  degrade_noise_high 0.0 = no noise kernel is launched
             degrade_blur=False, degrade_kernel=21, degrade_random=True, degrade_sig=2.6, degrade_sig_min=0.2, degrade_sig_max=4.0,
             degrade_rate_iso=1.0, degrade_scaling=3, degrade_noise_high=0.0, degrade_rate_cln=0.2, degrade_seed=None,
             degrade_eval=False,
             # not in main_sradsgan.py: validation numbers by the papers' protocol (sradsgan_amd.metrics) beside the reference trainer's
             # own; 'reference' = nothing new runs.  eval_crop_border None = scale_factor
             eval_protocol='reference', eval_crop_border=None, eval_y_channel=True,
             # not in main_sradsgan.py: weight_lpips * LPIPS(gen_hr, imgs_hr) in the generator's loss (lpips.LPIPS.loss; needs the
             # weights of lpips_alexnet + lpips_lin, or set_lpips); 0.0 = no LPIPS code runs in the step
             weight_lpips=0.0,
             # not in main_sradsgan.py: weight_contrast * the reference's contrastive VGG19 loss (model/loss.py:173-263) of (gen_hr,
             # imgs_hr, the batch's bicubic image) in the generator's loss; contrast_loss 'l1' = ContrastLoss, 'cosine' =
             # ContrastCosineLoss; contrast_vgg19 = a torchvision VGG19 state-dict file (or set_contrast); 0.0 = none of it runs
             weight_contrast=0.0, contrast_loss='l1', contrast_ablation=False, contrast_vgg19=None)
    d.update(overrides)
    return argparse.Namespace(**d)


def weights_init_normal(m, mean=0.0, std=0.02):
    """utils/utils.py:97-114 (applied at sradsgan.py:713-714)."""
    # written through the parameters themselves, not `.data`: the write moves their version, which is what the packed weight images of a
    # net that has already run are refreshed by (ops.packed_weight)
    name = m.__class__.__name__
    with torch.no_grad():
        if name.find('Linear') != -1 or name.find('Conv2d') != -1 or name.find('ConvTranspose2d') != -1:
            m.weight.normal_(mean, std)
            if m.bias is not None:
                m.bias.zero_()
        elif name.find('BatchNorm') != -1:
            m.weight.normal_(1.0, 0.02)
            if m.bias is not None:
                m.bias.zero_()


ATTENTION_MODES = ('',) + tuple(ops.TAIL_ORDERS)       # la_mode / ga_mode of sradsgan.py:215-324, 365-439: '', CA-SA, SA-CA, CA, SA, CA|SA
POOL_MODES = ops.POOL_MODES


def attention_ablation(args):
    """The generator's attention-ablation switches (sradsgan.py:420-439) read from `args`, absent ones at the values the reference's
    trainer hard-codes (:669-671): a dict of GeneratorResNet keyword arguments.  A value outside the reference's vocabulary would
    build a generator that silently has no attention at all (its constructors test `'CA' in mode`), so it is a ValueError here."""
    opts = dict(rla_mode=getattr(args, 'rla_mode', 'CA-SA'), bla_mode=getattr(args, 'bla_mode', 'CA-SA'),
                ga_mode=getattr(args, 'ga_mode', 'CA-SA'), pool_mode=getattr(args, 'pool_mode', 'Avg|Max'),
                addconv=getattr(args, 'addconv', True))
    for name in ('rla_mode', 'bla_mode', 'ga_mode'):
        if opts[name] not in ATTENTION_MODES:
            raise ValueError('args.%s must be one of %r, got %r' % (name, ATTENTION_MODES, opts[name]))
    if opts['pool_mode'] not in POOL_MODES:
        raise ValueError('args.pool_mode must be one of %r, got %r' % (POOL_MODES, opts['pool_mode']))
    if not isinstance(opts['addconv'], bool):
        raise ValueError('args.addconv must be a bool, got %r' % (opts['addconv'],))
    return opts


EVAL_PROTOCOLS = ('reference', 'published')


def evaluation_protocol(args):
    """The validation protocol read from `args`, absent fields at their defaults: None for eval_protocol 'reference' -- the reference
    trainer's own numbers and nothing else -- or, for 'published', the dict(crop_border, y_channel) that validate.evaluate takes to add
    the papers' PSNR / SSIM (sradsgan_amd.metrics): `eval_crop_border` pixels shaved from every border (default scale_factor) and, with
    `eval_y_channel` (default True), the BT.601 luma instead of RGB.  Anything else is a ValueError."""
    name = getattr(args, 'eval_protocol', 'reference')
    if name not in EVAL_PROTOCOLS:
        raise ValueError('args.eval_protocol must be one of %r, got %r' % (EVAL_PROTOCOLS, name))
    crop, y = getattr(args, 'eval_crop_border', None), getattr(args, 'eval_y_channel', True)
    if crop is None:
        crop = args.scale_factor
    if isinstance(crop, bool) or not isinstance(crop, int) or crop < 0:
        raise ValueError('args.eval_crop_border must be None or a non-negative integer, got %r' % (crop,))
    if not isinstance(y, bool):
        raise ValueError('args.eval_y_channel must be a bool, got %r' % (y,))
    return None if name == 'reference' else dict(crop_border=crop, y_channel=y)


def training_augment(args, rank=0):
    """The data.Augment that `args.augment_*` ask for -- the crop / noise / rotation / flips of Dataset.__getitem__ (dataset.py:273-306)
    for uint8 training tiles -- or None when every switch is off (absent fields are off): then nothing is built and the trainer's
    batches are the un-augmented ones."""
    flags = dict(random_crop=bool(getattr(args, 'augment_random_crop', False)), rotate=bool(getattr(args, 'augment_rotate', False)),
                 fliplr=bool(getattr(args, 'augment_fliplr', False)), fliptb=bool(getattr(args, 'augment_fliptb', False)),
                 noise=getattr(args, 'augment_noise', None))
    if not any(flags.values()):
        return None
    return sdata.Augment(args.crop_size, args.scale_factor, seed=getattr(args, 'augment_seed', None), rank=rank, **flags)


def training_degrade(args, rank=0, test=False):
    """The degrade.SRMDPreprocessing that `args.degrade_*` ask for -- per-sample Gaussian blur, bicubic down-sampling and noise of
    model/util.py for uint8 training tiles -- or None when `degrade_blur` is off (an absent field is off): then nothing is built and
    the trainer's batches are the plain bicubic ones.  test=True: the object for the test set, built only with `degrade_eval` on,
    with the stable kernel of deviation `degrade_sig` and no noise, so that an evaluation is reproducible."""
    if not getattr(args, 'degrade_blur', False) or (test and not getattr(args, 'degrade_eval', False)):
        return None
    g = lambda name, default: getattr(args, 'degrade_' + name, default)
    noise_high = float(g('noise_high', 0.0))
    return sdegrade.SRMDPreprocessing(args.scale_factor, random=bool(g('random', True)) and not test, kernel=g('kernel', 21),
                                      noise=noise_high > 0.0 and not test, sig=g('sig', 2.6), sig_min=g('sig_min', 0.2),
                                      sig_max=g('sig_max', 4.0), rate_iso=g('rate_iso', 1.0), scaling=g('scaling', 3),
                                      rate_cln=g('rate_cln', 0.2), noise_high=noise_high, seed=g('seed', None), rank=rank)


class SRADSGAN(object):
    eval_label = 'sradsgan'          # metric key prefix of mfeNew_validate / mfeNew_validateByClass lines (bicubic_* / <label>_*)

    def __init__(self, args, train_loader=None, test_loader=None):
        for k in ('model_name', 'train_dataset', 'test_dataset', 'crop_size', 'test_crop_size', 'hr_height', 'hr_width',
                  'num_threads', 'num_channels', 'scale_factor', 'epoch', 'num_epochs', 'save_epochs', 'batch_size',
                  'test_batch_size', 'lr', 'b1', 'b2', 'data_dir', 'root_dir', 'save_dir', 'gpu_mode', 'n_cpu',
                  'sample_interval', 'clip_value', 'lambda_gp', 'gp', 'penalty_type', 'grad_penalty_Lp_norm',
                  'weight_gan', 'weight_content', 'max_train_samples'):                       # sradsgan.py:513-556
            setattr(self, k, getattr(args, k))
        self.relative = args.relativeGan
        self.loss_Lp_norm = args.loss_Lp_norm
        for name, value, choices in (('penalty_type', self.penalty_type, ('LS', 'hinge')),              # main_sradsgan.py:53-56 `choices`
                                     ('grad_penalty_Lp_norm', self.grad_penalty_Lp_norm, ('L2', 'L1', 'Linf')),
                                     ('loss_Lp_norm', self.loss_Lp_norm, ('L1', 'L2'))):
            if value not in choices:
                raise ValueError('--%s must be one of %s, got %r' % (name, choices, value))
        self.weight_lpips = getattr(args, 'weight_lpips', 0.0)
        if isinstance(self.weight_lpips, bool) or not isinstance(self.weight_lpips, (int, float)) or not self.weight_lpips >= 0:
            raise ValueError('args.weight_lpips must be a number >= 0, got %r' % (self.weight_lpips,))
        self.weight_contrast = getattr(args, 'weight_contrast', 0.0)
        if isinstance(self.weight_contrast, bool) or not isinstance(self.weight_contrast, (int, float)) or not self.weight_contrast >= 0:
            raise ValueError('args.weight_contrast must be a number >= 0, got %r' % (self.weight_contrast,))
        self.contrast_loss = getattr(args, 'contrast_loss', 'l1')
        if self.contrast_loss not in ('l1', 'cosine'):
            raise ValueError("args.contrast_loss must be 'l1' or 'cosine', got %r" % (self.contrast_loss,))
        self.contrast_ablation = bool(getattr(args, 'contrast_ablation', False))
        self.contrast_vgg19 = getattr(args, 'contrast_vgg19', None)                  # a state-dict path, see set_contrast
        self.contrast = None
        self._check_loss_options()
        self.attention = attention_ablation(args)
        self.eval_protocol = evaluation_protocol(args)          # None, or the papers' protocol beside the reference's (validation)
        # the discriminator's normalisation (base_networks.Discriminator's norm_type, the line the reference keeps as a comment at
        # sradsgan.py:672): absent / None = this trainer's own BatchNorm discriminator, else model.discriminators.PatchDiscriminator
        self.d_norm_type = getattr(args, 'd_norm_type', None)
        self.d_attention = bool(getattr(args, 'd_attention', False))
        if self.d_norm_type is not None and self.d_norm_type not in NORM_TYPES:
            raise ValueError('args.d_norm_type must be None or one of %r, got %r' % (NORM_TYPES, self.d_norm_type))
        # spectral normalisation of D's block convs (base_networks.Discriminator's use_spectralnorm): model.spectral.SpectralPatchDiscriminator.
        # The normalisation beside it must be said: the trainer's default D is the BatchNorm one, the reference class's default is '' --
        # no silent choice between the two
        self.d_spectralnorm = getattr(args, 'd_spectralnorm', False)
        if not isinstance(self.d_spectralnorm, bool):
            raise ValueError('args.d_spectralnorm must be a bool, got %r' % (self.d_spectralnorm,))
        if self.d_spectralnorm and self.d_norm_type is None:
            raise ValueError("args.d_spectralnorm needs an explicit args.d_norm_type, one of %r ('' = no normalisation beside the spectral one)"
                             % (NORM_TYPES,))
        if not torch.cuda.is_available():
            raise Exception('No GPU found, please run without --gpu_mode=False')               # main_sradsgan.py:95-96
        # generator depth: the reference hard-codes 12 groups x 3 blocks (:669-671); overridable for tests
        self.n_residual_blocks = getattr(args, 'n_residual_blocks', 12)
        self.n_basic_blocks = getattr(args, 'n_basic_blocks', 3)
        self.pretrained_generator = getattr(args, 'pretrained_generator', None)      # chain training, see _build
        self.pretrained_discriminator = getattr(args, 'pretrained_discriminator', None)
        self.train_loader, self.test_loader = train_loader, test_loader
        self.self_ensemble = bool(getattr(args, 'self_ensemble', False))            # validate / mfeNew_validate report the "+" numbers
        self.lpips = None
        self.lpips_alexnet = getattr(args, 'lpips_alexnet', None)                    # state-dict paths, see set_lpips
        self.lpips_lin = getattr(args, 'lpips_lin', None)
        if bool(self.lpips_alexnet) != bool(self.lpips_lin):
            raise ValueError('LPIPS needs both args.lpips_alexnet (torchvision AlexNet state dict) and args.lpips_lin (alex.pth)')
        # data parallel: one process per GPU under torch.distributed; replicas start identical (broadcast
        # from rank 0), gradients are averaged by TrainStep's GradSync, BatchNorm stays local, rank 0 owns files and
        # logs, validation results and with them every rollback decision are rank 0's
        self.rank, self.world = dp.rank_world()
        self.device = torch.device('cuda', torch.cuda.current_device())
        self.augment = training_augment(args, self.rank)                            # None unless an augmentation switch is on
        self.degrade = training_degrade(args, self.rank)                            # None unless args.degrade_blur is on
        self.degrade_test = training_degrade(args, self.rank, test=True)            # None unless args.degrade_eval is on as well
        self.generator = self.discriminator = self.feature_extractor = None
        self.step = None
        self.log_dict = OrderedDict()
        self.loss_log_path = os.path.join(self.save_dir, 'loss_log.txt')
        self.val_log_path = os.path.join(self.save_dir, 'val_log.txt')

    # (grad_penalty_Lp_norm, penalty_type) pairs the trainer runs: those with a recorded iteration of the reference to hold the
    # whole step against (tests/golden/train_small.npz, gan_options.npz).  TrainStep and ops.gp_penalty take all six.
    penalty_pairs = (('L2', 'LS'), ('L1', 'LS'), ('Linf', 'hinge'))

    def _check_loss_options(self):
        if (self.grad_penalty_Lp_norm, self.penalty_type) not in self.penalty_pairs:
            raise NotImplementedError('the trainer runs the penalties with a recorded reference iteration, (norm, penalty) in %s, got '
                                      '(%r, %r); TrainStep takes any pair (sradsgan.py:595-641)'
                                      % (self.penalty_pairs, self.grad_penalty_Lp_norm, self.penalty_type))

    # ------------------------------------------------------------------ networks ---------------- #
    def _new_generator(self):
        return GeneratorResNet(ResGroup, n_residual_blocks=self.n_residual_blocks, n_basic_blocks=self.n_basic_blocks,
                               upscale_factor=self.scale_factor, **self.attention)            # :669-671, :1263-1265

    def _new_discriminator(self):
        if getattr(self, 'd_spectralnorm', False):
            return SpectralPatchDiscriminator(norm_type=self.d_norm_type, attention=self.d_attention)
        if self.d_norm_type is None:
            return Discriminator()
        return PatchDiscriminator(norm_type=self.d_norm_type, attention=self.d_attention)

    def _build(self):
        self.generator = self._new_generator()
        self.discriminator = self._new_discriminator()
        self.feature_extractor = FeatureExtractor()
        model_dir = os.path.join(self.save_dir, 'model')
        if self.epoch != 0:                                                                     # :705-711
            self.load_epoch_network(model_dir + '/generator_param_epoch_%d.pkl' % self.epoch, self.generator, strict=True)
            self.load_epoch_network(model_dir + '/discriminator_param_epoch_%d.pkl' % self.epoch, self.discriminator, strict=True)
        else:
            self.generator.apply(weights_init_normal)                                           # :713-714
            if getattr(self, 'd_spectralnorm', False):
                spectral_init_(self.discriminator)              # (the reference's apply() raises for a spectral D: model/spectral.py)
            else:
                self.discriminator.apply(weights_init_normal)
            # chain training (:716-721, commented out in the reference and edited by hand per scale): start from the
            # previous scale's checkpoints.  strict=False there still raises on shape mismatches, so the partial load
            # is shape-aware (checkpoint.load_compatible): the up-sampler conv keeps its fresh init across 2^n <-> 3^n
            self.chain_report = {}
            for label, net in (('generator', self.generator), ('discriminator', self.discriminator)):
                path = getattr(self, 'pretrained_' + label, None)
                if path:
                    self.chain_report[label] = ckpt.load_compatible(net, torch.load(path, map_location='cpu'))
                    print('%s initialised from %s: %d tensors loaded, %d kept their init' % (
                        label, path, len(self.chain_report[label][0]),
                        len(self.chain_report[label][1]) + len(self.chain_report[label][2])))
        self.generator.to(self.device), self.discriminator.to(self.device), self.feature_extractor.to(self.device)
        self.feature_extractor.eval()                                                           # :727
        if self.world > 1:
            dp.broadcast_module(self.generator, 0), dp.broadcast_module(self.discriminator, 0)
            dp.broadcast_module(self.feature_extractor, 0)
            if getattr(self, 'grad_sync', None) is None:
                self.grad_sync = dp.GradSync(self.world)
            self._alpha_rng = np.random.RandomState(1234 + self.rank)                           # alpha drawn per rank
        loss_lpips = None
        if self.weight_lpips > 0:                       # the perceptual term of the generator's loss: the metric's model, as a loss
            loss_lpips = self._lpips_model()
            if loss_lpips is None:
                raise ValueError('args.weight_lpips = %r needs LPIPS weights: args.lpips_alexnet + args.lpips_lin, or set_lpips(model) '
                                 'before training' % (self.weight_lpips,))
            if self.world > 1:
                dp.broadcast_module(loss_lpips, 0)
        loss_contrast = None
        if self.weight_contrast > 0:                    # the contrastive term of the generator's loss
            loss_contrast = self._contrast_model()
            if loss_contrast is None:
                raise ValueError('args.weight_contrast = %r needs VGG19 weights: args.contrast_vgg19, or set_contrast(model) before '
                                 'training' % (self.weight_contrast,))
            if self.world > 1:
                dp.broadcast_module(loss_contrast, 0)
        self.step = TrainStep(self.generator, self.discriminator, self.feature_extractor, lr=self.lr, b1=self.b1, b2=self.b2,
                              weight_content=self.weight_content, weight_gan=self.weight_gan, lambda_gp=self.lambda_gp,
                              clip_value=self.clip_value, use_gp=bool(self.gp), grad_sync=getattr(self, 'grad_sync', None),
                              penalty_type=self.penalty_type, grad_penalty_Lp_norm=self.grad_penalty_Lp_norm,
                              loss_Lp_norm=self.loss_Lp_norm, relative=bool(self.relative), lpips=loss_lpips,
                              weight_lpips=float(self.weight_lpips), contrast=loss_contrast,
                              weight_contrast=float(self.weight_contrast))

    def _batch(self, item, test=False):
        """(lr, hr, bc) device float tensors from a loader item: the reference's 4-tuple, a uint8 HR batch [B,H,W,3],
        or data.DevicePrefetcher's (uint8 batch, file names).  uint8 tiles get the reference's per-sample transforms
        on the device: bicubic LR for training (dataset.py:418-436), bilinear LR for the test set (data.py:329-343) -- or, with
        args.degrade_blur on, the blurred and noisy LR of degrade.SRMDPreprocessing (the test set only with args.degrade_eval)."""
        if isinstance(item, (tuple, list)) and len(item) == 2 and torch.is_tensor(item[0]) and item[0].dtype == torch.uint8:
            item = item[0]
        if torch.is_tensor(item) and item.dtype == torch.uint8:
            degrade = getattr(self, 'degrade_test' if test else 'degrade', None)
            if degrade is not None:                                                 # blurred (and noisy) LR instead of plain bicubic
                return sdegrade.degraded_training_batch(item.to(self.device), self.scale_factor, degrade,
                                                        augment=None if test else getattr(self, 'augment', None))
            if not test and getattr(self, 'augment', None) is not None:              # training tiles only, never the test set
                return sdata.augmented_training_batch(item.to(self.device), self.scale_factor, self.augment)
            make = sdata.test_batch if test else sdata.training_batch
            return make(item.to(self.device), self.scale_factor)
        lr, hr, bc = item[0], item[1], item[2]
        return lr.to(self.device).float(), hr.to(self.device).float(), bc.to(self.device).float()

    # ------------------------------------------------------------------ datasets ---------------- #
    def load_dataset(self, dataset='train', max_samples=20000, dirs=None):
        """sradsgan.py:643-656: DataLoader(shuffle=True, drop_last=True) over the training folders resp.
        DataLoader(shuffle=False, drop_last=True) over the test folders of `args.data_dir`, as a device prefetcher of
        uint8 tiles.  `dirs` overrides the directory list (per-class validation)."""
        if self.num_channels == 1:
            raise NotImplementedError('load_dataset: RGB tiles only (num_channels=3 is what main_sradsgan.py passes)')
        if dataset == 'train':
            print('Loading train dct_datasets...')
            folders = sdata.rgb_train_dirs(self.data_dir, self.train_dataset) if dirs is None else dirs
            tiles = sdata.TileFolder(folders, crop_size=self.crop_size, scale_factor=self.scale_factor)
            return sdata.DevicePrefetcher(tiles, self.batch_size, self.device, shuffle=True, drop_last=True,
                                          num_workers=self.num_threads, rank=self.rank, world=self.world)
        if dataset == 'test':
            print('Loading test dct_datasets...')
            folders = sdata.rgb_test_dirs(self.data_dir, self.test_dataset) if dirs is None else dirs
            tiles = sdata.TileFolder(folders, crop_size=self.crop_size, scale_factor=self.scale_factor)
            return sdata.DevicePrefetcher(tiles, self.test_batch_size, self.device, shuffle=False, drop_last=True,
                                          num_workers=self.num_threads)
        raise ValueError("load_dataset: dataset must be 'train' or 'test'")

    # ------------------------------------------------------------------ training ---------------- #
    def train(self):
        """sradsgan.py:658-1036.  Returns the per-epoch history (avg losses and validation metrics)."""
        if self.train_loader is None:
            self.train_loader = self.load_dataset(dataset='train', max_samples=self.max_train_samples)    # :749
        if self.test_loader is None:
            self.test_loader = self.load_dataset(dataset='test')                                          # :750
        os.makedirs(self.save_dir, exist_ok=True)
        self._build()
        model_dir = os.path.join(self.save_dir, 'model')
        control = ckpt.PlateauRollback(self.lr)
        avg_loss_G, avg_loss_D, history = [], [], []
        step_count = 0
        epoch = self.epoch
        start_time = time.time()
        while control.keep_training(epoch, self.num_epochs):                                    # :803
            self.generator.train()
            self.discriminator.train()
            epoch_loss_G = epoch_loss_D = 0.0
            n_batches = 0
            for i, item in enumerate(self.train_loader):
                imgs_lr, imgs_hr, imgs_bc = self._batch(item)
                rng = getattr(self, '_alpha_rng', None) or np.random
                alpha = torch.from_numpy(rng.random_sample((imgs_hr.size(0), 1, 1, 1))).float().to(self.device)   # :609
                if self.weight_contrast > 0:                                                    # the negative is the batch's bicubic image
                    out = self.step(imgs_lr, imgs_hr, alpha, negatives=imgs_bc)
                else:
                    out = self.step(imgs_lr, imgs_hr, alpha)                                    # :829-892
                step_count += 1
                n_batches += 1
                if (i + 1) % self.sample_interval == 0 or i == 0:                               # host reads only at log cadence
                    lg, ld = float(out['loss_G']), float(out['loss_D'])
                    self.log_dict['loss_G'], self.log_dict['loss_D'] = lg, ld
                    if 'lpips' in out:                                                          # only with args.weight_lpips > 0
                        self.log_dict['lpips'] = float(out['lpips'])
                    if 'contrast' in out:                                                       # only with args.weight_contrast > 0
                        self.log_dict['contrast'] = float(out['contrast'])
                    rlt = OrderedDict(model=self.model_name, epoch=epoch, iters=step_count, time=time.time() - start_time)
                    rlt.update(self.log_dict)
                    if self.rank == 0:
                        print(sval.append_log(self.loss_log_path, 'train', rlt))               # :898-906, 963-969
                epoch_loss_G = epoch_loss_G + out['loss_G']
                epoch_loss_D = epoch_loss_D + out['loss_D']
            avg_loss_G.append(float(epoch_loss_G) / max(n_batches, 1))                          # :975-976
            avg_loss_D.append(float(epoch_loss_D) / max(n_batches, 1))
            val = self.validate(epoch=epoch, mode='train', save_img=((epoch + 1) % self.save_epochs == 0))   # :978
            val = tuple(dp.broadcast_floats(val, 0, self.device))                               # rank 0's numbers decide
            history.append(dict(epoch=epoch, loss_G=avg_loss_G[-1], loss_D=avg_loss_D[-1], psnr=val[0], ssim=val[1],
                                ergas=val[2], lpips=val[3]))
            if self.rank == 0:
                self.save_epoch_network(save_dir=model_dir, network=self.generator, network_label='generator', iter_label=epoch + 1)
                self.save_epoch_network(save_dir=model_dir, network=self.discriminator, network_label='discriminator', iter_label=epoch + 1)
            dp.barrier()                                                                        # files exist before any rank rolls back
            reload_g = lambda n: self.load_epoch_network(model_dir + '/generator_param_epoch_%d.pkl' % n, self.generator)
            epoch, rolled = control.update(epoch, val[0], val[1], val[2], val[3] if not math.isnan(val[3]) else 10000,
                                           step=self.step, on_rollback=reload_g)               # :985-1036
            self.lr = control.lr
            if rolled:
                print('optimizer_G_Learning rate decay: lr={}'.format(self.step.lr_G))
        if self.rank == 0:
            self.save_model(epoch=None)
        dp.barrier()
        return history

    # ------------------------------------------------------------------ validation -------------- #
    def set_lpips(self, model):
        """Use `model` (a loaded sradsgan_amd.lpips.LPIPS, or None to switch the metric off) as `self.lpips_metric` of the reference
        (sradsgan.py:561)."""
        self.lpips = None if model is None else model.to(self.device)

    def set_contrast(self, model):
        """Use `model` (one of sradsgan_amd.contrast's single-negative losses with its VGG19 weights loaded, or None) as the contrastive
        term of the generator's loss (args.weight_contrast > 0)."""
        self.contrast = None if model is None else model.to(self.device)

    def _contrast_model(self):
        if self.contrast is None and self.contrast_vgg19:
            cls = scontrast.ContrastLoss if self.contrast_loss == 'l1' else scontrast.ContrastCosineLoss
            model = cls(ablation=self.contrast_ablation)
            model.vgg.load_torchvision_vgg19(torch.load(self.contrast_vgg19, map_location='cpu'))
            self.set_contrast(model)
        return self.contrast

    def _lpips_model(self):
        if self.lpips is None and self.lpips_alexnet:
            model = slpips.LPIPS()
            model.load_torchvision_alexnet(torch.load(self.lpips_alexnet, map_location='cpu'))
            model.load_lin(torch.load(self.lpips_lin, map_location='cpu'))
            self.set_lpips(model)
        return self.lpips

    def _evaluate_loader(self, generator, label, loader=None, totals=None):
        if loader is None:
            if self.test_loader is None:
                self.test_loader = self.load_dataset(dataset='test')                              # :1074, :1277
            loader = self.test_loader
        sums = {k: 0.0 for k in ('bicubic_mse', 'bicubic_psnr', 'bicubic_ssim', 'bicubic_ergas', label + '_mse', label + '_psnr',
                                 label + '_ssim', label + '_ergas')}
        lpips = self._lpips_model()
        metrics = ('mse', 'psnr', 'ssim', 'ergas') + (() if lpips is None else ('lpips',))
        if lpips is not None:
            sums['bicubic_lpips'] = sums[label + '_lpips'] = 0.0
        protocol = getattr(self, 'eval_protocol', None)
        if protocol is not None:
            metrics += ('pub_psnr', 'pub_ssim')
            for prefix in ('bicubic', label):
                sums[prefix + '_pub_psnr'] = sums[prefix + '_pub_ssim'] = 0.0
        img_num = 0
        was_training, inner = generator.training, generator
        if getattr(self, 'self_ensemble', False):                                                # the "+" protocol: 8 views, merged
            generator = SelfEnsemble(inner)
        generator.eval()                                                                         # :1288
        start = time.time()
        for item in loader:
            imgs_lr, imgs_hr, imgs_bc = self._batch(item, test=True)
            out = sval.evaluate(generator, imgs_lr, imgs_hr, self.scale_factor, bicubic=imgs_bc, lpips=lpips, protocol=protocol)
            img_num += imgs_hr.size(0)
            for k in metrics:
                sums['bicubic_' + k] += float(out['bicubic'][k].sum())
                sums[label + '_' + k] += float(out['sr'][k].sum())
        inner.train(was_training)
        if totals is not None:                                                                   # running sums over classes
            totals['num'] = totals.get('num', 0) + img_num
            for k, v in sums.items():
                totals[k] = totals.get(k, 0.0) + v
        avg = {k: v / max(img_num, 1) for k, v in sums.items()}                                 # :1365-1374
        return avg, time.time() - start

    def _log_val(self, epoch, avg, elapsed, label, model=None):
        rlt = OrderedDict(model=self.model_name if model is None else model, epoch=epoch, iters=epoch, time=elapsed)
        for prefix in ('bicubic', label):                                                        # :1377-1390 key order
            for k in ('mse', 'psnr', 'ssim', 'ergas'):
                rlt['%s_%s' % (prefix, k)] = avg['%s_%s' % (prefix, k)]
            rlt['%s_lpips' % prefix] = avg.get('%s_lpips' % prefix, float('nan'))
            if getattr(self, 'eval_protocol', None) is not None:                                 # the papers' numbers, after the LPIPS slot
                for k in ('pub_psnr', 'pub_ssim'):
                    rlt['%s_%s' % (prefix, k)] = avg['%s_%s' % (prefix, k)]
        if self.rank != 0:
            return
        os.makedirs(self.save_dir, exist_ok=True)
        print(sval.append_log(self.val_log_path, 'val', rlt))

    def validate(self, epoch=0, mode='test', save_img=False):
        """sradsgan.py:1058-1194 -> (psnr, ssim, ergas, lpips) averaged over the test set."""
        if mode == 'test':
            self.generator = self._new_generator().to(self.device)                              # :1065-1067
            self.load_epoch_model(epoch)
        avg, elapsed = self._evaluate_loader(self.generator, 'srcnn')
        self._log_val(epoch, avg, elapsed, 'srcnn')
        return avg['srcnn_psnr'], avg['srcnn_ssim'], avg['srcnn_ergas'], avg.get('srcnn_lpips', float('nan'))

    def mfeNew_validate(self, epoch=100, modelpath=None):
        """sradsgan.py:1258-1391: fresh generator, optional `modelpath` (strict=False), same averages and log line
        (keys bicubic_* / <eval_label>_*)."""
        self.generator = self._new_generator().to(self.device)
        if modelpath is not None:
            self.generator.load_state_dict(torch.load(modelpath, map_location='cpu'), strict=False)   # :1270-1271
            ckpt._after_load()
        avg, elapsed = self._evaluate_loader(self.generator, self.eval_label)
        self._log_val(epoch, avg, elapsed, self.eval_label)
        return (avg[self.eval_label + '_psnr'], avg[self.eval_label + '_ssim'], avg[self.eval_label + '_ergas'],
                avg.get(self.eval_label + '_lpips', float('nan')))

    def mfeNew_validateByClass(self, epoch, save_img=False, modelpath=None):
        """sradsgan.py:1393-1601: the validation of mfeNew_validate once per class folder of the test set, one
        `val_log.txt` line per class (model = class name) and a final "Total" line over all images.  Like the
        reference one loader per class directory of the test set is built (:1433-1447) unless `self.class_loaders` (an
        ordered mapping class name -> iterable of batches) was injected.  Returns {class or 'Total': averages}."""
        loaders = getattr(self, 'class_loaders', None)
        if not loaders:                                                                          # :1430-1447
            loaders = OrderedDict()
            for d in sdata.rgb_test_dirs(self.data_dir, self.test_dataset):
                loaders[os.path.split(d)[-1]] = self.load_dataset(dataset='test', dirs=[d])
                print('Number of val images in [{:s}]: {:d}'.format(d, len(loaders[os.path.split(d)[-1]])))
        self.generator = self._new_generator().to(self.device)
        if modelpath is not None:
            self.generator.load_state_dict(torch.load(modelpath, map_location='cpu'), strict=False)   # :1400-1401
            ckpt._after_load()
        start, totals, result = time.time(), {}, OrderedDict()
        for name, loader in loaders.items():
            avg, _ = self._evaluate_loader(self.generator, self.eval_label, loader=loader, totals=totals)
            self._log_val(epoch, avg, time.time() - start, self.eval_label, model=name)              # :1548-1564
            result[name] = avg
        num = max(totals.pop('num', 0), 1)
        result['Total'] = {k: v / num for k, v in totals.items()}                               # :1568-1577
        self._log_val(epoch, result['Total'], time.time() - start, self.eval_label, model='Total')
        return result

    def mfe_test_single(self, img_fn, modelpath=None):
        """sradsgan.py:1603-1641: centre-crop `test_crop_size` of one image file, super-resolve it, and write
        `SR_SRADSGAN_<name>` and `SR_Bicubic_<name>` into save_dir with save_img1's quantisation (x255, clamp, truncate;
        utils/utils.py:169-187).  The bicubic image is img_interp's (utils.py:755-780: uint8 via ToPILImage, Pillow
        bicubic) on the device.  The comparison figure (matplotlib) is not drawn.  Returns the two uint8 HWC arrays."""
        from PIL import Image
        import numpy as np
        self.generator = self._new_generator().to(self.device)
        if modelpath is not None:
            self.generator.load_state_dict(torch.load(modelpath, map_location='cpu'), strict=False)   # :1609-1610
            ckpt._after_load()
        self.generator.eval()
        img = Image.open(img_fn).convert('RGB')
        c = self.test_crop_size
        left, top = int(round((img.width - c) / 2.0)), int(round((img.height - c) / 2.0))          # transforms.CenterCrop
        u8 = torch.from_numpy(np.asarray(img.crop((left, top, left + c, top + c)), dtype=np.uint8).copy())
        u8 = u8.unsqueeze(0).contiguous().to(self.device)                                        # [1,c,c,3] uint8
        x = sdata.to_tensor(u8)
        gen = self.generator
        if getattr(self, 'self_ensemble', False):
            gen = SelfEnsemble(gen)
        with torch.no_grad():
            sr = gen(x)
        bc_u8 = sdata.resize_u8(u8, c * self.scale_factor, c * self.scale_factor, 'bicubic')[0]  # [H,W,3]
        sr_u8 = (sr[0] * 255.0).clamp(0, 255).to(torch.uint8).permute(1, 2, 0)                   # save_img1
        os.makedirs(self.save_dir, exist_ok=True)
        name = os.path.basename(img_fn)
        out = []
        for tag, t in (('SRADSGAN', sr_u8), ('Bicubic', bc_u8)):
            arr = t.contiguous().cpu().numpy()
            Image.fromarray(arr).save(os.path.join(self.save_dir, 'SR_%s_%s' % (tag, name)))
            out.append(arr)
        return tuple(out)

    def mfe_test_scene(self, img_fn, modelpath=None, tile=None, overlap=None):
        """A whole image file, however large, instead of mfe_test_single's centre crop (no counterpart in the reference):
        the file is super-resolved in overlapping LR tiles of side `tile` (default crop_size // scale_factor, the LR size
        the generator was trained on) that overlap by `overlap` (default tile // 4), blended with feathered seams on the
        device (sradsgan_amd.scene) and written as `SR_<model_name>_<name>` into save_dir with save_img1's quantisation.
        Tiling approximates a whole-scene forward -- attention sees one tile at a time; the feather hides the seams, it
        does not remove the difference.  Returns the uint8 HWC array [H * scale, W * scale, 3]."""
        from PIL import Image
        from . import scene as sscene
        self.generator = self._new_generator().to(self.device)
        if modelpath is not None:
            self.generator.load_state_dict(torch.load(modelpath, map_location='cpu'), strict=False)
            ckpt._after_load()
        self.generator.eval()
        u8 = torch.from_numpy(np.asarray(Image.open(img_fn).convert('RGB'), dtype=np.uint8).copy())
        tile = self.crop_size // self.scale_factor if tile is None else tile
        overlap = tile // 4 if overlap is None else overlap
        arr = sscene.super_resolve_scene(self.generator, u8, self.scale_factor, tile, overlap).cpu().numpy()
        os.makedirs(self.save_dir, exist_ok=True)
        Image.fromarray(arr).save(os.path.join(self.save_dir, 'SR_%s_%s' % (self.model_name, os.path.basename(img_fn))))
        return arr

    def mfe_classify_scenes(self, hr_u8_batches, labels, vgg, head, means, mode='sr', modelpath=None):
        """Scene_classification_mfe.py's evaluate() for this trainer's model and scale (sradsgan_amd.classify.classify_sr): the HR
        uint8 tiles are down-sampled, super-resolved by a fresh generator (optional `modelpath`, strict=False), quantised like
        save_img1 and classified by `head` on `vgg`'s bottleneck features, all on the device.  mode 'bicubic' / 'lr' give the
        script's baseline rows.  Returns {accuracy, confusion [true, pred], report, pred}."""
        from . import classify as sclassify
        self.generator = self._new_generator().to(self.device)
        if modelpath is not None:
            self.generator.load_state_dict(torch.load(modelpath, map_location='cpu'), strict=False)
            ckpt._after_load()
        self.generator.eval()
        return sclassify.classify_sr(self.generator, self.scale_factor, hr_u8_batches, labels, vgg, head, means, mode=mode)

    # ------------------------------------------------------------------ checkpoints ------------- #
    def save_epoch_network(self, save_dir, network, network_label, iter_label):
        return ckpt.save_epoch_network(save_dir, network, network_label, iter_label)

    def load_epoch_network(self, load_path, network, strict=True):
        ckpt.load_epoch_network(load_path, network, strict=strict)
        print('Trained model is loaded.')

    def save_model(self, epoch=None):
        ckpt.save_model(self.save_dir, self.generator, self.discriminator, epoch)
        print('Trained model is saved.')

    def load_model(self):
        ok = ckpt.load_model(self.save_dir, self.generator)
        print('Trained model is loaded.' if ok else 'No model exists to load.')
        return ok

    def load_epoch_model(self, epoch):
        path = os.path.join(self.save_dir, 'model', 'generator_param_epoch_%d.pkl' % epoch)
        if not os.path.exists(path):
            print('No model exists to load.')
            return False
        ckpt.load_epoch_network(path, self.generator)
        print('Trained model is loaded.')
        return True


def chain_train(args, scales, loaders, trainer_cls=SRADSGAN):
    """BASELINE configs[4]: the multi-scale chain x2 -> x3 -> x4 -> x8 -> x9 the reference runs by hand (re-launching
    main_sradsgan.py per --scale_factor after editing the paths at sradsgan.py:716-721).  One trainer per scale, results
    under <save_dir>/x<scale>; every stage after the first starts from the previous stage's final generator /
    discriminator files through the shape-aware partial load.  `loaders(scale)` -> (train_loader, test_loader) for
    that scale's tile size.  Returns {scale: (history, chain_report)}."""
    out, prev = OrderedDict(), None
    for scale in scales:
        a = argparse.Namespace(**vars(args))
        a.scale_factor, a.epoch = scale, 0
        a.save_dir = os.path.join(args.save_dir, 'x%d' % scale)
        if prev is not None:
            a.pretrained_generator = os.path.join(prev, 'model', 'generator_param.pkl')
            a.pretrained_discriminator = os.path.join(prev, 'model', 'discriminator_param.pkl')
        train_loader, test_loader = loaders(scale)
        net = trainer_cls(a, train_loader=train_loader, test_loader=test_loader)
        history = net.train()
        out[scale] = (history, getattr(net, 'chain_report', {}))
        prev = a.save_dir
    return out
