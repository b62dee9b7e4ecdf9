"""SPADEModel: the GauGAN teacher-training step of `train.py --model spade` (reference models/spade_model.py:22-288) on the gfx950 kernels --
one-hot + edge semantics, InceptionSPADEGenerator in train mode, the multiscale spectral-instance discriminator, hinge / feature-matching /
VGG losses, two FusedAdam updates (G first, then D) -- with the surface the reference's Trainer touches.  The networks and losses live in
cat_amd/spade_model_modules.py; the device, data and bookkeeping halves follow distillers/base_spade_distiller.py; evaluation goes through
distillers/evaluation.py.  One process drives one GPU: multi-rank training of the teacher is not built."""
import argparse

import torch

from .. import ops
from ..spade_model_modules import SPADEModelModules
from ..spade_modules import SPADEStep
from .base_model import BaseModel


class SPADEModel(SPADEStep, BaseModel):
    _FLAGS = [  # spade_model.py:27-39
        ('--norm_G', dict(type=str, default='spadesyncbatch3x3', help='instance normalization or batch normalization')),
        ('--num_upsampling_layers', dict(choices=('normal', 'more', 'most'), default='more')),
    ]
    _TRAIN_FLAGS = [  # spade_model.py:40-81
        ('--restore_G_path', dict(type=str, default=None, help='the path to restore the generator')),
        ('--restore_D_path', dict(type=str, default=None, help='the path to restore the discriminator')),
        ('--real_stat_path', dict(type=str, required=True, help='the path to load the groud-truth images information to compute FID.')),
        ('--lambda_gan', dict(type=float, default=1, help='weight for gan loss')),
        ('--lambda_feat', dict(type=float, default=10, help='weight for gan feature loss')),
        ('--lambda_vgg', dict(type=float, default=10, help='weight for vgg loss')),
        ('--beta2', dict(type=float, default=0.999, help='momentum term of adam')),
        ('--no_TTUR', dict(action='store_true', help='Use TTUR training scheme')),
        ('--no_fid', dict(action='store_true', help='No FID evaluation during training')),
        ('--no_mIoU', dict(action='store_true', help='No mIoU evaluation during training')),
        ('--virtual_replicas', dict(type=int, default=1)),      # the arithmetic of that many reference GPUs on this one (host.set_virtual_replicas)
    ]

    @staticmethod
    def modify_commandline_options(parser, is_train):
        assert isinstance(parser, argparse.ArgumentParser)
        parser.set_defaults(netG='inception_spade')
        for flag, kw in SPADEModel._FLAGS:
            parser.add_argument(flag, **kw)
        if is_train:
            for flag, kw in SPADEModel._TRAIN_FLAGS:
                parser.add_argument(flag, **kw)
            parser.set_defaults(netD='multi_scale', ndf=64, dataset_mode='cityscapes', batch_size=16, print_freq=50,
                                save_latest_freq=10000000000, save_epoch_freq=10, nepochs=100, nepochs_decay=100, init_type='xavier',
                                active_fn='nn.LeakyReLU')
            # networks.modify_commandline_options (networks.py:296-305): the discriminator class adds its own flags; the generator adds none
            from ..discriminators import MultiscaleDiscriminator
            if parser.get_default('netD') == 'multi_scale':
                parser = MultiscaleDiscriminator.modify_commandline_options(parser, is_train)
        return parser

    def __init__(self, opt):
        super(SPADEModel, self).__init__(opt)
        ops.default_branch_streams(True)       # the GauGAN step is ~1 500 small launches: side streams gain 6 - 9 % (base_spade_distiller.py)
        self.model_names = ['G']
        self.visual_names = ['labels', 'fake_B', 'real_B']
        mopt = argparse.Namespace(**vars(opt))
        mopt.gpu_ids = list(self._dev_ids)
        self.modules = SPADEModelModules(mopt).to(self.device)
        self.modules_on_one_gpu = self.modules
        if opt.isTrain:
            self.model_names.append('D')
            self.loss_names = ['G_gan', 'G_feat', 'G_vgg', 'D_real', 'D_fake']
            self.optimizer_G, self.optimizer_D = self.modules_on_one_gpu.create_optimizers()
            self.optimizers = [self.optimizer_G, self.optimizer_D]
            self.best_fid = 1e9
            self.best_mIoU = -1e9
            self.fids, self.mIoUs = [], []
            self.is_best = False
            self.eval_dataloader = None
            self._eval_ready = False
        else:
            self.modules.eval()

    # the reference keeps the networks on `modules`; BaseModel's eval / train / print_networks look for net<name> on the model
    @property
    def netG(self):
        return self.modules_on_one_gpu.netG

    @property
    def netD(self):
        return self.modules_on_one_gpu.netD

    # -- the step (spade_model.py:163-215) ------------------------------------------------------------------------------------
    def forward(self, on_one_gpu=False):
        self.fake_B = self.modules_on_one_gpu(self.input_semantics)

    def test(self):
        with torch.no_grad():
            self.forward(on_one_gpu=True)

    def profile(self, verbose=True):
        macs, params = self.modules_on_one_gpu.profile(self.input_semantics[:1])
        if verbose:
            print('MACs: %.3fG\tParams: %.3fM' % (macs / 1e9, params / 1e6), flush=True)
        return macs, params

    def backward_G(self):
        losses = self._losses('G_loss')
        self.fake_B = self.modules_on_one_gpu._last
        losses['loss_G'].backward()

    def optimize_parameters(self, steps):
        self.set_requires_grad(self.modules_on_one_gpu.netD, False)
        self.optimizer_G.zero_grad()
        self.backward_G()
        self.optimizer_G.step()
        self.set_requires_grad(self.modules_on_one_gpu.netD, True)
        self.optimizer_D.zero_grad()
        self.backward_D()
        self.optimizer_D.step()

    # -- evaluation (spade_model.py:113-128, 217-288) ---------------------------------------------------------------------------
    def _want_metrics(self):
        want_fid = not getattr(self.opt, 'no_fid', False)
        want_miou = 'cityscapes' in str(getattr(self.opt, 'dataroot', '')) and not getattr(self.opt, 'no_mIoU', False)
        return want_fid, want_miou

    def _prepare_evaluation(self):
        """What the reference's __init__ builds for evaluation, created on first use and only where evaluation needs it: the inception model
        and the real-image statistics (unless no_fid), the DRN model (cityscapes, unless no_mIoU).  The evaluation dataloader stays the
        integrator's (`model.eval_dataloader`; cat_amd owns no datasets)."""
        from ..distillers import evaluation as E
        want_fid, want_miou = self._want_metrics()
        if want_fid and getattr(self, 'fid_fn', None) is None and getattr(self, 'inception_model', None) is None:
            ckpt = getattr(self.opt, 'inception_path', None)
            if ckpt is None:
                raise RuntimeError('evaluate_model: FID needs the torchvision-keyed FID inception checkpoint (opt.inception_path) or an '
                                   'attached model.fid_fn; pass --no_fid to train without it')
            E.attach_fid(self, ckpt, self.opt.real_stat_path)
        if want_miou and getattr(self, 'miou_fn', None) is None and getattr(self, 'drn_model', None) is None:
            E.attach_miou(self, self.opt.drn_path, getattr(self.opt, 'table_path', None), getattr(self.opt, 'cityscapes_path', None))
        self._eval_ready = True

    def evaluate_model(self, step, save_image=False):
        from ..distillers import evaluation as E
        if not self._eval_ready:
            self._prepare_evaluation()

        def images(j):
            return {'input': E.tensor2label(self.input_semantics[j], self.opt.input_nc + 2), 'real': E.image_of(self, self.real_B[j]),
                    'fake': E.image_of(self, self.fake_B[j])}
        want_fid, want_miou = self._want_metrics()
        return E.evaluate(_EvalView(self), step, self.modules_on_one_gpu.netG, self.set_input, images, want_fid, want_miou, save_all=save_image)

    # -- bookkeeping (spade_model.py:290-342) -----------------------------------------------------------------------------------
    def load_networks(self, verbose=True, teacher_only=False, restore_pretrain=True):
        self.modules_on_one_gpu.load_networks(verbose)
        if self.isTrain:
            self.restore_optimizers(self.modules_on_one_gpu._ttur()[2:])


class _EvalView:
    """evaluation.evaluate reads the generated batch as `Sfake_B` (the distillers' name); everything else -- the bookkeeping it updates
    included -- is the model's own."""

    def __init__(self, model):
        object.__setattr__(self, '_m', model)

    def __getattr__(self, name):
        return getattr(self._m, 'fake_B' if name == 'Sfake_B' else name)

    def __setattr__(self, name, value):
        setattr(self._m, name, value)
