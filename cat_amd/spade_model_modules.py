"""SPADEModelModules: the nn.Module of the GauGAN TEACHER step (`train.py --model spade`): generator, multiscale discriminator and the
GAN / feature-matching / VGG criteria, evaluated inside `forward(mode=...)` with the reference's attribute names, modes and loss keys
(models/modules/spade_modules/spade_model_modules.py:13-175).

The reference wraps this module in DataParallelWithCallback; here one process drives one GPU (multi-rank teacher training is not built:
DESIGN §7).

The discriminator's loss head -- num_D * n_layers_D feature-matching L1 terms + num_D GAN terms in the G step, 2 * num_D hinge terms in the D
step -- is ONE ops.MultiLossFn call each (two forward launches, one backward launch) instead of a LossFn reduction pair and a backward
launch per term.  CAT_LOSS_MULTI=0 selects the per-term path (A/B switch, read once at import).  Either way the losses are LossValue objects
(lossvalue.py): the weights travel as backward seeds, nothing is added with torch arithmetic.  The VGG terms stay per-term: they are
interleaved with the VGG slices."""
import copy
import os

import torch

from . import _lib as L
from . import loss as closs
from . import networks, ops
from .optim import FusedAdam
from .lossvalue import LossValue
from .prune import model_profiling
from .spade_modules import SPADEModules

_LOSS_MULTI = os.environ.get('CAT_LOSS_MULTI', '1') != '0'


def loss_multi_enabled():
    return _LOSS_MULTI


class SPADEModelModules(SPADEModules):
    def __init__(self, opt):
        opt = copy.deepcopy(opt)
        if len(opt.gpu_ids) > 0:
            opt.gpu_ids = opt.gpu_ids[:1]
        self.gpu_ids = opt.gpu_ids
        super(SPADEModelModules, self).__init__()
        self.opt = opt
        self.model_names = ['G']
        self.visual_names = ['labels', 'fake_B', 'real_B']
        self.netG = networks.define_G(opt.input_nc, opt.output_nc, opt.ngf, opt.netG, opt.norm, getattr(opt, 'dropout_rate', 0), opt.init_type,
                                      opt.init_gain, self.gpu_ids, opt=opt)
        if opt.isTrain:
            self.model_names.append('D')
            self.netD = networks.define_D(opt.input_nc + opt.output_nc, opt.ndf, opt.netD, opt.n_layers_D, opt.norm, opt.init_type,
                                          opt.init_gain, self.gpu_ids, opt=opt)
            self.criterionGAN = closs.GANLoss(opt.gan_mode)
            self.criterionFeat = closs.L1Loss()
            self.criterionVGG = closs.VGGLoss(width_div=getattr(opt, 'vgg_width_div', 1))
            if len(self.gpu_ids) > 0:
                self.criterionVGG.to(torch.device('cuda', self.gpu_ids[0]))
            self.optimizers = []
            self.loss_names = ['G_gan', 'G_feat', 'G_vgg', 'D_real', 'D_fake']
        else:
            self.netG.eval()

    def create_optimizers(self):
        """spade_model_modules.py:52-65."""
        beta1, beta2, G_lr, D_lr = self._ttur()
        optimizer_G = FusedAdam(list(self.netG.parameters()), lr=G_lr, betas=(beta1, beta2))
        optimizer_D = FusedAdam(list(self.netD.parameters()), lr=D_lr, betas=(beta1, beta2))
        return optimizer_G, optimizer_D

    def generate_fake(self, input_semantics):
        return self.netG(input_semantics)

    def profile(self, input_semantics):
        """spade_model_modules.py:80-91: (macs, params) of the generator at the input's geometry."""
        batch_, channel_, height_, width_ = input_semantics.shape
        return model_profiling(self.netG, height_, width_, batch_, channel_, verbose=False)

    # -- losses -------------------------------------------------------------------------------------------------------------
    def _head(self, terms):
        """terms: [(kind, target, a, b)] -> their 0-d means, in order: one MultiLossFn call, or one LossFn per term (CAT_LOSS_MULTI=0)."""
        if not _LOSS_MULTI:
            return [ops.LossFn.apply(a, b, kind, target) for kind, target, a, b in terms]
        flat = []
        for _, _, a, b in terms:
            flat += [a, b]
        return list(ops.MultiLossFn.apply(tuple((kind, target) for kind, target, _, _ in terms), *flat))

    def compute_G_loss(self, input_semantics, real_B):
        """spade_model_modules.py:93-115.  G_gan is criterionGAN's list form (mean over num_D) * lambda_gan; G_feat is
        sum_ij L1(fake_ij, real_ij.detach()) * lambda_feat / num_D (no gradient reaches the second operand of a loss term)."""
        opt = self.opt
        fake_B = self.netG(input_semantics)
        f_d, f_v = ops.fanout(fake_B, 2)
        pred_fake, pred_real = self.discriminate(input_semantics, f_d, real_B)
        num_D = len(pred_fake)
        kind, target = self.criterionGAN.kind(True, False)
        terms = [(kind, target, p[-1], None) for p in pred_fake]
        for i in range(num_D):
            for j in range(len(pred_fake[i]) - 1):
                terms.append((L.LOSS_L1, 0.0, pred_fake[i][j], pred_real[i][j]))
        vals = self._head(terms)
        loss_G_gan = LossValue([(opt.lambda_gan / num_D, v) for v in vals[:num_D]])
        loss_G_feat = LossValue([(opt.lambda_feat / num_D, v) for v in vals[num_D:]])
        loss_G_vgg = LossValue([(w * opt.lambda_vgg, t) for w, t in self.criterionVGG.terms(f_v, real_B)])
        loss_G = loss_G_gan + loss_G_feat + loss_G_vgg
        self._last = fake_B
        return {'loss_G': loss_G, 'G_gan': loss_G_gan, 'G_feat': loss_G_feat, 'G_vgg': loss_G_vgg}

    def compute_D_loss(self, input_semantics, real_B):
        """spade_model_modules.py:117-134: fake_B is REGENERATED under no_grad, after the G update, with the generator still in train mode
        (its SynchronizedBatchNorm running statistics advance a second time in every step, as in the reference)."""
        with torch.no_grad():
            fake_B = self.netG(input_semantics)
        pred_fake, pred_real = self.discriminate(input_semantics, fake_B, real_B)
        num_D = len(pred_fake)
        kf, tf = self.criterionGAN.kind(False, True)
        kr, tr = self.criterionGAN.kind(True, True)
        vals = self._head([(kf, tf, p[-1], None) for p in pred_fake] + [(kr, tr, p[-1], None) for p in pred_real])
        loss_D_fake = LossValue([(1.0 / num_D, v) for v in vals[:num_D]])
        loss_D_real = LossValue([(1.0 / num_D, v) for v in vals[num_D:]])
        return {'loss_D': loss_D_fake + loss_D_real, 'D_fake': loss_D_fake, 'D_real': loss_D_real}
