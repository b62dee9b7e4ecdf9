"""Profiler: the reference's profiler.py:38-164 (`profile.py`, the entry point of every scripts/*/evaluate_*.sh) for the tasks
'distill' and 'train', on cat_amd models.

    from cat_amd.profiler import Profiler          # the three-line profile.py
    profiler = Profiler('distill')
    profiler.start()

cat_amd does not own options/, data/ or utils/logger.py.  With none of `opt`, `dataloader`, `logger` given they are imported from
sys.path exactly as the reference's profile.py imports them (run it from a CAT checkout); with the objects given nothing of the reference
is needed.  `create_model` defaults to cat_amd's own create_distiller / create_model.

Same order and same logger calls as the reference: command line appended to opt.txt, seeds, data_channel / height / width from the first
batch, model created and set up, pretrained student loaded by netG kind, two `n_macs` lines, two `FLOPs; Params` lines; start() shrinks
5 + 10 times, prints the mean of the last ten times, reloads the pretrained student and evaluates.

The second pair of lines is torchprofile.profile_macs in the reference (one MAC per output element per Cin/groups * kh * kw of every
aten::_convolution).  torchprofile is not a dependency here: the lines carry conv_macs -- the true convolution MACs of SURVEY 8d, counted
from the module tree and the input shape without a forward pass -- and say so (DESIGN.md relates the two counts)."""
import os
import random
import sys
import time
import warnings

import numpy as np
import torch
from torch import nn

from . import pretrained, prune


def set_seed(seed):
    np.random.seed(seed)
    random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def conv_macs(net, shape):
    """True convolution multiply-accumulates of one forward of `net` (an InceptionGenerator or InceptionSPADEGenerator) at the input
    `shape` = (N, C, H, W): every Conv2d by its output size, every ConvTranspose2d by its INPUT size (each input element meets each
    filter tap once; the reference's n_macs counts it by the output size, 4x too many at stride 2), norms not at all.  Shape propagation
    over the module tree (prune.model_profiling); no forward pass.  Leaves the network's n_macs as model_profiling sets them."""
    n, c, h, w = shape
    for m in net.modules():
        m.__dict__.pop('n_macs', None)      # a module the forward never reaches (the SPADE of a block without branches) counts nothing
    prune.model_profiling(net, h, w, batch=n, channel=c)
    total = sum(getattr(m, 'n_macs', 0) for m in net.modules() if isinstance(m, nn.Conv2d))
    transposed = [m for m in net.modules() if isinstance(m, nn.ConvTranspose2d)]
    if transposed:
        up = getattr(net, 'up_sampling', None)
        if up is None or any(all(m is not s for s in up) for m in transposed):
            raise NotImplementedError('conv_macs: a ConvTranspose2d outside InceptionGenerator.up_sampling')
        cur = prune._profile(net.features, prune._profile(net.down_sampling, shape))
        for sub in up:
            if isinstance(sub, nn.ConvTranspose2d):
                kh, kw = sub.kernel_size
                total += (cur[1] * sub.out_channels * kh * kw * cur[2] * cur[3] // sub.groups) * cur[0]
            cur = prune._profile(sub, cur)
    return int(total)


def timed_shrink(model, opt):
    """prune.shrink, returning the seconds it took (the reference's shrink returns its own pruning time)."""
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    t0 = time.time()
    prune.shrink(model, opt)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return time.time() - t0


class Profiler:
    def __init__(self, task, opt=None, dataloader=None, logger=None, create_model=None, shrink=None):
        if task not in ('train', 'distill'):
            raise NotImplementedError('Unknown task [%s]!!!' % task)
        if opt is None:
            if task == 'train':
                from options.train_options import TrainOptions as Options
            else:
                from options.distill_options import DistillOptions as Options
            opt = Options().parse()
        if create_model is None:
            if task == 'train':
                from .models import create_model
            else:
                from .distillers import create_distiller as create_model
        opt.tensorboard_dir = opt.log_dir if getattr(opt, 'tensorboard_dir', None) is None else opt.tensorboard_dir
        print(' '.join(sys.argv))
        if opt.phase != 'train':
            warnings.warn('You are not using training set for %s!!!' % task)
        with open(os.path.join(opt.log_dir, 'opt.txt'), 'a') as f:
            f.write(' '.join(sys.argv) + '\n')
        set_seed(opt.seed)

        if dataloader is None:
            from data import create_dataloader
            dataloader = create_dataloader(opt)
        dataset_size = len(dataloader.dataset)
        print('The number of training images = %d' % dataset_size)
        opt.iters_per_epoch = len(dataloader)
        if opt.dataset_mode in ['aligned', 'unaligned']:
            opt.data_channel, opt.data_height, opt.data_width = next(iter(dataloader))['A' if opt.direction == 'AtoB' else 'B'].shape[1:]
        elif opt.dataset_mode in ['cityscapes']:
            input_ = next(iter(dataloader))
            opt.data_height, opt.data_width = input_['label'].shape[2:]
            opt.data_channel = opt.input_nc
            if opt.contain_dontcare_label:
                opt.data_channel += 1
            if not opt.no_instance:
                opt.data_channel += input_['instance'].shape[1]
        else:
            raise NotImplementedError
        print(f'data shape is: channel={opt.data_channel}, height={opt.data_height}, width={opt.data_width}.')

        model = create_model(opt)
        model.setup(opt)
        if logger is None:
            from utils.logger import Logger
            logger = Logger(opt)

        self.opt, self.dataloader, self.model, self.logger, self.task = opt, dataloader, model, logger, task
        self._shrink = timed_shrink if shrink is None else shrink
        self._load_pretrained_student()

        m = getattr(model, 'modules_on_one_gpu', model)
        if self.task == 'distill':
            logger.print_info(f'netG teacher FLOPs: {m.netG_teacher.n_macs}.')
            logger.print_info(f'netG student FLOPs: {m.netG_student.n_macs}.')
            shape = (1, opt.data_channel, opt.data_height, opt.data_width)
            t_macs, s_macs = m.netG_teacher.n_macs, m.netG_student.n_macs
            macs_t, macs_s = conv_macs(m.netG_teacher, shape), conv_macs(m.netG_student, shape)
            m.netG_teacher.n_macs, m.netG_student.n_macs = t_macs, s_macs
            params_t = sum(p.numel() for p in m.netG_teacher.parameters())
            params_s = sum(p.numel() for p in m.netG_student.parameters())
            logger.print_info(f'netG teacher FLOPs: {macs_t} (true conv MACs); Params: {params_t}.')
            logger.print_info(f'netG student FLOPs: {macs_s} (true conv MACs); Params: {params_s}.')

    def _load_pretrained_student(self):
        if getattr(self.opt, 'pretrained_student_G_path', '') and self.task == 'distill':
            pretrained.load(self.model, self.opt)      # by netG kind, with the two asserts of profiler.py:85-86

    def evaluate(self, epoch, iter, message, save_image=False):
        start_time = time.time()
        metrics = self.model.evaluate_model(iter, save_image=save_image)
        self.logger.print_current_metrics(epoch, iter, metrics, time.time() - start_time)
        self.logger.print_info(message)

    def start(self):
        if self.task == 'distill':
            N_test = 10
            pruning_time_list = []
            for i in range(5):
                self._shrink(self.model, self.opt)
            for i in range(N_test):
                pruning_time_list.append(self._shrink(self.model, self.opt))
            print(f'Average pruning time for {N_test} experiments: {np.mean(pruning_time_list):.2f}s.')
        self._load_pretrained_student()
        self.evaluate(0, 0, 'Model evaluated.', save_image=True)

    def measure_latency(self, iters=20, warmup=5, graph=True):
        """Not part of the reference's sequence (start() does not call it): teacher and student inference time per image at
        eval_batch_size, by HIP events, each generator on cat_amd.infer.StudentRunner."""
        from .infer import StudentRunner
        opt = self.opt
        m = getattr(self.model, 'modules_on_one_gpu', self.model)
        n = int(getattr(opt, 'eval_batch_size', 1))
        x = torch.ones([n, opt.data_channel, opt.data_height, opt.data_width], device=self.model.device)
        out = {}
        for name in ('teacher', 'student'):
            net = getattr(m, 'netG_' + name, None)
            if net is None:
                continue
            modes = [(mod, mod.training) for mod in net.modules()]      # module by module: parts may have been left in eval() on purpose
            runner = StudentRunner(net, x, graph=graph)
            try:
                out[name] = runner.latency(iters, warmup) / n
            finally:
                runner.release()
                for mod, was in modes:
                    mod.training = was
            self.logger.print_info(f'netG {name} latency: {out[name]:.3f} ms/img at batch {n} ({"hipGraph" if graph else "eager"}, HIP events).')
        return out
