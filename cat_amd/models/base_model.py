"""BaseModel: the host-side glue of models/base_model.py:12-232 that `train.py` / `Trainer` touch (device, save_dir, setup,
schedulers, loss dictionary, requires_grad toggling, checkpoints with the reference's file names and state_dict keys).  Dataset
loaders stay with the reference: the integrator attaches the evaluation dataloaders.  `evaluate_model` of the three
models goes through cat_amd/distillers/evaluation.evaluate; the metric networks (cat_amd/metric: InceptionV3 and DRN-D-105 on the HIP kernels)
are created on first use from the checkpoints the options name (`_prepare_evaluation`)."""
from abc import ABC, abstractmethod

import torch

from .. import host, ops


class BaseModel(host.StepHost, ABC):
    def __init__(self, opt):
        super().__init__(opt)
        self.model_names, self.visual_names, self.loss_names, self.optimizers = [], [], [], []
        self.metric = 0

    @staticmethod
    def modify_commandline_options(parser, is_train):
        return parser

    @abstractmethod
    def set_input(self, input):
        pass

    @abstractmethod
    def forward(self):
        pass

    @abstractmethod
    def optimize_parameters(self, steps):
        pass

    def _to_device_act(self, x):
        return ops.to_nhwc(x.to(self.device, dtype=torch.float32, non_blocking=True))

    def eval(self):
        for name in self.model_names:
            getattr(self, 'net' + name).eval()

    def train(self):
        for name in self.model_names:
            getattr(self, 'net' + name).train()

    def test(self):
        with torch.no_grad():
            self.forward()

    def get_image_paths(self):
        return self.image_paths

    def load_networks(self, verbose=True, teacher_only=False, restore_pretrain=True):
        host.restore_named(self, verbose)

    def enable_data_parallel(self, reducer):
        """One process per GPU (cat_amd.parallel): replicas are synchronised once, then the flat gradient buckets are all-reduced
        after each backward pass.  Every loss of these models is a mean over the batch = plain gradient averaging."""
        self.dp = reducer
        reducer.broadcast_parameters([getattr(self, 'net' + n) for n in self.model_names])

    def _prepare_evaluation(self, stats, want_miou):
        """What the reference's __init__ builds for evaluation, created on first use: the inception model (opt.inception_path) and the real
        statistics -- stats = {attribute: name of the option with its file} -- unless a fid_fn is attached; the DRN model (opt.drn_path,
        opt.table_path, opt.cityscapes_path) if want_miou, unless a miou_fn is attached."""
        import numpy as np

        from ..distillers import evaluation as E

        def attached(name):
            fn = getattr(self, name, None)
            return fn is not None and not getattr(fn, 'cat_builtin', False)
        if not attached('fid_fn'):
            if getattr(self, 'inception_model', None) is None:
                ckpt = getattr(self.opt, 'inception_path', None)
                if ckpt is None:
                    raise RuntimeError('evaluate_model: FID needs the torchvision-keyed FID inception checkpoint (opt.inception_path), an '
                                       'attached model.inception_model or an attached model.fid_fn')
                from ..metric.features import load_inception
                self.inception_model = load_inception(2048, ckpt, self.device, 'FID')
            for attr, option in stats.items():
                if getattr(self, attr, None) is None:
                    path = getattr(self.opt, option, None)
                    if path is None:
                        raise RuntimeError('evaluate_model: FID needs the real statistics {mu, sigma} (opt.%s), an attached model.%s or an '
                                           'attached model.fid_fn' % (option, attr))
                    setattr(self, attr, np.load(path))
        if want_miou and not attached('miou_fn') and getattr(self, 'drn_model', None) is None:
            ckpt = getattr(self.opt, 'drn_path', None)
            if ckpt is None:
                raise RuntimeError('evaluate_model: the cityscapes mIoU needs the DRN-D-105 checkpoint (opt.drn_path; evaluation.attach_miou) '
                                   'or an attached model.miou_fn = lambda fakes, names: ...')
            E.attach_miou(self, ckpt, getattr(self.opt, 'table_path', None), getattr(self.opt, 'cityscapes_path', None))
