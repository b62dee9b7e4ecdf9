"""BaseModel: the host-side glue of models/base_model.py:12-232 that `train.py` / `Trainer` touch (device, save_dir, setup,
schedulers, loss dictionary, requires_grad toggling, checkpoints with the reference's file names and state_dict keys).  Dataset
loaders stay with the reference; FID / mIoU evaluation is the distillers' path (cat_amd/distillers/evaluation.py,
cat_amd/metric: InceptionV3 and DRN-D-105 on the HIP kernels)."""
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

    def evaluate_model(self, step):
        raise NotImplementedError('teacher-training models: evaluate with the distillers\' path -- cat_amd.distillers.evaluation.evaluate + '
                                  'attach_fid / attach_miou (InceptionV3 pool3 features and the DRN-D-105 cityscapes mIoU on the HIP kernels, '
                                  'cat_amd.metric); mIoU needs the reference\'s DRN checkpoint and the cityscapes data (SURVEY §2 rows 18-19)')
