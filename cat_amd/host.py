"""StepHost: what `train.py` / `Trainer` touch on every model and distiller besides the step itself (reference models/base_model.py:12-232,
repeated in the distillers' bases): the device of this process, save_dir, schedulers, the loss dictionary, requires_grad toggling and the
checkpoint wire format.  The checkpoint helpers and the bookkeeping methods need nothing that only the constructor creates."""
import os
from collections import OrderedDict

import torch

from . import lossvalue, networks


def cpu_state_dict(net):
    """NCHW / OIHW-contiguous host values under the module's own keys: the checkpoint wire format."""
    return OrderedDict((k, v.detach().cpu().contiguous()) for k, v in net.state_dict().items())


def load_state(net, path, verbose=True):
    if verbose:
        print('Load network at %s' % path)
    net.load_state_dict(torch.load(path, map_location='cpu'))


def named_nets(owner):
    """[(name, net<name>)] over owner.model_names: the reference's naming of models/base_model.py."""
    return [(name, getattr(owner, 'net' + name)) for name in owner.model_names]


def distilled_nets(owner):
    """What a distiller saves, by file tag: the student as G, the discriminator, the 1x1 adaptors (base_inception_distiller.py:367-396)."""
    return [('G', owner.netG_student), ('D', owner.netD)] + [('A-%d' % i, net) for i, net in enumerate(owner.netAs)]


def restore_named(owner, verbose=True):
    """net<name> <- opt.restore_<name>_path for the names that have one (models/base_model.py:201-215)."""
    for name, net in named_nets(owner):
        path = getattr(owner.opt, 'restore_%s_path' % name, None)
        if path is not None:
            load_state(net, path, verbose)


def save_nets(nets, epoch, save_dir):
    for tag, net in nets:
        torch.save(cpu_state_dict(net), os.path.join(save_dir, '%s_net_%s.pth' % (epoch, tag)))


class StepHost:
    _NOUN = 'models'       # '<package> <noun> need an MI355X ...'

    def __init__(self, opt):
        self.opt = opt
        self.gpu_ids = list(getattr(opt, 'gpu_ids', [0]))
        self.isTrain = opt.isTrain
        if not torch.cuda.is_available():
            raise RuntimeError('cat_amd %s need an MI355X (HIP kernels only; there is no CPU path)' % self._NOUN)
        # one process drives one GPU (torch.distributed / RCCL handles data parallelism): gpu_ids[0] or LOCAL_RANK
        dev_index = int(os.environ.get('LOCAL_RANK', self.gpu_ids[0] if self.gpu_ids else 0))
        self.device = torch.device('cuda', dev_index)
        torch.cuda.set_device(self.device)
        self._dev_ids = [dev_index]
        self.save_dir = os.path.join(getattr(opt, 'log_dir', '.'), 'checkpoints')
        self.image_paths = []
        self.dp = None     # cat_amd.parallel.DataParallelReducer when world_size > 1
        self.virtual_replicas = 1      # set_virtual_replicas

    def seed(self, value):
        """Constant 0-d device tensors used as backward seeds (d total / d term)."""
        return lossvalue.seed(self.device, value)

    backward_terms = staticmethod(lossvalue.backward_terms)

    def set_virtual_replicas(self, replicas):
        """Compute, on this one GPU, what `replicas` reference GPUs under nn.DataParallel compute on the same batch (a recipe written for k
        GPUs: --virtual_replicas k): every training BatchNorm of every network this host owns takes its statistics per
        torch.chunk(batch, replicas) shard (networks.set_virtual_replicas), and the steps read self.virtual_replicas for their per-replica
        distillation terms.  Under a DataParallelReducer with W ranks the result is that of W * replicas reference GPUs.  1 = as built.
        The SPADE family's SynchronizedBatchNorm layers are truly synchronised: their statistics stay whole-batch, but with more than one
        replica the reference takes its multi-replica arm (clamp(var, eps), sync_batchnorm/batchnorm.py:103-140).  A host that owns such
        layers and has no multi-rank reducer installs ops.ReplicaSync -- the same kernels as under a reducer, the exchange an identity --
        while replicas > 1, and removes it again at 1 (ops.set_bn_sync is process-wide, as under enable_data_parallel)."""
        from . import nn as cnn
        from . import ops
        replicas = int(replicas)
        if replicas < 1:
            raise ValueError('virtual_replicas must be >= 1, got %d' % replicas)
        nets = [net for v in list(vars(self).values()) for net in (v if isinstance(v, (list, tuple)) else [v]) if isinstance(net, torch.nn.Module)]
        self.virtual_replicas = replicas
        for net in nets:
            networks.set_virtual_replicas(net, replicas)
            if hasattr(net, 'calc_distill_loss'):      # the SPADE family keeps its loss terms on the module that owns the networks
                net.virtual_replicas = replicas
        if any(cnn._exchanges(m) for net in nets for m in net.modules()):
            cur = ops.bn_sync()
            if replicas > 1 and cur is None:
                ops.set_bn_sync(ops.ReplicaSync())
            elif replicas == 1 and isinstance(cur, ops.ReplicaSync):
                ops.set_bn_sync(None)

    def setup(self, opt, verbose=True):
        self.set_virtual_replicas(getattr(opt, 'virtual_replicas', 1))
        if self.isTrain:
            self.schedulers = [networks.get_scheduler(optimizer, opt) for optimizer in self.optimizers]
        self.load_networks(verbose)
        if verbose:
            self.print_networks()

    def _networks(self):
        """(printed name, net) of print_networks."""
        return named_nets(self)

    def print_networks(self):
        for name, net in self._networks():
            print('[Network %s] Total number of parameters : %.3f M' % (name, sum(p.numel() for p in net.parameters()) / 1e6))

    def finish_pending(self):
        """Complete work a schedule deferred past optimize_parameters (the inception distiller's data-parallel step keeps the student's
        gradient all-reduce and Adam update in flight until the weights are needed): called by everything that reads weights or optimizer
        state.  Nothing is ever pending in the other steps."""

    def stage_replay(self, batch):
        """Called by cat_amd.graph.GraphedStep before it replays the captured step on `batch`: host decisions the capture could not record
        (the CycleGAN image pools' random draws) are taken here and handed to the graph through device memory.  Nothing to stage in the
        other steps."""

    def get_current_visuals(self):
        self.finish_pending()
        return OrderedDict((n, getattr(self, n)) for n in self.visual_names if hasattr(self, n))

    def update_learning_rate(self, logger=None):
        self.finish_pending()       # a pending Adam step must use the learning rate of the step that produced its gradient
        for scheduler in self.schedulers:
            scheduler.step()
        lr = self.optimizers[0].param_groups[0]['lr']
        (logger.print_info if logger is not None else print)('learning rate = %.7f\n' % lr)

    def get_current_losses(self):
        errors_set = OrderedDict()
        for name in self.loss_names:
            if not hasattr(self, 'loss_' + name):
                continue
            if any(ch.isdigit() for ch in name):
                key = 'Specific_loss/' + name
            elif name.startswith('D_'):
                key = 'D_loss/' + name
            elif name.startswith('G_'):
                key = 'G_loss/' + name
            else:
                assert False
            errors_set[key] = float(getattr(self, 'loss_' + name))
        return errors_set

    def set_requires_grad(self, nets, requires_grad=False):
        if not isinstance(nets, list):
            nets = [nets]
        for net in nets:
            if net is not None:
                for param in net.parameters():
                    param.requires_grad = requires_grad

    # -- checkpoints ----------------------------------------------------------------------------------------------------------
    def save_networks(self, epoch):
        self.finish_pending()
        os.makedirs(self.save_dir, exist_ok=True)
        self._save(epoch)

    def _save(self, epoch):
        """What save_networks writes into save_dir: the named networks here (models/base_model.py:217-232 saves no optimizer state);
        the distillers and the GauGAN steps write theirs and add save_optimizers."""
        save_nets(named_nets(self), epoch, self.save_dir)

    def save_optimizers(self, epoch):
        for i, optimizer in enumerate(self.optimizers):
            torch.save(optimizer.state_dict(), os.path.join(self.save_dir, '%s_optim-%d.pth' % (epoch, i)))

    def restore_optimizers(self, lrs):
        """opt.restore_O_path (when set): optimizer i <- '<path>-<i>.pth', then every group of optimizer i runs at lrs[i] -- the rule is
        the caller's (the distillers restart at opt.lr, the GauGAN teacher at its TTUR rates)."""
        path = getattr(self.opt, 'restore_O_path', None)
        if not path:
            return
        for i, (optimizer, lr) in enumerate(zip(self.optimizers, lrs)):
            optimizer.load_state_dict(torch.load('%s-%d.pth' % (path, i), map_location='cpu'))
            for param_group in optimizer.param_groups:
                param_group['lr'] = lr
