"""Data parallelism for the distillation step: one process per GPU, gradients exchanged with RCCL over xGMI.

The reference uses single-process nn.DataParallel (models/networks.py:157-161): scatter the batch, replicate the
module, gather outputs to GPU 0, compute the losses there.  Here every rank owns a full replica and its shard of the
batch (same contiguous chunking as DataParallel.scatter), and only gradients cross the fabric:

  * the buckets are the FusedAdam flat gradient buffers themselves (one per optimizer param group: D ~ 11-44 MB,
    student 2-4 MB, netAs ~0.3 MB) -- no bucket copies, one ring all-reduce per bucket;
  * D bucket: reduced right after backward_D (Adam D needs it before backward_G reads the updated D);
  * G bucket: launched asynchronously on RCCL's stream; its completion is only awaited where the student's updated
    weights are needed (the next student forward), so it overlaps the next iteration's frozen-teacher forward, which
    runs on a side HIP stream and depends on no trainable state;
  * loss semantics of DataParallel are reproduced with gradient AVERAGING (sum all-reduce, 1/world_size
    folded into the Adam kernel) plus a world_size factor on the per-shard KA seed (inception_distiller.py:136-148
    sums per-device KA terms).
"""
import os

import torch
import torch.distributed as dist

from . import derived


def init_distributed(backend=None):
    """Initialise torch.distributed from the torchrun environment (RANK / WORLD_SIZE / LOCAL_RANK / MASTER_*).
    backend 'nccl' is RCCL on ROCm; 'gloo' is used by the CPU tests."""
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world <= 1:
        return 0, 1, 0
    rank = int(os.environ['RANK'])
    local = int(os.environ.get('LOCAL_RANK', rank))
    if backend is None:
        backend = os.environ.get('CAT_DIST_BACKEND') or ('nccl' if torch.cuda.is_available() else 'gloo')
    if 'CAT_FORCE_DEVICE' in os.environ:      # test hook: several ranks on ONE GPU (gloo transport; RCCL needs one device per rank)
        local = int(os.environ['CAT_FORCE_DEVICE'])
    if backend == 'nccl':
        torch.cuda.set_device(local)
    if not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        kw = {}
        if backend == 'nccl':
            kw['device_id'] = torch.device('cuda', local)
        dist.init_process_group(backend=backend, rank=rank, world_size=world, **kw)
    return rank, world, local


def init_single_rank_group(backend=None, local=0):
    """A world_size-1 process group on this GPU (backend 'nccl' = RCCL with one rank).  It lets a one-GPU box run the data-parallel
    schedule end to end -- RCCL loaded, `device_id=` initialisation, all-reduce on the real flat gradient buckets, Work.wait() stream
    ordering -- which is what `bench.py --dp-schedule 1` and tests/test_dp_gpu.py::test_single_rank_rccl_* exercise."""
    if dist.is_initialized():
        return 0, 1, local
    import socket
    backend = backend or os.environ.get('CAT_DIST_BACKEND') or 'nccl'
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    kw = {}
    if backend == 'nccl':
        torch.cuda.set_device(local)
        kw['device_id'] = torch.device('cuda', local)
    dist.init_process_group(backend=backend, init_method=f'tcp://127.0.0.1:{port}', rank=0, world_size=1, **kw)
    return 0, 1, local


def backend_version():
    """'rccl x.y.z' (torch.cuda.nccl.version() IS the RCCL version on ROCm) or the backend's name."""
    if not dist.is_initialized():
        return None
    b = dist.get_backend()
    if b == 'nccl':
        try:
            return 'rccl ' + '.'.join(str(v) for v in torch.cuda.nccl.version())
        except Exception:      # noqa: BLE001  (version query is informational only)
            return 'rccl'
    return b


def _watchdog_retired_all():
    """True once ProcessGroupNCCL's watchdog has retired every collective this process enqueued: its `pg_status` (part of the flight-recorder
    dump, maintained by the watchdog thread itself) reports last_completed_collective == last_enqueued_collective for every group.
    None if this torch build does not expose the status (the caller then falls back to waiting a few polling periods)."""
    import pickle
    try:
        from torch._C import _distributed_c10d as c10d
        status = pickle.loads(c10d._dump_nccl_trace(includeCollectives=False, includeStackTraces=False, onlyActive=True)).get('pg_status')
        if not status:
            return None
        for st in status.values():
            if int(st['last_completed_collective']) < int(st['last_enqueued_collective']):
                return False
        return True
    except Exception:      # noqa: BLE001  (diagnostic API: any surprise means "unknown")
        return None


def settle_collectives(seconds=None):
    """Call before a hipGraph capture in a process that has issued RCCL collectives.  ProcessGroupNCCL's watchdog thread polls the events of
    collectives it has not yet seen complete (every ~100 ms); a poll that lands inside a stream capture is refused by the HIP runtime
    (hipErrorCapturedEvent: "operation not permitted on an event last recorded in a capturing stream") and the watchdog takes the process
    down -- observed with a world_size-1 group when the capture started right after the warm-up steps.  After a device synchronize every
    collective HAS completed on the GPU; what is waited for here is the WATCHDOG having retired them, observed through its own bookkeeping
    (`_watchdog_retired_all`: a handshake, not a timing assumption; bounded by CAT_DP_CAPTURE_SETTLE_MAX_S, default 30 s).  Only where that status is not
    available does the fixed CAT_DP_CAPTURE_SETTLE_S wait of round 3 remain."""
    if not dist.is_initialized() or dist.get_backend() != 'nccl':
        return
    import time
    torch.cuda.synchronize()
    if seconds is not None:
        time.sleep(seconds)
        return
    deadline = time.monotonic() + float(os.environ.get('CAT_DP_CAPTURE_SETTLE_MAX_S', '30'))
    state = _watchdog_retired_all()
    while state is False and time.monotonic() < deadline:
        time.sleep(0.02)
        state = _watchdog_retired_all()
    if state is None:      # no status from this build: a few polling periods
        time.sleep(float(os.environ.get('CAT_DP_CAPTURE_SETTLE_S', '1.0')))
    elif state is False:      # never observed; proceed as round 3 did (the captures run with capture_error_mode='thread_local')
        import warnings
        warnings.warn('settle_collectives: the RCCL watchdog still reports unfinished collectives after a device synchronize')


def shard_batch(batch, rank, world_size):
    """The chunk DataParallel.scatter would hand replica `rank` (contiguous split of dim 0, torch.chunk semantics)."""
    out = {}
    for k, v in batch.items():
        out[k] = v.chunk(world_size, 0)[rank] if torch.is_tensor(v) else v
    return out


class PendingReduce:
    def __init__(self, works, optimizer, world_size):
        self.works, self.optimizer, self.world_size = works, optimizer, world_size

    def wait(self):
        """Make the CURRENT stream wait for the collective (no host sync for NCCL/RCCL works)."""
        for w in self.works:
            w.wait()
        self.works = []


class DataParallelReducer:
    def __init__(self, group=None):
        if not dist.is_initialized():
            raise RuntimeError('torch.distributed is not initialised (launch with torchrun / init_distributed())')
        self.group = group
        self.world_size = dist.get_world_size(group)
        self.rank = dist.get_rank(group)

    def _buckets(self, optimizer_or_tensors):
        if hasattr(optimizer_or_tensors, 'flat_grads'):
            return optimizer_or_tensors.flat_grads()
        return list(optimizer_or_tensors)

    def reduce_async(self, optimizer_or_tensors):
        """Sum-all-reduce every gradient bucket; the 1/world_size average is applied by the optimizer kernel."""
        works = [dist.all_reduce(b, op=dist.ReduceOp.SUM, group=self.group, async_op=True) for b in self._buckets(optimizer_or_tensors)]
        if hasattr(optimizer_or_tensors, 'grad_scale'):
            optimizer_or_tensors.grad_scale = 1.0 / self.world_size
        return PendingReduce(works, optimizer_or_tensors, self.world_size)

    def reduce(self, optimizer_or_tensors):
        self.reduce_async(optimizer_or_tensors).wait()

    def reduce_slice_async(self, optimizer, lo, hi):
        """Sum-all-reduce floats [lo, hi) of a one-bucket optimizer's flat gradient buffer (a gradient-ready slice issued while the rest of
        the backward pass still runs: SURVEY 8e overlap 2).  Ordered behind the CURRENT stream's work at the time of the call."""
        (bucket,) = optimizer.flat_grads()
        work = dist.all_reduce(bucket[lo:hi], op=dist.ReduceOp.SUM, group=self.group, async_op=True)
        optimizer.grad_scale = 1.0 / self.world_size
        return PendingReduce([work], optimizer, self.world_size)

    def broadcast_parameters(self, modules, src=0):
        """Replicas start identical (DataParallel replicates GPU 0's module every forward).  Conv weights may already live in
        their padded channels_last storage (a strided view): those travel through a dense staging copy."""
        for m in modules:
            for t in list(m.parameters()) + list(m.buffers()):
                d = t.data
                if d.is_contiguous():
                    dist.broadcast(d, src=src, group=self.group)
                else:
                    stage = d.contiguous()
                    dist.broadcast(stage, src=src, group=self.group)
                    d.copy_(stage)
        # the broadcast wrote through .data (no version bump): drop every cache derived from the old values
        derived.drop_derived(modules)

    def all_reduce_sum_(self, t):
        """In-place sum over ranks, ordered with the CURRENT stream (SynchronizedBatchNorm's [sum x | sum x^2] exchange,
        models/modules/sync_batchnorm/batchnorm.py:103-123: ReduceAddCoalesced + Broadcast become one all-reduce)."""
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return t

    def all_reduce_sum_many_(self, tensors):
        """Several small statistics buffers as ONE collective (the lockstep units of fused_spade.prepass): flattened into one message and
        scattered back -- element-wise sums, so every buffer ends up exactly as after its own all_reduce_sum_."""
        if len(tensors) == 1:
            return self.all_reduce_sum_(tensors[0])
        # adjacent slices of one arena (what fused_spade._drive_many hands out): the collective runs on the arena span itself -- no
        # torch.cat / copy_ kernels on the step (gaps are the arena's 16-byte alignment padding: summed along, never read)
        first, ok = tensors[0], True
        end = first.data_ptr() + 4 * first.numel()
        for t in tensors[1:]:
            ok = ok and t.is_contiguous() and t.dtype == first.dtype and t.device == first.device and \
                t.untyped_storage().data_ptr() == first.untyped_storage().data_ptr() and end <= t.data_ptr() <= end + 12
            end = t.data_ptr() + 4 * t.numel()
        if ok and first.is_contiguous() and first.dtype == torch.float32:
            span = torch.as_strided(first, ((end - first.data_ptr()) // 4,), (1,), first.storage_offset())
            dist.all_reduce(span, op=dist.ReduceOp.SUM, group=self.group)
            return tensors
        flat = torch.cat([t.reshape(-1) for t in tensors])
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.group)
        o = 0
        for t in tensors:
            n = t.numel()
            t.copy_(flat[o:o + n].view_as(t))
            o += n
        return tensors

    def max_over_ranks(self, seconds):
        t = torch.tensor([seconds], dtype=torch.float64, device='cuda' if dist.get_backend(self.group) == 'nccl' else 'cpu')
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)
        return float(t.item())
