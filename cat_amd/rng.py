"""Device-resident random state of the dropout kernels (csrc/dropout.hip).

One int64 tensor {seed, counter} per device.  draw() enqueues cat_rng_draw, which writes a 4-int ticket {lo32(counter), lo32(seed),
hi32(seed), 0} and increments the counter ON THE DEVICE: every dropout launch of one block forward (and of its backward pass) reads
that ticket, and a step replayed as a captured graph advances the counter exactly like the same step run eagerly, so each replay
draws fresh masks.  The seed defaults to torch.initial_seed() when a device's state is created (its first draw); manual_seed() sets it
and resets the counter.  Neither depends on the rank: data-parallel replicas draw the same masks, as the reference's nn.DataParallel
replicas do after torch.cuda.manual_seed_all."""
import torch

from . import _lib as L
from . import ops

_STATE = {}         # device index -> int64 tensor [seed, counter]
_SEED = None        # manual_seed() value for states created later (None: torch.initial_seed())


def _signed(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= (1 << 63) else v


def _index(device):
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    return device.index if device.index is not None else torch.cuda.current_device()


def state_tensor(device=None):
    """The {seed, counter} tensor of `device`, created on first use."""
    i = _index(device)
    st = _STATE.get(i)
    if st is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('cat_amd.rng: the first dropout draw on a device cannot happen inside a graph capture (run a step eagerly first)')
        seed = torch.initial_seed() if _SEED is None else _SEED
        st = torch.tensor([_signed(seed), 0], dtype=torch.int64, device=torch.device('cuda', i))
        _STATE[i] = st
    return st


def manual_seed(seed, device=None):
    """Seed the dropout masks of `device` (default: every device, including those whose state is created later); the counter restarts."""
    global _SEED
    if device is None:
        _SEED = int(seed)
        for st in _STATE.values():
            st.copy_(torch.tensor([_signed(int(seed)), 0], dtype=torch.int64))
    else:
        state_tensor(device).copy_(torch.tensor([_signed(int(seed)), 0], dtype=torch.int64))


def get_state(device=None):
    """-> (seed, counter) as unsigned Python ints (synchronises)."""
    s, c = (int(v) for v in state_tensor(device).cpu().tolist())
    return s & ((1 << 64) - 1), c & ((1 << 64) - 1)


def set_state(seed, counter, device=None):
    state_tensor(device).copy_(torch.tensor([_signed(int(seed)), _signed(int(counter))], dtype=torch.int64))


def draw(device=None):
    """Enqueue one draw on the current stream -> the ticket (int32 [4] device tensor) the dropout kernels of one block forward read."""
    st = state_tensor(device)
    ticket = torch.empty(4, dtype=torch.int32, device=st.device)
    L.call('cat_rng_draw', ops._p(st), ops._p(ticket), ops._stream())
    return ticket


def threshold(p):
    """Keep an element iff its 32-bit draw is >= floor(p * 2^32) (p < 1)."""
    return min(int(p * 4294967296.0), 4294967295)
