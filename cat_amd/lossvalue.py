"""Scalar losses as weighted sums of 0-d device tensors, and the one way they are differentiated: `torch.autograd.backward` seeded with the
weights, so the hot loop never combines loss terms with torch arithmetic kernels."""
import torch

from . import ops

_CACHE = {}


def seed(device, value):
    """The constant 0-d float32 tensor `value` on `device` (a backward seed, d total / d term): one per (device, value), created on first
    use -- in the eager warm-up steps, before any capture."""
    key = (device, float(value))
    t = _CACHE.get(key)
    if t is None:
        t = _CACHE[key] = torch.full((), key[1], device=device, dtype=torch.float32)
    return t


def backward_terms(terms):
    """sum_i w_i * t_i .backward() without building the sum: [(w_i, t_i)] seeds torch.autograd.backward, in the given order."""
    terms = [(w, t) for w, t in terms if t.requires_grad]
    torch.autograd.backward([t for _, t in terms], [seed(t.device, w) for w, t in terms])
    ops.sync_side_streams()


class LossValue:
    """A scalar loss kept on the device: sum_i w_i * t_i.  float() synchronises (trainer.py:135-139 does that only every
    print_freq iterations)."""

    def __init__(self, terms):
        self.terms = [(float(w), t) for w, t in terms]

    def __float__(self):
        return float(sum(w * float(t) for w, t in self.terms))

    def item(self):
        return float(self)

    def detach(self):
        return self

    def mean(self):          # losses['loss_G'].mean() in models/spade_model.py:191 (one replica per process)
        return self

    def __mul__(self, k):
        return LossValue([(w * k, t) for w, t in self.terms])

    __rmul__ = __mul__

    def __truediv__(self, k):
        return self * (1.0 / k)

    def __add__(self, other):
        if isinstance(other, (int, float)) and other == 0:
            return self
        if isinstance(other, torch.Tensor):
            other = LossValue([(1.0, other)])
        return LossValue(self.terms + other.terms)

    __radd__ = __add__

    def backward(self):
        backward_terms(self.terms)
