"""The one keyed cache of operands derived from weights, Adam state and running statistics ("Derived operands and their keys").

The kernels change those tensors through raw pointers, so every cached operand carries the key it was derived under -- an
`optim.weights_key` / `optim.pack_key` plus explicit extras (mode, plan signature, input shape) -- and lives in a SLOT: an attribute name
declared once through `slot()`, as a module-level constant next to its user.  `lookup` is the only way an entry is compared and stored,
`drop` / `drop_derived` the only way one is thrown away, so a cache that is declared is also invalidated by a parameter broadcast.
The fused-unit plans (R7) and the quad-granule layers (`_cat_q`, the holders of R8) keep their own staleness rules: their slots hold the
object itself, not an Entry, and are declared only so that `drop` covers them."""
from collections import namedtuple

from . import optim

Entry = namedtuple('Entry', 'key value')

SLOTS = []      # every declared attribute name


def slot(name):
    """Declare the attribute `name` as a cache slot; returns the name."""
    if name not in SLOTS:
        SLOTS.append(name)
    return name


def peek(holder, slot, sub=None):
    """The Entry cached on `holder` under `slot` (of its sub-key `sub` where the slot holds one entry per mode), or None."""
    ent = holder.__dict__.get(slot)
    return ent if sub is None or ent is None else ent.get(sub)


def lookup(holder, slot, key, make, sub=None):
    """The cached value if it was derived under `key`; else `make(prev)` -- prev: the stale Entry or None; make refreshes prev.value in place
    and returns it where the operand's address must stay put, or allocates -- stored under `key`."""
    prev = peek(holder, slot, sub)
    if prev is not None and prev.key == key:
        return prev.value
    ent = Entry(key, make(prev))
    if sub is None:
        holder.__dict__[slot] = ent
    else:
        holder.__dict__.setdefault(slot, {})[sub] = ent
    return ent.value


def drop(obj):
    """Forget every derived operand cached on `obj`."""
    for name in SLOTS:
        obj.__dict__.pop(name, None)


def drop_derived(modules):
    """The values under `modules` were overwritten through `.data` (no version bump): drop every operand derived from the old ones, on the
    parameters, buffers and sub-modules, and advance the weights epoch for whatever is cached elsewhere."""
    for m in modules:
        for obj in [*m.parameters(), *m.buffers(), *m.modules()]:
            drop(obj)
    optim._bump_weights_epoch()
