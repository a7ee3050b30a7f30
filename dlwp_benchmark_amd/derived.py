"""The one rule for values derived from parameters (packed bf16 / f16 weight images, transposed weights, descriptors, plans,
step graphs): a value is cached and re-derived when a source tensor's (data_ptr, _version) or device changes, or when the pack
epoch does.  Writes through `.data` change neither pointer nor version; HipBackbone.invalidate_packed() (called by
load_state_dict / _apply, and by users after such writes) bumps the epoch, which is part of every key."""
import functools
import weakref

import torch

_EPOCH = [0]


def pack_epoch() -> int:
    return _EPOCH[0]


def bump_pack_epoch() -> int:
    _EPOCH[0] += 1
    return _EPOCH[0]


def source_key(*tensors, extra=()):
    """The key of a value derived from `tensors` (None: an absent optional source) and the tuple of plain values `extra`.  (The
    device goes in as the torch.device itself: it compares like its string and costs half as much on a per-step key.)"""
    return (*[None if t is None else (t.data_ptr(), t._version, t.device) for t in tensors], extra, _EPOCH[0])


class Derived:
    """One cached derived value.  eager_only="<name>": deriving allocates and launches, so a stale or missing value inside a
    graph capture is an error."""

    def __init__(self, eager_only=None):
        self._key = None
        self._value = None
        self._eager_only = eager_only

    def get(self, key, build):
        if key != self._key:
            if self._eager_only and torch.cuda.is_current_stream_capturing():
                from .lib import DlwpError

                raise DlwpError(f"{self._eager_only}: the weight pack must be made before a graph capture (run one eager step first)")
            self._value = build()
            self._key = key
        return self._value


# (id(tensor), slot) -> (weak reference, holder): a holder lives exactly as long as the tensor it belongs to (the finalizer
# drops it), so a captured step graph -- which keeps its module, hence its parameters, alive -- never replays against a freed
# value; nothing here is ever cleared wholesale
_HOLDERS = {}


def _drop(k, ref) -> None:
    hit = _HOLDERS.get(k)
    if hit is not None and hit[0] is ref:       # (ids are reused after a free: only the entry of THIS tensor)
        del _HOLDERS[k]


def derived_for(tensor: torch.Tensor, slot, make=Derived):
    """The holder (`make()`, created on first use) of `slot` that belongs to `tensor`: a Parameter, or any tensor the caller
    keeps alive."""
    k = (id(tensor), slot)
    hit = _HOLDERS.get(k)
    if hit is None or hit[0]() is not tensor:
        hit = (weakref.ref(tensor, functools.partial(_drop, k)), make())
        _HOLDERS[k] = hit
    return hit[1]


def live_holders() -> int:
    return len(_HOLDERS)
