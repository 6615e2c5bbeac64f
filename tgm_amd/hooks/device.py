"""DeviceTransferHook and PinMemoryHook (contract of tgm/hooks/device.py): move, or page-lock, every tensor a batch holds.

A device-resident graph materialises its batches on the device already, so a pipeline built here needs neither; scripts written against
the reference list them, and on such a batch both are the identity.  ``_relocate`` visits the batch's public dataclass fields and, through
them, lists, tuples and dicts to any depth, and offers every tensor it meets to a ``place`` function; only a tensor that ``place`` answers
with another object is stored back, so a tensor that is already where it should be stays the same object in the same container.  A tuple
cannot be stored into: it is replaced by a new one when something in it moved.  ``EdgeFeaturesById`` (core/lazy.py) moves by its backing
tensors -- the edge ids, the table, whatever was gathered already -- and stays lazy.  Pure Python, no kernel.
"""
from __future__ import annotations

import dataclasses
from typing import Any, Callable, Iterator, List, Set, Tuple, Union

import torch
from torch import Tensor

from ..core import DGBatch, DGraph
from ..core.lazy import EdgeFeaturesById
from .base import StatelessHook
from .registry import hook

Place = Callable[[Tensor], Tensor]
Store = Callable[[Any, Any], None]


def _slots(holder: Any) -> Tuple[Iterator[Tuple[Any, Any]], Store]:
    """The (key, value) slots of a mutable holder and the call that stores into one; nothing for anything else."""
    if isinstance(holder, EdgeFeaturesById):  # list.__getitem__ reads the cache as it is (None: not gathered yet) instead of gathering
        cached = [(h, list.__getitem__(holder, h)) for h in range(len(holder))]
        return iter(cached + [('eids', holder.eids), ('table', holder.table)]), lambda k, v: setattr(holder, k, v) if isinstance(k, str) else list.__setitem__(holder, k, v)
    if isinstance(holder, list):
        return iter(list(enumerate(holder))), holder.__setitem__
    if isinstance(holder, dict):
        return iter(list(holder.items())), holder.__setitem__
    if dataclasses.is_dataclass(holder) and not isinstance(holder, type):
        public = [(name, value) for name, value in vars(holder).items() if not name.startswith('_')]  # (the loader's bookkeeping is private)
        return iter(public), lambda name, value: setattr(holder, name, value)
    return iter(()), lambda k, v: None


def _placed_tuple(items: tuple, place: Place, todo: List[Any]) -> tuple:
    """`items` with its tensors placed (nested tuples likewise); mutable holders inside it are queued on `todo` and keep their identity."""
    out = []
    for item in items:
        if torch.is_tensor(item):
            item = place(item)
        elif isinstance(item, tuple):
            item = _placed_tuple(item, place, todo)
        else:
            todo.append(item)
        out.append(item)
    return items if all(a is b for a, b in zip(items, out)) else tuple(out)


def _relocate(batch: Any, place: Place) -> None:
    todo: List[Any] = [batch]
    visited: Set[int] = set()  # a holder reachable twice (or through itself) is walked once
    while todo:
        holder = todo.pop()
        if id(holder) in visited:
            continue
        visited.add(id(holder))
        slots, store = _slots(holder)
        for key, value in slots:
            if torch.is_tensor(value):
                moved = place(value)
            elif isinstance(value, tuple):
                moved = _placed_tuple(value, place, todo)
            else:
                todo.append(value)
                continue
            if moved is not value:
                store(key, moved)


@hook
class PinMemoryHook(StatelessHook):
    """Pin all host tensors in the batch to page-locked memory; does nothing where no device is available.

    Key words: cpu, gpu, cuda, non-pageable memory.
    """

    def __call__(self, dg: DGraph, batch: DGBatch) -> DGBatch:
        if torch.cuda.is_available():
            _relocate(batch, lambda t: t.pin_memory() if t.device.type == 'cpu' and not t.is_pinned() else t)
        return batch


@hook
class DeviceTransferHook(StatelessHook):
    """Move all tensors in the batch to ``device`` (``non_blocking=True``).

    Key words: cpu, gpu, cuda, device transfer.
    """

    def __init__(self, device: Union[str, torch.device]) -> None:
        super().__init__()
        self.device = torch.device(device)

    def __call__(self, dg: DGraph, batch: DGBatch) -> DGBatch:
        # (Tensor.to answers with the tensor itself when it is there already, also for 'cuda' against 'cuda:0')
        _relocate(batch, lambda t: t.to(self.device, non_blocking=True))
        return batch
