"""The operand caches of the natively trained BaseConv weights: one record per weight, one freshness test.

``frlw_baseconv_train_fwd`` / ``_bwd`` read the re-laid GEMM operands of a weight (forward + data-gradient operand) from a
caller-owned cache: ``w == NULL`` in the forward says "the cache is ready", ``w_cache != NULL`` in the backward "the forward's
operands are still valid".  A wrong yes runs a convolution on another weight's or on stale operands and returns FRLW_OK, so it is
asked in one place, ``WeightOperands.holds``: by the forward, the backward (train_ops.py) and the batched layout's plan below."""
from __future__ import annotations

import os
import weakref
from collections import namedtuple
from typing import NamedTuple

import torch

from .. import _lib, _pins

_RECORDS = {}  # id(weight; of a stacked pair: the first one) -> WeightOperands; the weight's weakref callback drops the entry
_PLANS = {}    # id(model) -> _Plan of layout_all_weights; the model's weakref callback drops the entry


def native_enabled():
    return os.environ.get("FRLW_NATIVE_TRAIN", "1") != "0"


class Key(NamedTuple):
    """What one layout writes and what a reader asks for: both operands, in the buffer at ``cache``, of the weight that lies at ``ptrs``
    (two entries: stacked on a second weight), for one parity class and precision, laid out from these in-place ``versions``."""
    cache: int
    ptrs: tuple
    parity: int
    precision: int
    versions: tuple


class WeightOperands:
    """The operand cache of one weight: whose it is, the buffer and what the buffer holds."""
    __slots__ = ("ref", "second", "cache", "written", "batched", "__weakref__")

    def __init__(self, weight):
        self.ref = weakref.ref(weight, lambda _r, key=id(weight): _RECORDS.pop(key, None))  # nothing keyed by id outlives its tensor
        self.second = None    # weakref of the second weight while the weight runs as the first of a stacked pair
        self.cache = None     # float32 buffer: the forward operand, then the data-gradient operand
        self.written = None   # the Key of the last layout into ``cache`` (None: it holds nothing)
        self.batched = False  # ... which the batched launch wrote (True) or a forward's own layout kernels

    def weights(self):
        """(weight,) or (weight, second weight); None once one of them is gone."""
        both = (self.ref(),) if self.second is None else (self.ref(), self.second())
        return None if any(t is None for t in both) else both

    def key(self, parity, precision):
        """The Key a layout of the weight(s) as they are now writes."""
        both = self.weights()
        return Key(self.cache.data_ptr(), tuple(t.data_ptr() for t in both), parity, precision, tuple(t._version for t in both))

    def holds(self, key, any_version=False):
        """THE freshness test: the cache holds what ``key`` names, and that is what a layout of the weights as they are now would
        write -- the same buffer, weight(s) and addresses, parity class, precision and versions.  ``any_version``: whatever
        the versions (the batched launch asks whether its table still fits; it is about to write the current ones)."""
        n = 4 if any_version else 5
        return (self.written is not None and self.weights() is not None
                and self.key(key.parity, key.precision)[:n] == key[:n] == self.written[:n])


def operands_of(lib, weight, weight2, Cin, Cout, k):
    """The record of ``weight`` (created on first use) with a cache large enough for both operands of a (Cout, Cin, k, k) layer
    in either precision; ``weight2``: the weight runs as the first of a stacked pair with it (None: on its own).  A buffer that
    is replaced is retired (a live HIP graph may still launch on it); the new one holds nothing."""
    rec = _RECORDS.get(id(weight))
    if rec is None or rec.ref() is not weight:  # (an id is a tensor's own only while the tensor lives)
        rec = _RECORDS[id(weight)] = WeightOperands(weight)
    rec.second = None if weight2 is None else weakref.ref(weight2)
    n = lib.frlw_baseconv_weight_cache_floats(Cin, Cout, k, 1)  # room for either precision
    if rec.cache is None or rec.cache.numel() < n or rec.cache.device != weight.device:
        _pins.retire(rec.cache)
        rec.cache, rec.written = torch.empty(int(n), dtype=torch.float32, device=weight.device), None
    return rec


# one model's batched layout: weakref, device table of frlw_weight_layout_item_t, its elements, [(record, Key the entry writes), ...]
_Plan = namedtuple("_Plan", "model table total rows")


def _layout_plan(model):
    """One table entry per natively trained BaseConv weight of `model` whose operand cache has been written (= that has run
    one forward), for the parity class and precision of that write; the first weight of a stacked pair stands for both
    (Cout = the pair's channels, w2 / split = the second weight)."""
    lib = _lib.load()
    rows, items, first = [], [], 0
    for mod in model.modules():
        conv, bn = getattr(mod, "conv", None), getattr(mod, "bn", None)
        if not isinstance(conv, torch.nn.Conv2d) or not isinstance(bn, torch.nn.BatchNorm2d):
            continue
        w = conv.weight
        rec = _RECORDS.get(id(w))
        both = rec.weights() if rec is not None and rec.ref() is w and rec.written is not None else None
        if both is None or not all(t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 for t in both):
            continue
        key = rec.key(rec.written.parity, rec.written.precision)
        Cout, Cin, k = sum(t.shape[0] for t in both), w.shape[1], w.shape[2]
        n_f, n_d = (lib.frlw_conv_operand_floats(k * k * a, b, key.precision) for a, b in ((Cin, Cout), (Cout, Cin)))
        if rec.cache.numel() < n_f + n_d:
            continue
        items.append(_lib.FrlwWeightLayoutItem(w=key.ptrs[0], w_fwd=key.cache, w_dgrad=key.cache + 4 * n_f, Cout=Cout, Cin=Cin, k=k,
                                               dgrad_parity=key.parity, precision=key.precision, first=first,
                                               w2=key.ptrs[1] if len(both) == 2 else None, split=w.shape[0] if len(both) == 2 else 0))
        first += n_f + n_d
        rows.append((rec, key))
    if not rows:
        return None
    table = torch.frombuffer(bytearray((_lib.FrlwWeightLayoutItem * len(items))(*items)), dtype=torch.uint8).to(rows[0][0].cache.device)
    return _Plan(weakref.ref(model, lambda _r, key=id(model): _PLANS.pop(key, None)), table, first, rows)


def layout_all_weights(model):
    """Lay out the GEMM operands of EVERY BaseConv weight of `model` in one launch (call it once per step, before the
    forward: the per-layer forwards then find their cache ready and skip their own layout kernel -- 74 launches of ~5 us).
    Does nothing until the layers have run once (their caches are created by the first forward), or off the GPU."""
    if not native_enabled():
        return False
    plan = _PLANS.get(id(model))
    if plan is None or plan.model() is not model or not all(rec.holds(key, any_version=True) for rec, key in plan.rows):
        if plan is not None:
            _pins.retire(plan.table)  # the item table a captured layout launch reads
        plan = _PLANS[id(model)] = _layout_plan(model)
        if plan is None:
            del _PLANS[id(model)]
            return False
    _lib.check(_lib.load().frlw_conv_weight_layouts_batch(plan.table.data_ptr(), len(plan.rows), plan.total,
                                                          torch.cuda.current_stream(plan.table.device).cuda_stream), "weight_layouts_batch")
    for i, (rec, key) in enumerate(plan.rows):
        rec.written, rec.batched = rec.key(key.parity, key.precision), True  # (the same entry, at the versions just laid out)
        plan.rows[i] = (rec, rec.written)
    return True
