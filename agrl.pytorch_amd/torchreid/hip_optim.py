"""The optimiser update of the train step on the library's own kernel (csrc/optim.hip): ``optimizer.step()`` of the reference's
``train()`` (train_vidreid_xent_htri.py:411-413) for the optimisers its ``optimizers.init_optim`` builds from torch (optimizers.py:7-15).

``HipAdam`` / ``HipSGD`` ARE ``torch.optim.Adam`` / ``torch.optim.SGD``: the same ``param_groups``, ``state`` and ``state_dict()``
(Adam: ``step``, ``exp_avg``, ``exp_avg_sq`` [, ``max_exp_avg_sq``]; SGD: ``momentum_buffer``), so ``set_wd``, ``adjust_learning_rate``, the
reference's lr schedulers and checkpoints work unchanged and a state dict moves between the native and the stock class in both
directions. Only ``step()`` differs: on CUDA parameters every launch class -- the parameters of one group that have a gradient
and share a step count (Adam) or a first-step flag (SGD) -- is ONE multi-tensor launch (``agrl_adam_step`` / ``agrl_sgd_step``) that
reads p, g and the state once, writes p and the state once and, with ``zero_grads``, stores +0.0 over the gradients it consumed.
There is no per-tensor launch, no synchronisation, and after the first step no allocation: the device tables of a launch class are
cached under the pointer set they describe, so a table is rebuilt (one host-to-device copy) only when a pointer or the active set
changed -- a re-allocated ``.grad``, ``load_state_dict``, an htri-only step after an xent + htri one (both sets stay cached).

CPU parameters take the stock ``step()``: the reference's own CPU-runnable configuration, as everywhere in this package. On CUDA
without the library ``step()`` raises ``HipLibraryError``. This module is NOT named ``optimizers``: ``torchreid.optimizers`` stays the
reference's (rmsprop / adabound / radam live there)."""
from __future__ import annotations

import collections
import math
import weakref

import numpy as np
import torch

from . import _hip

CHUNK = 4096        # elements per chunk, MAX_GRID workgroups at most, WORDS int64 words per descriptor: csrc/optim.hip's constants
MAX_GRID = 2048     # (checked against agrl_optim_geometry at the first native step)
WORDS = 8
MAX_TABLES = 16     # cached launch classes per optimiser (least recently used goes first)
STEP_BLOCK = 1024   # step counts per shared CPU block (NativeStepMixin._step_view)


def build_chunk_table(numels, chunk=CHUNK):
    """int32 (n_chunks, 2) rows {tensor, chunk index inside the tensor}: chunk c of tensor t covers its elements
    [c * chunk, min(numel, (c + 1) * chunk)); every element of every tensor is in exactly one chunk, tensors in order."""
    numels = np.asarray(numels, dtype=np.int64).reshape(-1)
    if numels.size == 0 or (numels <= 0).any():
        raise ValueError("build_chunk_table: every tensor needs at least one element")
    counts = (numels + (chunk - 1)) // chunk
    if int(counts.max()) > np.iinfo(np.int32).max or int(counts.sum()) > np.iinfo(np.int32).max:
        raise ValueError("build_chunk_table: too many chunks for an int32 table")
    first = np.cumsum(counts) - counts
    table = np.empty((int(counts.sum()), 2), dtype=np.int32)
    table[:, 0] = np.repeat(np.arange(numels.size, dtype=np.int64), counts)
    table[:, 1] = np.arange(table.shape[0], dtype=np.int64) - np.repeat(first, counts)
    return table


def build_descriptors(rows):
    """rows of (param, grad, state0, state1, state2, numel) pointers / counts -> int64 (n, WORDS) descriptor table; the vec word is
    set where every non-null pointer of the row is 16-byte aligned."""
    desc = np.zeros((len(rows), WORDS), dtype=np.int64)
    for i, row in enumerate(rows):
        desc[i, :6] = row
        desc[i, 6] = 1 if all(ptr % 16 == 0 for ptr in row[:5]) else 0
    return desc


def adam_constants(lr, beta1, beta2, step):
    """The step's constants in double (the launch rounds each once to fp32): 1 - beta1, beta2, 1 - beta2, lr / (1 - beta1^t),
    1 / sqrt(1 - beta2^t)."""
    return (1.0 - beta1, beta2, 1.0 - beta2, lr / (1.0 - beta1 ** step), 1.0 / math.sqrt(1.0 - beta2 ** step))


class NativeStepMixin(object):
    """What HipAdam and HipSGD share: routing, validation, the cached device tables."""

    def _native_init(self, zero_grads):
        self.zero_grads = bool(zero_grads)
        self._tables = collections.OrderedDict()
        self._geometry_checked = False

    def load_state_dict(self, state_dict):
        """As in torch; what the native route remembered about the replaced state (records, device tables) goes with it."""
        super().load_state_dict(state_dict)
        self._recs, self._tables, self._step_blocks, self._block_vers = {}, collections.OrderedDict(), [], {}

    def _records(self):
        """id(parameter) -> _Record: what lets a step skip re-validating tensors it has already seen (never pickled)."""
        recs = getattr(self, "_recs", None)
        if recs is None:
            recs = self._recs = {}
        return recs

    def _step_view(self, step):
        """-> (0-dim view holding the count ``step``, block index, slot). The per-parameter ``step`` tensors of the native route are
        views into shared CPU blocks of STEP_BLOCK floats, so that advancing every count of a block is ONE tensor operation instead
        of one per parameter; to state_dict(), torch.save and the stock optimisers they are ordinary 0-dim float32 tensors."""
        blocks = getattr(self, "_step_blocks", None)
        if blocks is None:
            blocks = self._step_blocks = []
        if torch.is_tensor(step) and not step.is_cuda and step.dim() == 0 and step.dtype == torch.float32:
            for bi, (block, used) in enumerate(blocks):      # already one of ours (the state survived, the record did not)
                if step.untyped_storage().data_ptr() == block.untyped_storage().data_ptr() and step.storage_offset() < used:
                    return step, bi, step.storage_offset()
        if not blocks or blocks[-1][1] == STEP_BLOCK:
            blocks.append([torch.zeros(STEP_BLOCK, dtype=torch.float32), 0])
        block, slot = blocks[-1][0], blocks[-1][1]
        blocks[-1][1] += 1
        block[slot] = float(step)
        return block[slot], len(blocks) - 1, slot

    def _sync_counts(self):
        """Before a step touches any count: a block somebody else wrote into since its counts were last advanced (its version
        counter moved) makes every record of that block read its tensor again."""
        vers = self._block_versions()
        for bi, (block, _) in enumerate(getattr(self, "_step_blocks", None) or ()):
            if block._version != vers.get(bi):
                for rec in self._records().values():
                    if getattr(rec, "block", None) == bi:
                        rec.val = int(rec.step.item())
                vers[bi] = block._version

    def _block_versions(self):
        vers = getattr(self, "_block_vers", None)
        if vers is None:
            vers = self._block_vers = {}
        return vers

    def _advance_steps(self, counted):
        """+1 on the count tensor of every record in ``counted`` (their ``val`` already advanced): one operation per block."""
        slots = collections.defaultdict(list)
        for rec in counted:
            slots[rec.block].append(rec.slot)
        for bi, hit in slots.items():
            block, used = self._step_blocks[bi]
            if len(hit) == used:
                block[:used] += 1
            else:
                block[torch.tensor(hit, dtype=torch.int64)] += 1
            self._block_versions()[bi] = block._version

    def _all_cpu(self):
        return all(not p.is_cuda for group in self.param_groups for p in group["params"])

    def _stock_step(self, closure, zero):
        """CPU parameters: the stock optimiser's step (called once -- not through a second layer of the step hooks)."""
        fn = super(NativeStepMixin, type(self)).step
        if getattr(fn, "hooked", False):
            fn = fn.__wrapped__
        loss = fn(self, closure)
        if zero:
            with torch.no_grad():
                for group in self.param_groups:
                    for p in group["params"]:
                        if p.grad is not None:      # what the step consumed
                            p.grad.zero_()
        return loss

    def _refuse(self, group, flags):
        for flag in flags:
            if group.get(flag):
                raise NotImplementedError("%s: %s=True is not implemented by the native step (use torch.optim on the reference's "
                                          "torchreid.optimizers route)" % (type(self).__name__, flag))

    @staticmethod
    def _check_tensors(p, g):
        if not p.is_cuda:
            raise ValueError("native optimiser step: CPU and CUDA parameters in one optimiser")
        if p.dtype != torch.float32:
            raise TypeError("native optimiser step: parameters must be float32, got %s" % p.dtype)
        if not p.is_contiguous():
            raise ValueError("native optimiser step: parameters must be contiguous (shape %s, strides %s)" % (tuple(p.shape), p.stride()))
        if g.is_sparse or g.layout != torch.strided:
            raise NotImplementedError("native optimiser step: sparse gradients are not implemented")
        if g.dtype != torch.float32:
            raise TypeError("native optimiser step: gradients must be float32, got %s" % g.dtype)
        if g.device != p.device or g.shape != p.shape or not g.is_contiguous():
            raise ValueError("native optimiser step: a gradient must be a contiguous tensor of its parameter's shape on its device")

    @staticmethod
    def _check_state(p, s, name):
        if s.dtype != torch.float32 or s.device != p.device or s.shape != p.shape or not s.is_contiguous():
            raise ValueError("native optimiser step: state %r must be a contiguous float32 tensor of its parameter's shape on its device" % name)
        return s.data_ptr()

    def _tables_for(self, device, rows):
        """(descriptor table, chunk table) on ``device`` for these rows, from the cache when this exact pointer set was seen before."""
        from . import hip_ops as ops
        if not getattr(self, "_geometry_checked", False):
            if ops.optim_geometry() != (CHUNK, MAX_GRID, WORDS):
                raise _hip.HipLibraryError("%s was built with optimiser geometry %r, this module expects %r" % (
                    _hip.LIB_PATH, ops.optim_geometry(), (CHUNK, MAX_GRID, WORDS)))
            self._geometry_checked = True
        if getattr(self, "_tables", None) is None:
            self._tables = collections.OrderedDict()
        key = (device.index, tuple(rows))
        entry = self._tables.get(key)
        if entry is not None:
            self._tables.move_to_end(key)
            return entry[0], entry[1]
        host_desc = torch.from_numpy(build_descriptors(rows)).pin_memory()
        host_chunks = torch.from_numpy(build_chunk_table([row[5] for row in rows])).pin_memory()
        # the pinned sources stay in the entry: the copies are asynchronous on the current stream, ahead of the launch that reads them
        entry = (host_desc.to(device, non_blocking=True), host_chunks.to(device, non_blocking=True), host_desc, host_chunks)
        self._tables[key] = entry
        while len(self._tables) > MAX_TABLES:
            self._tables.popitem(last=False)
        return entry[0], entry[1]

    def _begin(self, closure, zero_grads):
        """-> (loss, zero flag) for the native route: the closure as in torch, the library present."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        _hip.lib()
        return loss, (getattr(self, "zero_grads", False) if zero_grads is None else bool(zero_grads))


class _Record(object):
    """What a step learned about one parameter, trusted again while the very same tensor objects sit at the very same addresses:
    the validated gradient (a weak reference: a record must not keep a released gradient's memory) and state tensors, the
    descriptor row, the step count (``val``) and where its tensor lives."""
    __slots__ = ("p", "g", "state", "s0", "s1", "s2", "row", "device", "step", "block", "slot", "val")


class HipAdam(NativeStepMixin, torch.optim.Adam):
    """torch.optim.Adam (amsgrad=True: AMSGrad) whose step on CUDA parameters is one agrl_adam_step launch per launch class.
    ``zero_grads`` (constructor flag or ``step(zero_grads=...)``, default off): the step leaves every gradient it consumed allocated
    and filled with +0.0 -- the zero-fill rides on the update's own pass."""

    def __init__(self, params, *args, zero_grads=False, **kwargs):
        super().__init__(params, *args, **kwargs)
        self._native_init(zero_grads)

    def _adam_record(self, rec, p, g, amsgrad):
        """Lazy state as in torch, everything validated -> the parameter's record (``rec`` is reused when there is one)."""
        state = self.state[p]
        if len(state) == 0:
            state["step"] = 0.0
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if amsgrad:
                state["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        rec = rec if rec is not None else _Record()
        # the count lives on the host, as in torch (a device tensor, from a capturable / fused optimiser's state dict, is read once)
        rec.step, rec.block, rec.slot = self._step_view(state["step"])
        state["step"] = rec.step
        rec.val = int(rec.step.item())
        rec.p, rec.g, rec.state, rec.device = p, weakref.ref(g), state, p.device
        rec.s0, rec.s1, rec.s2 = state["exp_avg"], state["exp_avg_sq"], state["max_exp_avg_sq"] if amsgrad else None
        rec.row = (p.data_ptr(), g.data_ptr(), self._check_state(p, rec.s0, "exp_avg"), self._check_state(p, rec.s1, "exp_avg_sq"),
                   self._check_state(p, rec.s2, "max_exp_avg_sq") if amsgrad else 0, p.numel())
        return rec

    @torch.no_grad()
    def step(self, closure=None, *, zero_grads=None):
        if self._all_cpu():
            return self._stock_step(closure, getattr(self, "zero_grads", False) if zero_grads is None else bool(zero_grads))
        from . import hip_ops as ops
        loss, zero = self._begin(closure, zero_grads)
        recs, states = self._records(), self.state
        items = []
        for gi, group in enumerate(self.param_groups):
            self._refuse(group, ("maximize", "capturable", "differentiable", "decoupled_weight_decay"))
            amsgrad = bool(group["amsgrad"])
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                rec = recs.get(id(p))
                if rec is not None and rec.p is p and rec.g() is g and states.get(p) is rec.state:
                    state, row = rec.state, rec.row
                    if (state.get("exp_avg") is rec.s0 and state.get("exp_avg_sq") is rec.s1 and state.get("step") is rec.step
                            and (state.get("max_exp_avg_sq") is rec.s2 if amsgrad else rec.s2 is None)
                            and p.data_ptr() == row[0] and g.data_ptr() == row[1] and rec.s0.data_ptr() == row[2]
                            and rec.s1.data_ptr() == row[3] and (not amsgrad or rec.s2.data_ptr() == row[4])):
                        items.append((gi, rec, None))
                        continue
                self._check_tensors(p, g)       # a tensor changed hands or moved: validate again (nothing is written in this pass)
                items.append((gi, rec, (p, g, amsgrad)))
        classes, counted = collections.OrderedDict(), []
        self._sync_counts()
        for gi, rec, todo in items:
            if todo is not None:
                rec = recs[id(todo[0])] = self._adam_record(rec, *todo)
            rec.val += 1
            counted.append(rec)
            if rec.row[5] > 0:
                classes.setdefault((gi, rec.device, rec.val), []).append(rec.row)
        self._advance_steps(counted)
        for (gi, device, t), rows in classes.items():
            group = self.param_groups[gi]
            beta1, beta2 = (float(b) for b in group["betas"])
            tensors, chunks = self._tables_for(device, rows)
            ops.adam_step(tensors, chunks, float(group["weight_decay"]), *adam_constants(float(group["lr"]), beta1, beta2, t),
                          float(group["eps"]), group["amsgrad"], zero)
        return loss


class HipSGD(NativeStepMixin, torch.optim.SGD):
    """torch.optim.SGD (momentum, Nesterov momentum, dampening 0) whose step on CUDA parameters is one agrl_sgd_step launch per
    launch class; ``zero_grads`` as for HipAdam."""

    def __init__(self, params, *args, zero_grads=False, **kwargs):
        super().__init__(params, *args, **kwargs)
        self._native_init(zero_grads)

    @torch.no_grad()
    def step(self, closure=None, *, zero_grads=None):
        if self._all_cpu():
            return self._stock_step(closure, getattr(self, "zero_grads", False) if zero_grads is None else bool(zero_grads))
        from . import hip_ops as ops
        loss, zero = self._begin(closure, zero_grads)
        recs, states = self._records(), self.state
        items = []
        for gi, group in enumerate(self.param_groups):
            self._refuse(group, ("maximize", "differentiable"))
            if group["dampening"] != 0:
                raise NotImplementedError("HipSGD: dampening is not implemented by the native step")
            momentum = group["momentum"] != 0
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                rec = recs.get(id(p))
                if rec is not None and rec.p is p and rec.g() is g and p.data_ptr() == rec.row[0] and g.data_ptr() == rec.row[1]:
                    if not momentum and rec.s0 is None:
                        items.append((gi, rec, None))
                        continue
                    if momentum and rec.s0 is not None and states[p].get("momentum_buffer") is rec.s0 and rec.s0.data_ptr() == rec.row[2]:
                        items.append((gi, rec, None))
                        continue
                self._check_tensors(p, g)
                items.append((gi, rec, (p, g, momentum)))
        classes = collections.OrderedDict()
        for gi, rec, todo in items:
            first = False
            if todo is not None:
                p, g, momentum = todo
                rec = recs[id(p)] = rec if rec is not None else _Record()
                rec.p, rec.g, rec.s0, rec.device, buf = p, weakref.ref(g), None, p.device, 0
                if momentum:
                    state = self.state[p]
                    first = state.get("momentum_buffer") is None
                    if first:
                        state["momentum_buffer"] = torch.empty_like(p, memory_format=torch.preserve_format)   # written by this step
                    rec.s0 = state["momentum_buffer"]
                    buf = self._check_state(p, rec.s0, "momentum_buffer")
                rec.row = (p.data_ptr(), g.data_ptr(), buf, 0, 0, p.numel())
            if rec.row[5] > 0:
                classes.setdefault((gi, rec.device, first), []).append(rec.row)
        for (gi, device, first), rows in classes.items():
            group = self.param_groups[gi]
            tensors, chunks = self._tables_for(device, rows)
            ops.sgd_step(tensors, chunks, float(group["weight_decay"]), float(group["momentum"]), float(group["lr"]),
                         group["momentum"] != 0, first, group["nesterov"], zero)
        return loss


def init_optim(optim, params, lr, weight_decay):
    """The reference's ``optimizers.init_optim`` (optimizers.py:7-23) for the optimisers it builds from torch, as the native classes
    with the same hyper-parameters; the driver's one-line change is ``from torchreid.hip_optim import init_optim``."""
    if optim == 'adam':
        return HipAdam(params, lr=lr, weight_decay=weight_decay)
    elif optim == 'amsgrad':
        return HipAdam(params, lr=lr, weight_decay=weight_decay, amsgrad=True)
    elif optim == 'sgd':
        return HipSGD(params, lr=lr, momentum=0.9, weight_decay=weight_decay)
    elif optim == 'nesterov':
        return HipSGD(params, lr=lr, momentum=0.9, weight_decay=weight_decay, nesterov=True)
    elif optim in ('rmsprop', 'adabound', 'radam'):
        raise NotImplementedError("optimizer %r has no native step: build it with the reference's torchreid.optimizers.init_optim" % optim)
    else:
        raise KeyError("Unsupported optimizer: {}".format(optim))
