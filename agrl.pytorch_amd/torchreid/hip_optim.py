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
without the library ``step()`` raises ``HipLibraryError``.

The other three names of ``init_optim`` have native classes too, on the same kernel skeleton and the same routing:
``HipRMSprop`` IS ``torch.optim.RMSprop`` (``agrl_rmsprop_step``, one launch per group); ``HipAdaBound`` and ``HipRAdam`` restate the
reference's own ``AdaBound`` / ``RAdam`` classes (optimizers.py:26-211; torch ships neither rule) with the reference's constructor
signatures, group keys and state keys, so state dicts move both ways; their launch classes are keyed on the step count like Adam's
(``agrl_adabound_step`` / ``agrl_radam_step``), and they carry the rule a second time as per-tensor torch operations for CPU
parameters and for ``hip_native = False``. ``init_optim_native`` builds all seven names; ``init_optim`` keeps refusing the three.
This module is NOT named ``optimizers``: ``torchreid.optimizers`` stays the reference's."""
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
    """What every native optimiser class shares: routing, validation, the cached device tables."""

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

    @staticmethod
    def _mark_written(ops, recs, zero):
        """After the launches of a step: the kernels wrote the parameters, the state tensors and, with ``zero``, the gradients of ``recs``
        through raw pointers. One version bump over all of them (hip_ops.written) makes the step visible the way torch.optim's is: the
        eval forward's pack cache rebuilds (models/_resnet_hip.fingerprint), and a backward through a graph recorded before the step
        raises torch's in-place-modification error instead of differentiating against the stepped weights."""
        tensors = []
        for rec in recs:
            tensors.append(rec.p)
            if rec.s0 is not None:
                tensors.append(rec.s0)
            if rec.s1 is not None:
                tensors.append(rec.s1)
            if rec.s2 is not None:
                tensors.append(rec.s2)
            if zero:
                g = rec.g()
                if g is not None:
                    tensors.append(g)
        if tensors:
            ops.written(tensors)


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
        self._mark_written(ops, counted, zero)
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
        classes, stepped = collections.OrderedDict(), []
        for gi, rec, todo in items:
            first = False
            if todo is not None:
                p, g, momentum = todo
                rec = recs[id(p)] = rec if rec is not None else _Record()
                rec.p, rec.g, rec.s0, rec.device, buf = p, weakref.ref(g), None, p.device, 0
                rec.s1 = rec.s2 = None
                if momentum:
                    state = self.state[p]
                    first = state.get("momentum_buffer") is None
                    if first:
                        state["momentum_buffer"] = torch.empty_like(p, memory_format=torch.preserve_format)   # written by this step
                    rec.s0 = state["momentum_buffer"]
                    buf = self._check_state(p, rec.s0, "momentum_buffer")
                rec.row = (p.data_ptr(), g.data_ptr(), buf, 0, 0, p.numel())
            stepped.append(rec)
            if rec.row[5] > 0:
                classes.setdefault((gi, rec.device, first), []).append(rec.row)
        for (gi, device, first), rows in classes.items():
            group = self.param_groups[gi]
            tensors, chunks = self._tables_for(device, rows)
            ops.sgd_step(tensors, chunks, float(group["weight_decay"]), float(group["momentum"]), float(group["lr"]),
                         group["momentum"] != 0, first, group["nesterov"], zero)
        self._mark_written(ops, stepped, zero)
        return loss


def adabound_constants(lr, beta1, beta2, step, final_lr, gamma, base_lr):
    """AdaBound's step constants in double (the launch rounds each once to fp32): 1 - beta1, beta2, 1 - beta2,
    step_size = lr sqrt(1 - beta2^t) / (1 - beta1^t), and the clamp bounds lower = final (1 - 1 / (gamma t + 1)),
    upper = final (1 + 1 / (gamma t)) with final = final_lr lr / base_lr (the lr schedulers move final_lr through lr)."""
    final = final_lr * lr / base_lr
    return (1.0 - beta1, beta2, 1.0 - beta2, lr * math.sqrt(1.0 - beta2 ** step) / (1.0 - beta1 ** step),
            final * (1.0 - 1.0 / (gamma * step + 1.0)), final * (1.0 + 1.0 / (gamma * step)))


def radam_constants(lr, beta1, beta2, step, weight_decay):
    """RAdam's step constants in double: 1 - beta1, beta2, 1 - beta2, decay = weight_decay lr, step_size, and whether the step takes
    the adaptive form. With N_max = 2 / (1 - beta2) - 1 and N = N_max - 2 t beta2^t / (1 - beta2^t): the step size is rectified when
    N > 5, the adaptive form runs when N > 4 -- for 4 < N <= 5 (step 5 at beta2 = 0.999) it runs with the unrectified step size."""
    beta2_t = beta2 ** step
    n_max = 2.0 / (1.0 - beta2) - 1.0
    n = n_max - 2.0 * step * beta2_t / (1.0 - beta2_t)
    step_size = lr / (1.0 - beta1 ** step)
    if n > 5:
        step_size *= math.sqrt((1.0 - beta2_t) * (n - 4.0) / (n_max - 4.0) * (n - 2.0) / n * n_max / (n_max - 2.0))
    return (1.0 - beta1, beta2, 1.0 - beta2, weight_decay * lr, step_size, n > 4)


class StatefulNativeMixin(NativeStepMixin):
    """The native step of HipRMSprop, HipAdaBound and HipRAdam: the same routing, validated-record cache and launch classes as HipAdam,
    with what differs between the rules stated by the class:

        REFUSED                  group flags the native step does not implement
        STEP_IS_TENSOR           the count is a 0-dim float32 tensor kept through _step_view (torch's classes) or a Python int
        _state_names(group)      the state keys behind the descriptor's slots {s0, s1, s2} (None: the slot is unused)
        _fill_state(state, p, group)   lazy state, as the stock class creates it
        _class_key(gi, rec)      what one launch covers: (group, device[, step count])
        _launch(ops, group, key, tensors, chunks, zero)"""
    REFUSED = ()
    STEP_IS_TENSOR = False

    def _record_holds(self, rec, names, p, g):
        state, row = rec.state, rec.row
        for k, (name, t) in enumerate(zip(names, (rec.s0, rec.s1, rec.s2))):
            if name is None:
                if t is not None:
                    return False
            elif t is None or state.get(name) is not t or t.data_ptr() != row[2 + k]:
                return False
        if self.STEP_IS_TENSOR and state.get("step") is not rec.step:
            return False
        return p.data_ptr() == row[0] and g.data_ptr() == row[1]

    def _make_record(self, rec, p, g, group, names):
        """Lazy state as in the stock class, everything validated -> the parameter's record (``rec`` is reused when there is one)."""
        state = self.state[p]
        self._fill_state(state, p, group)
        rec = rec if rec is not None else _Record()
        rec.step = rec.block = rec.slot = rec.val = None
        if self.STEP_IS_TENSOR:
            rec.step, rec.block, rec.slot = self._step_view(state["step"])
            state["step"] = rec.step
            rec.val = int(rec.step.item())
        rec.p, rec.g, rec.state, rec.device = p, weakref.ref(g), state, p.device
        rec.s0, rec.s1, rec.s2 = (state[name] if name is not None else None for name in names)
        rec.row = (p.data_ptr(), g.data_ptr()) + tuple(0 if name is None else self._check_state(p, state[name], name) for name in names) + (p.numel(),)
        return rec

    def _native_step(self, closure, zero_grads):
        from . import hip_ops as ops
        loss, zero = self._begin(closure, zero_grads)
        recs, states = self._records(), self.state
        items = []
        for gi, group in enumerate(self.param_groups):
            self._refuse(group, self.REFUSED)
            names = self._state_names(group)
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                rec = recs.get(id(p))
                if rec is not None and rec.p is p and rec.g() is g and states.get(p) is rec.state and self._record_holds(rec, names, p, g):
                    items.append((gi, rec, None))
                    continue
                self._check_tensors(p, g)       # a tensor changed hands or moved: validate again (nothing is written in this pass)
                items.append((gi, rec, (p, g, group, names)))
        classes, counted, stepped = collections.OrderedDict(), [], []
        if self.STEP_IS_TENSOR:
            self._sync_counts()
        for gi, rec, todo in items:
            if todo is not None:
                rec = recs[id(todo[0])] = self._make_record(rec, *todo)
            stepped.append(rec)
            if self.STEP_IS_TENSOR:
                rec.val += 1
                counted.append(rec)
            else:
                rec.state["step"] += 1
                rec.val = int(rec.state["step"])
            if rec.row[5] > 0:
                classes.setdefault(self._class_key(gi, rec), []).append(rec.row)
        if counted:
            self._advance_steps(counted)
        for key, rows in classes.items():
            tensors, chunks = self._tables_for(key[1], rows)
            self._launch(ops, self.param_groups[key[0]], key, tensors, chunks, zero)
        self._mark_written(ops, stepped, zero)
        return loss


class HipRMSprop(StatefulNativeMixin, torch.optim.RMSprop):
    """torch.optim.RMSprop (not centered; momentum optional) whose step on CUDA parameters is one agrl_rmsprop_step launch per
    (group, device); the same groups, state (``step``, ``square_avg`` [, ``momentum_buffer``]) and state dict as the stock class.
    ``zero_grads`` as for HipAdam."""
    REFUSED = ("centered", "maximize", "capturable", "differentiable")
    STEP_IS_TENSOR = True

    def __init__(self, params, *args, zero_grads=False, **kwargs):
        super().__init__(params, *args, **kwargs)
        self._native_init(zero_grads)

    def _state_names(self, group):
        return ("square_avg", "momentum_buffer" if group["momentum"] > 0 else None, None)

    def _fill_state(self, state, p, group):
        if len(state) == 0:
            state["step"] = 0.0
            state["square_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        if group["momentum"] > 0 and "momentum_buffer" not in state:     # starts at zero: the kernel has no first-step form
            state["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)

    def _class_key(self, gi, rec):
        return (gi, rec.device)

    def _launch(self, ops, group, key, tensors, chunks, zero):
        alpha = float(group["alpha"])
        ops.rmsprop_step(tensors, chunks, float(group["weight_decay"]), alpha, 1.0 - alpha, float(group["eps"]), float(group["momentum"]),
                         float(group["lr"]), group["momentum"] > 0, zero)

    @torch.no_grad()
    def step(self, closure=None, *, zero_grads=None):
        if self._all_cpu():
            return self._stock_step(closure, getattr(self, "zero_grads", False) if zero_grads is None else bool(zero_grads))
        return self._native_step(closure, zero_grads)


class RestatedRuleMixin(StatefulNativeMixin):
    """What HipAdaBound and HipRAdam share. Torch ships neither rule, so the class carries both routes: the native launch per
    (group, device, step count), and the same rule per tensor in torch operations (``_torch_update``) -- taken by CPU parameters,
    and by CUDA parameters while the instance attribute ``hip_native`` is False (the convention of TripletLoss.hip_native; it is what
    tools/optim_extra_bench.py measures the native step against). ``step`` is a Python int, as in the reference's classes."""

    def _init_routes(self, zero_grads):
        self._native_init(zero_grads)
        self.hip_native = True

    def _class_key(self, gi, rec):
        return (gi, rec.device, rec.val)

    def _torch_step(self, closure, zero):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            consts = {}                                  # step count -> this group's constants
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise NotImplementedError("%s: sparse gradients are not implemented" % type(self).__name__)
                state = self.state[p]
                self._fill_state(state, p, group)
                state["step"] += 1
                t = int(state["step"])
                if t not in consts:
                    consts[t] = self._constants(group, gi, t)
                self._torch_update(group, p, g, state, consts[t])
                if zero:
                    g.zero_()
        return loss

    @torch.no_grad()
    def step(self, closure=None, *, zero_grads=None):
        if self._all_cpu() or not getattr(self, "hip_native", True):
            return self._torch_step(closure, getattr(self, "zero_grads", False) if zero_grads is None else bool(zero_grads))
        return self._native_step(closure, zero_grads)


class HipAdaBound(RestatedRuleMixin, torch.optim.Optimizer):
    """AdaBound / AMSBound (Luo et al., ICLR 2019) as the reference's ``optimizers.AdaBound`` states it (optimizers.py:26-138), restated:
    the same constructor signature, defaults, ``param_groups`` keys and state keys (``step`` -- a Python int --, ``exp_avg``,
    ``exp_avg_sq`` [, ``max_exp_avg_sq``]), so a state dict moves between the two classes in both directions. Adam's moments; the
    per-element rate step_size / (sqrt(v) + eps) -- no bias correction in the denominator -- is clamped to [lower, upper], bounds that
    close in on final_lr as the count grows (adabound_constants). ``base_lrs`` is taken at construction (a group added later brings its
    own) and is not part of the state dict: final_lr follows a scheduled lr through lr / base_lr. On CUDA parameters the step is one
    agrl_adabound_step launch per (group, device, step count); ``zero_grads`` as for HipAdam."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), final_lr=0.1, gamma=1e-3, eps=1e-8, weight_decay=0, amsbound=False, *,
                 zero_grads=False):
        for name, value, ok in (("learning rate", lr, 0.0 <= lr), ("epsilon value", eps, 0.0 <= eps),
                                ("beta parameter at index 0", betas[0], 0.0 <= betas[0] < 1.0),
                                ("beta parameter at index 1", betas[1], 0.0 <= betas[1] < 1.0),
                                ("final learning rate", final_lr, 0.0 <= final_lr), ("gamma parameter", gamma, 0.0 <= gamma < 1.0)):
            if not ok:
                raise ValueError("Invalid %s: %s" % (name, value))
        super().__init__(params, dict(lr=lr, betas=betas, final_lr=final_lr, gamma=gamma, eps=eps, weight_decay=weight_decay, amsbound=amsbound))
        self.base_lrs = [group["lr"] for group in self.param_groups]
        self._init_routes(zero_grads)

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("amsbound", False)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if hasattr(self, "base_lrs"):
            self.base_lrs.append(self.param_groups[-1]["lr"])

    def _state_names(self, group):
        return ("exp_avg", "exp_avg_sq", "max_exp_avg_sq" if group["amsbound"] else None)

    def _fill_state(self, state, p, group):
        if len(state) == 0:
            state["step"] = 0
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        if group["amsbound"] and "max_exp_avg_sq" not in state:
            state["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)

    def _constants(self, group, gi, t):
        beta1, beta2 = (float(b) for b in group["betas"])
        return adabound_constants(float(group["lr"]), beta1, beta2, t, float(group["final_lr"]), float(group["gamma"]), float(self.base_lrs[gi]))

    def _launch(self, ops, group, key, tensors, chunks, zero):
        omb1, beta2, omb2, step_size, lower, upper = self._constants(group, key[0], key[2])
        ops.adabound_step(tensors, chunks, float(group["weight_decay"]), omb1, beta2, omb2, step_size, float(group["eps"]), lower, upper,
                          group["amsbound"], zero)

    def _torch_update(self, group, p, g, state, consts):
        omb1, beta2, omb2, step_size, lower, upper = consts
        if group["weight_decay"] != 0:
            g = g.add(p, alpha=group["weight_decay"])
        m, v = state["exp_avg"], state["exp_avg_sq"]
        m.lerp_(g, omb1)
        v.mul_(beta2).addcmul_(g, g, value=omb2)
        if group["amsbound"]:
            v = torch.maximum(state["max_exp_avg_sq"], v, out=state["max_exp_avg_sq"])
        rate = v.sqrt().add_(group["eps"])
        rate = torch.div(rate.new_full((), step_size), rate, out=rate).clamp_(lower, upper)
        p.sub_(rate.mul_(m))


class HipRAdam(RestatedRuleMixin, torch.optim.Optimizer):
    """RAdam (Liu et al., ICLR 2020) as the reference's ``optimizers.RAdam`` states it (optimizers.py:141-211), restated: the same
    constructor signature, defaults, ``param_groups`` keys and state keys (``step`` -- a Python int --, ``exp_avg``, ``exp_avg_sq``), so
    a state dict moves between the two classes in both directions. It is NOT torch.optim.RAdam, which differs in both thresholds and
    in the weight decay: here the gradient takes no weight decay (the parameter shrinks by weight_decay lr before the update), the
    step size is rectified when N > 5 and the adaptive form runs when N > 4 (radam_constants).

    One deliberate difference from the reference: the step constants are computed per group. The reference caches them under
    ``step % 10`` across all groups, so a second group with another lr at the same count silently gets the first group's step size;
    here every group gets the step size of its own lr.

    On CUDA parameters the step is one agrl_radam_step launch per (group, device, step count); ``zero_grads`` as for HipAdam."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, *, zero_grads=False):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._init_routes(zero_grads)

    def _state_names(self, group):
        return ("exp_avg", "exp_avg_sq", None)

    def _fill_state(self, state, p, group):
        if len(state) == 0:
            state["step"] = 0
            state["exp_avg"] = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.preserve_format)
            state["exp_avg_sq"] = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.preserve_format)

    def _constants(self, group, gi, t):
        beta1, beta2 = (float(b) for b in group["betas"])
        return radam_constants(float(group["lr"]), beta1, beta2, t, float(group["weight_decay"]))

    def _launch(self, ops, group, key, tensors, chunks, zero):
        omb1, beta2, omb2, decay, step_size, adaptive = self._constants(group, key[0], key[2])
        ops.radam_step(tensors, chunks, omb1, beta2, omb2, decay, step_size, float(group["eps"]), adaptive, zero)

    def _torch_update(self, group, p, g, state, consts):
        omb1, beta2, omb2, decay, step_size, adaptive = consts
        g, w = g.float(), p.float()                      # fp32 arithmetic and state whatever the parameter's type (no copy for fp32)
        m, v = state["exp_avg"], state["exp_avg_sq"]
        v.mul_(beta2).addcmul_(g, g, value=omb2)
        m.lerp_(g, omb1)
        if decay != 0:
            w.add_(w, alpha=-decay)
        if adaptive:
            w.addcdiv_(m, v.sqrt().add_(group["eps"]), value=-step_size)
        else:
            w.add_(m, alpha=-step_size)
        if w is not p:
            p.copy_(w)


def init_optim_native(optim, params, lr, weight_decay):
    """The reference's ``optimizers.init_optim`` (optimizers.py:7-23) for all seven names, every one a native class with the reference's
    hyper-parameters; the driver's one-line change is ``from torchreid.hip_optim import init_optim_native as init_optim``."""
    if optim == 'rmsprop':
        return HipRMSprop(params, lr=lr, momentum=0.9, weight_decay=weight_decay)
    elif optim == 'adabound':
        return HipAdaBound(params, lr=lr, final_lr=100 * lr, weight_decay=weight_decay)
    elif optim == 'radam':
        return HipRAdam(params, lr=lr, weight_decay=weight_decay)
    return init_optim(optim, params, lr, weight_decay)


def init_optim(optim, params, lr, weight_decay):
    """The reference's ``optimizers.init_optim`` (optimizers.py:7-23) for the optimisers it builds from torch, as the native classes
    with the same hyper-parameters; the driver's one-line change is ``from torchreid.hip_optim import init_optim``. The other three
    names are built by ``init_optim_native``, which accepts all seven."""
    if optim == 'adam':
        return HipAdam(params, lr=lr, weight_decay=weight_decay)
    elif optim == 'amsgrad':
        return HipAdam(params, lr=lr, weight_decay=weight_decay, amsgrad=True)
    elif optim == 'sgd':
        return HipSGD(params, lr=lr, momentum=0.9, weight_decay=weight_decay)
    elif optim == 'nesterov':
        return HipSGD(params, lr=lr, momentum=0.9, weight_decay=weight_decay, nesterov=True)
    elif optim in ('rmsprop', 'adabound', 'radam'):
        raise NotImplementedError("optimizer %r is not built by init_optim: hip_optim.init_optim_native builds its native class, the "
                                  "reference's torchreid.optimizers.init_optim the stock one" % optim)
    else:
        raise KeyError("Unsupported optimizer: {}".format(optim))
