"""torchreid.hip_optim without a GPU: the factory, the CPU route (the stock optimisers, bit for bit), state dicts in both directions,
the chunk / descriptor tables of the multi-tensor kernel, and the bucket re-arming of parallel.GradientBuckets."""
import copy

import numpy as np
import pytest
import torch

from torchreid import hip_optim
from torchreid.hip_optim import CHUNK, HipAdam, HipSGD, build_chunk_table, build_descriptors, init_optim

C = CHUNK
SIZES = [1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 3]


def _params(seed=0, shapes=((7, 5), (13,), (3, 2, 4))):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]


def _set_grads(params, seed):
    g = torch.Generator().manual_seed(seed)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g)


VARIANTS = {
    "adam": (HipAdam, torch.optim.Adam, dict(lr=1e-2, weight_decay=5e-4)),
    "amsgrad": (HipAdam, torch.optim.Adam, dict(lr=1e-2, weight_decay=5e-4, amsgrad=True)),
    "sgd": (HipSGD, torch.optim.SGD, dict(lr=0.1, momentum=0.9, weight_decay=5e-4)),
    "nesterov": (HipSGD, torch.optim.SGD, dict(lr=0.1, momentum=0.9, weight_decay=5e-4, nesterov=True)),
}


def test_init_optim_names_hyperparameters_and_errors():
    for name in ("adam", "amsgrad", "sgd", "nesterov"):
        opt = init_optim(name, _params(), 3e-4, 5e-4)
        group = opt.param_groups[0]
        assert group["lr"] == 3e-4 and group["weight_decay"] == 5e-4
        if name in ("adam", "amsgrad"):
            assert type(opt) is HipAdam and isinstance(opt, torch.optim.Adam)
            assert group["amsgrad"] == (name == "amsgrad") and group["betas"] == (0.9, 0.999) and group["eps"] == 1e-8
        else:
            assert type(opt) is HipSGD and isinstance(opt, torch.optim.SGD)
            assert group["momentum"] == 0.9 and group["dampening"] == 0 and group["nesterov"] == (name == "nesterov")
        assert opt.zero_grads is False
    for name in ("rmsprop", "adabound", "radam"):
        with pytest.raises(NotImplementedError, match="torchreid.optimizers"):
            init_optim(name, _params(), 3e-4, 5e-4)
    with pytest.raises(KeyError, match="Unsupported optimizer"):
        init_optim("lion", _params(), 3e-4, 5e-4)


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_cpu_parameters_take_the_stock_step_bit_for_bit(name):
    native_cls, stock_cls, kw = VARIANTS[name]
    a, b = _params(), _params()
    native, stock = native_cls(a, **kw), stock_cls(b, **kw)
    for it in range(3):
        _set_grads(a, 10 + it)
        _set_grads(b, 10 + it)
        if it == 1:
            a[1].grad = b[1].grad = None          # skipped by both
        native.step()
        stock.step()
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    sa, sb = native.state_dict(), stock.state_dict()
    assert sa["param_groups"][0].keys() == sb["param_groups"][0].keys()
    for k in sb["state"]:
        assert sa["state"][k].keys() == sb["state"][k].keys()
        for name_ in sb["state"][k]:
            assert torch.equal(torch.as_tensor(sa["state"][k][name_]), torch.as_tensor(sb["state"][k][name_])), (k, name_)


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_state_dict_round_trip_with_the_stock_optimiser(name):
    native_cls, stock_cls, kw = VARIANTS[name]
    for first, second in ((native_cls, stock_cls), (stock_cls, native_cls)):
        a, b = _params(), _params()
        one, ref = first(a, **kw), first(b, **kw)
        for it in range(2):
            for params, opt in ((a, one), (b, ref)):
                _set_grads(params, 20 + it)
                opt.step()
        c = [torch.nn.Parameter(p.detach().clone()) for p in a]
        other = second(c, **kw)
        other.load_state_dict(copy.deepcopy(one.state_dict()))
        for it in range(2):
            for params, opt in ((c, other), (b, ref)):
                _set_grads(params, 30 + it)
                opt.step()
        for x, y in zip(c, b):
            assert torch.equal(x, y)


def test_zero_grads_and_closure_on_the_cpu_route():
    a = _params()
    opt = HipAdam(a, lr=1e-2, zero_grads=True)
    _set_grads(a, 1)
    a[2].grad = None
    kept = [None if p.grad is None else p.grad for p in a]
    opt.step()
    assert a[2].grad is None and all(p.grad is k and not p.grad.any() for p, k in zip(a[:2], kept[:2]))
    _set_grads(a, 2)
    opt.step(zero_grads=False)
    assert all(p.grad.any() for p in a)
    calls = []

    def closure():
        calls.append(1)
        loss = sum((p ** 2).sum() for p in a)
        for p in a:
            p.grad = None
        loss.backward()
        return loss
    loss = HipSGD(a, lr=0.1, momentum=0.9).step(closure)
    assert len(calls) == 1 and loss.requires_grad


def test_step_hooks_fire_once_on_the_cpu_route():
    torch.optim.Adam(_params(), lr=1e-3)       # instantiating the stock class wraps ITS step with the hook runner too
    a = _params()
    opt = HipAdam(a, lr=1e-3)
    seen = []
    opt.register_step_post_hook(lambda o, args, kwargs: seen.append(1))
    _set_grads(a, 3)
    opt.step()
    assert seen == [1]


def _coverage(table, numels, chunk):
    cover = [np.zeros(n, dtype=np.int32) for n in numels]
    for t, c in table.tolist():
        lo = c * chunk
        assert lo < numels[t]
        cover[t][lo:min(numels[t], lo + chunk)] += 1
    return cover


@pytest.mark.parametrize("numels", [SIZES, None], ids=["edge_sizes", "300_small"])
def test_chunk_table_covers_every_element_exactly_once(numels):
    if numels is None:
        numels = [int(v) for v in np.random.RandomState(0).randint(1, 8, size=300)]
        assert min(numels) == 1 and max(numels) == 7
    table = build_chunk_table(numels)
    assert table.dtype == np.int32 and table.shape == (sum(-(-n // C) for n in numels), 2)
    for cover in _coverage(table, numels, C):
        assert (cover == 1).all()
    assert (np.diff(table[:, 0]) >= 0).all()      # tensors in order, a tensor's chunks in order
    small = build_chunk_table([5, 1, 9], chunk=4)
    assert small.tolist() == [[0, 0], [0, 1], [1, 0], [2, 0], [2, 1], [2, 2]]
    with pytest.raises(ValueError):
        build_chunk_table([3, 0])
    with pytest.raises(ValueError):
        build_chunk_table([])


def test_descriptors_carry_pointers_counts_and_the_alignment_word():
    rows = [(1024, 2048, 4096, 8192, 0, 17), (1024, 2052, 4096, 8192, 0, 4), (1028, 2052, 4100, 8196, 16388, 4096), (1024, 2048, 0, 0, 0, 3)]
    desc = build_descriptors(rows)
    assert desc.dtype == np.int64 and desc.shape == (4, hip_optim.WORDS)
    assert [tuple(r[:6]) for r in desc.tolist()] == rows
    assert desc[:, 6].tolist() == [1, 0, 0, 1] and not desc[:, 7].any()


def test_adam_constants_are_formed_in_double():
    omb1, b2, omb2, step_size, inv = hip_optim.adam_constants(1e-4, 0.9, 0.999, 3)
    assert (omb1, b2, omb2) == (1.0 - 0.9, 0.999, 1.0 - 0.999)
    assert step_size == 1e-4 / (1.0 - 0.9 ** 3) and inv == 1.0 / np.sqrt(1.0 - 0.999 ** 3)
    # what the issue is about: the fp32 difference is 6e-5 off the double one
    assert abs(float(np.float32(1.0) - np.float32(0.999)) / omb2 - 1.0) > 1e-5 > abs(float(np.float32(omb2)) / omb2 - 1.0)


def test_buckets_skip_the_refill_once_after_mark_clean():
    from torchreid import parallel
    params = _params()
    buckets = parallel.GradientBuckets(params, bucket_bytes=64)
    assert len(buckets.buckets) > 1
    for flat, _ in buckets.buckets:
        flat.fill_(1.0)
    buckets._pending = [0] * len(buckets.buckets)
    buckets.mark_clean()              # (a lie here: shows that the fill is skipped and the counters re-armed)
    buckets.zero_grad()
    assert all(bool((flat == 1).all()) for flat, _ in buckets.buckets)
    assert buckets._pending == [len(group) for _, group in buckets.buckets]
    buckets.zero_grad()               # the word holds for one zero_grad only
    assert all(not flat.any() for flat, _ in buckets.buckets)
    buckets.remove()


def test_train_step_with_buckets_and_a_native_optimiser_leaves_the_buffers_zero():
    """parallel.train_step on CPU tensors (the stock arithmetic): with HipAdam the step zero-fills what it consumed, the buckets skip
    their refill, and two steps give bit for bit what torch.optim.Adam gives with the refill."""
    from recipe import recipe_state_dict, synthetic_adj, synthetic_clips
    from torchreid import losses, models, parallel
    results = []
    for native in (False, True):
        torch.manual_seed(0)
        m = models.init_model("vmgn", num_classes=5, loss={"xent", "htri"}, last_stride=1, num_split=4, num_gb=1, num_scale=1,
                              pyramid_part=True, use_pose=True, learn_graph=True, consistent_loss=False)
        m.load_state_dict(recipe_state_dict(m.state_dict(), seed=1))
        pids = torch.tensor([0, 0, 1, 1])
        x, adj = synthetic_clips(4, 2, H=64, W=32, seed=3, identities=pids.tolist()), synthetic_adj(4, 2, seed=3)
        opt = (HipAdam if native else torch.optim.Adam)(m.parameters(), lr=1e-3, weight_decay=5e-2)
        buckets = parallel.GradientBuckets(m.parameters(), bucket_bytes=8 << 20)
        for htri_only in (False, True):
            parallel.train_step(m, x, adj, pids, losses.CrossEntropyLabelSmooth(5, use_gpu=False), losses.TripletLoss(margin=0.3, soft=True),
                                opt, htri_only=htri_only, buckets=buckets)
            if native:
                assert buckets._clean and all(not flat.any() for flat, _ in buckets.buckets)
            else:
                assert not buckets._clean and any(bool(flat.any()) for flat, _ in buckets.buckets)
            assert all(p.grad is not None for p in m.parameters() if p.requires_grad)
        buckets.remove()
        results.append({k: v.clone() for k, v in m.state_dict().items()})
    for k in results[0]:
        assert torch.equal(results[0][k], results[1][k]), k


def test_native_route_groups_launches_by_step_count(monkeypatch):
    """The host bookkeeping of the native route without a device (the launch and the device tables are stubbed): one launch per
    (group, step count); parameters without a gradient do not advance; a count written from outside, a new gradient tensor and a
    reloaded state dict are all picked up; the counts in state_dict() are what torch.optim.Adam reads."""
    from torchreid import _hip
    from torchreid import hip_ops as ops
    launches = []
    monkeypatch.setattr(hip_optim.NativeStepMixin, "_all_cpu", lambda self: False)
    monkeypatch.setattr(hip_optim.NativeStepMixin, "_check_tensors", staticmethod(lambda p, g: None))
    monkeypatch.setattr(hip_optim.NativeStepMixin, "_tables_for", lambda self, device, rows: (len(rows), None))
    monkeypatch.setattr(_hip, "lib", lambda: None)
    monkeypatch.setattr(ops, "adam_step", lambda n, chunks, wd, omb1, b2, omb2, step_size, inv, eps, ams, zero:
                        launches.append((n, round(np.log(1.0 - 1e-3 / step_size) / np.log(0.9)))))     # (tensors, t) from lr / (1 - 0.9^t)
    ps = _params(shapes=((8,),) * 5)
    _set_grads(ps, 1)
    opt = HipAdam(ps, lr=1e-3)

    def counts():
        return [float(opt.state[p]["step"]) if p in opt.state else None for p in ps]

    def step():
        del launches[:]
        opt.step()
        return sorted(launches)
    assert step() == [(5, 1)] and step() == [(5, 2)] and counts() == [2.0] * 5
    ps[1].grad = ps[3].grad = None
    assert step() == [(3, 3)] and counts() == [3.0, 2.0, 3.0, 2.0, 3.0]
    opt.state[ps[3]]["step"].fill_(9.0)                  # written from outside while that parameter sits out
    ps[0].grad = torch.ones(8)                           # a new gradient tensor: its record is rebuilt in the same step
    assert step() == [(3, 4)] and counts() == [4.0, 2.0, 4.0, 9.0, 4.0]
    ps[1].grad, ps[3].grad = torch.ones(8), torch.ones(8)
    assert step() == [(1, 3), (1, 10), (3, 5)] and counts() == [5.0, 3.0, 5.0, 10.0, 5.0]
    saved = copy.deepcopy(opt.state_dict())
    stock = torch.optim.Adam(_params(shapes=((8,),) * 5), lr=1e-3)
    stock.load_state_dict(copy.deepcopy(saved))
    assert [float(v["step"]) for v in stock.state_dict()["state"].values()] == [5.0, 3.0, 5.0, 10.0, 5.0]
    step()
    opt.load_state_dict(saved)                           # rewinds the counts
    assert step() == [(1, 4), (1, 11), (3, 6)] and counts() == [6.0, 4.0, 6.0, 11.0, 6.0]


@pytest.mark.parametrize("kind", ["adam", "amsgrad", "sgd", "nesterov", "rmsprop", "adabound", "radam"])
@pytest.mark.parametrize("zero", [False, True])
def test_native_route_bumps_the_versions_of_what_it_wrote(kind, zero, monkeypatch):
    """The kernels write through raw pointers; the step makes the writes visible to whatever is keyed on torch's version counters (the
    eval forward's pack cache, autograd's saved tensors): +1 on every stepped parameter and state tensor, on the gradients only when
    the step zero-filled them, nothing on a parameter that sat out. All seven names of init_optim_native, i.e. all five step
    implementations (HipAdam, HipSGD, and StatefulNativeMixin's for HipRMSprop, HipAdaBound, HipRAdam). Launch and device tables stubbed,
    as above."""
    from torchreid import _hip
    from torchreid import hip_ops as ops
    launched = []
    for name in ("rmsprop_step", "adabound_step", "radam_step"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name: launched.append(_n))
    monkeypatch.setattr(hip_optim.NativeStepMixin, "_all_cpu", lambda self: False)
    monkeypatch.setattr(hip_optim.NativeStepMixin, "_check_tensors", staticmethod(lambda p, g: None))
    monkeypatch.setattr(hip_optim.NativeStepMixin, "_tables_for", lambda self, device, rows: (len(rows), None))
    monkeypatch.setattr(_hip, "lib", lambda: None)
    monkeypatch.setattr(ops, "adam_step", lambda *a: launched.append("adam_step"))
    monkeypatch.setattr(ops, "sgd_step", lambda *a: launched.append("sgd_step"))
    ps = _params(shapes=((8,),) * 3)
    _set_grads(ps, 1)
    ps[2].grad = None
    opt = hip_optim.init_optim_native(kind, ps, 1e-3, 5e-4)
    opt.step(zero_grads=zero)                            # creates the state
    state = [t for p in ps[:2] for k, t in sorted(opt.state[p].items()) if k != "step"]
    per_param = {"adam": 2, "amsgrad": 3, "sgd": 1, "nesterov": 1, "rmsprop": 2, "adabound": 2, "radam": 2}[kind]
    assert len(state) == 2 * per_param and all(torch.is_tensor(t) for t in state) and ps[2] not in opt.state
    want = {"amsgrad": "adam", "nesterov": "sgd"}.get(kind, kind) + "_step"
    assert launched and set(launched) == {want}         # the native route ran, not a per-tensor torch rule
    for _ in range(2):
        before = [t._version for t in ps + state], [p.grad._version for p in ps[:2]]
        opt.step(zero_grads=zero)
        assert [t._version for t in ps + state] == [v + 1 for v in before[0][:2]] + [before[0][2]] + [v + 1 for v in before[0][3:]]
        assert [p.grad._version for p in ps[:2]] == [v + (1 if zero else 0) for v in before[1]]
