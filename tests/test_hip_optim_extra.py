"""HipRMSprop, HipAdaBound and HipRAdam without a GPU: the restated rules (tests/optim_ref.py) against the reference's own recorded
trajectory (tests/golden/optim_extra.npz, written by tests/golden/make_optim_golden.py), the CPU route, state dicts in both
directions, the factory, RAdam's per-group constants and the host bookkeeping of the native route."""
import copy
import os

import numpy as np
import pytest
import torch

import optim_ref as R
from torchreid import hip_optim
from torchreid.hip_optim import HipAdaBound, HipAdam, HipRAdam, HipRMSprop, HipSGD, init_optim_native

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim_extra.npz"))
SIZES = [int(n) for n in GOLDEN["sizes"]]
VARIANTS = ["adabound", "amsbound", "radam", "rmsprop"]
STATE = {"adabound": [("m", "exp_avg"), ("v", "exp_avg_sq")], "amsbound": [("m", "exp_avg"), ("v", "exp_avg_sq"), ("vmax", "max_exp_avg_sq")],
         "radam": [("m", "exp_avg"), ("v", "exp_avg_sq")], "rmsprop": [("sq", "square_avg"), ("buf", "momentum_buffer")]}
TABLE = {"adabound": R.N_ADABOUND, "amsbound": R.N_ADABOUND, "radam": R.N_RADAM, "rmsprop": R.N_RMSPROP}


def arr(variant, key):
    return torch.from_numpy(GOLDEN["%s/%s" % (variant, key)])


def hyper(variant):
    """The fixture's group as a dict (betas re-paired)."""
    keys, values = [str(k) for k in GOLDEN[variant + "/group_keys"]], [float(v) for v in GOLDEN[variant + "/hyper"]]
    out = {}
    for k in keys:
        out[k] = (values.pop(0), values.pop(0)) if k == "betas" else values.pop(0)
    assert not values
    return out


def exact_step(variant, h, p, g, state, t):
    """One exact step of the variant's rule from float64 p, g and state {short name: tensor}; the hyper-parameters are the fixture's."""
    if variant == "rmsprop":
        return R.rmsprop_exact(p, g, state["sq"], state["buf"], h["lr"], h["alpha"], h["eps"], h["weight_decay"], h["momentum"])
    if variant == "radam":
        return R.radam_exact(p, g, state["m"], state["v"], h["lr"], h["betas"], h["eps"], h["weight_decay"], t)
    ams = variant == "amsbound"
    return R.adabound_exact(p, g, state["m"], state["v"], state["vmax"] if ams else state["v"], h["lr"], h["betas"], h["eps"], h["weight_decay"], t,
                            h["final_lr"], h["gamma"], h["lr"], ams)


def hold(name, got, exact, table):
    worst = {k: R.worst_ratio(got[k], ex, mag, table[k]) for k, (ex, mag) in exact.items()}
    print("%s: worst |got - exact| / bound %s" % (name, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    assert all(w <= 1.0 for w in worst.values()), (name, worst)
    return worst


def make(variant, params, **extra):
    h = hyper(variant)
    if variant == "rmsprop":
        return HipRMSprop(params, lr=h["lr"], alpha=h["alpha"], eps=h["eps"], weight_decay=h["weight_decay"], momentum=h["momentum"], **extra)
    if variant == "radam":
        return HipRAdam(params, lr=h["lr"], betas=h["betas"], eps=h["eps"], weight_decay=h["weight_decay"], **extra)
    return HipAdaBound(params, lr=h["lr"], betas=h["betas"], final_lr=h["final_lr"], gamma=h["gamma"], eps=h["eps"],
                       weight_decay=h["weight_decay"], amsbound=variant == "amsbound", **extra)


def split(flat):
    return [t.clone() for t in torch.split(flat, SIZES)]


def state_cat(opt, params, variant):
    return {short: torch.cat([opt.state[p][key] for p in params]) for short, key in STATE[variant]}


# ---- the restatement IS the reference's rule --------------------------------------------------------------------------------------
def test_the_fixture_is_what_the_generator_describes():
    assert SIZES == [5, 64, 130] and [str(v) for v in GOLDEN["variants"]] == VARIANTS
    for variant in VARIANTS:
        h = hyper(variant)
        assert h["lr"] == 3e-4 and h["weight_decay"] == 5e-4
        assert arr(variant, "g").shape == arr(variant, "p").shape == (8, 199) and arr(variant, "p0").shape == (199,)
        g, p0 = arr(variant, "g"), arr(variant, "p0")
        assert bool((g == 0).any()) and bool((p0 == 0).any())
        nz = g[g != 0].abs()
        assert float(nz.max() / nz.min()) > 1e6                       # several decades
        assert GOLDEN[variant + "/step"].tolist() == [[float(t)] * 3 for t in range(1, 9)]
    assert hyper("rmsprop")["momentum"] == 0.9 and hyper("adabound")["final_lr"] == 100 * 3e-4 and hyper("amsbound")["amsbound"] == 1.0


@pytest.mark.parametrize("variant", VARIANTS)
def test_the_references_trajectory_holds_under_the_restated_rule(variant):
    """Each recorded step, from the reference's own previous fp32 state, lies within the bound of the exact evaluation."""
    h = hyper(variant)
    zeros = torch.zeros(199, dtype=torch.float64)
    p, state = arr(variant, "p0").double(), {short: zeros for short, _ in STATE[variant]}
    for t in range(1, 9):
        exact = exact_step(variant, h, p, arr(variant, "g")[t - 1].double(), state, t)
        got = dict({short: arr(variant, key)[t - 1] for short, key in STATE[variant]}, p=arr(variant, "p")[t - 1])
        hold("reference %s step %d" % (variant, t), got, exact, TABLE[variant])
        p, state = got["p"].double(), {short: got[short].double() for short, _ in STATE[variant]}
    if variant == "radam":
        assert [R.radam_regime(h["lr"], h["betas"], t) for t in range(1, 9)] == ["momentum"] * 4 + ["unrectified"] + ["rectified"] * 3


# ---- the CPU route ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["adabound", "amsbound", "radam"])
def test_cpu_route_holds_the_contract_on_the_fixtures_inputs(variant):
    h = hyper(variant)
    params = [torch.nn.Parameter(t) for t in split(arr(variant, "p0"))]
    opt = make(variant, params)
    zeros = torch.zeros(199, dtype=torch.float64)
    for t in range(1, 9):
        for p, g in zip(params, split(arr(variant, "g")[t - 1])):
            p.grad = g
        state = {k: v.double() for k, v in state_cat(opt, params, variant).items()} if t > 1 else {short: zeros for short, _ in STATE[variant]}
        exact = exact_step(variant, h, torch.cat([p.detach() for p in params]).double(), arr(variant, "g")[t - 1].double(), state, t)
        opt.step()
        got = dict(state_cat(opt, params, variant), p=torch.cat([p.detach() for p in params]))
        hold("cpu route %s step %d" % (variant, t), got, exact, TABLE[variant])
        assert all(opt.state[p]["step"] == t and type(opt.state[p]["step"]) is int for p in params)


def test_rmsprop_on_cpu_is_the_stock_step_bit_for_bit():
    h = hyper("rmsprop")
    a = [torch.nn.Parameter(t) for t in split(arr("rmsprop", "p0"))]
    b = [torch.nn.Parameter(t) for t in split(arr("rmsprop", "p0"))]
    native = make("rmsprop", a)
    stock = torch.optim.RMSprop(b, lr=h["lr"], alpha=h["alpha"], eps=h["eps"], weight_decay=h["weight_decay"], momentum=h["momentum"])
    assert isinstance(native, torch.optim.RMSprop)
    for t in range(1, 9):
        for params in (a, b):
            for p, g in zip(params, split(arr("rmsprop", "g")[t - 1])):
                p.grad = g
        if t == 3:
            a[1].grad = b[1].grad = None                      # skipped by both
        native.step()
        stock.step()
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        if t < 3:                                             # (and the fixture was recorded by that very class)
            assert torch.equal(torch.cat([p.detach() for p in a]), arr("rmsprop", "p")[t - 1])
    sa, sb = native.state_dict(), stock.state_dict()
    assert sa["param_groups"][0].keys() == sb["param_groups"][0].keys()
    for k in sb["state"]:
        assert sa["state"][k].keys() == sb["state"][k].keys()
        assert all(torch.equal(sa["state"][k][n], sb["state"][k][n]) for n in sb["state"][k])


def test_zero_grads_closure_and_hooks_on_the_cpu_route():
    for variant in VARIANTS:
        params = [torch.nn.Parameter(t) for t in split(arr(variant, "p0"))]
        opt = make(variant, params, zero_grads=True)
        seen = []
        opt.register_step_post_hook(lambda o, args, kwargs: seen.append(1))
        for p, g in zip(params, split(arr(variant, "g")[0])):
            p.grad = g
        params[2].grad = None
        kept = [p.grad for p in params]
        opt.step()
        assert params[2].grad is None and all(p.grad is k and not p.grad.any() for p, k in zip(params[:2], kept[:2]))
        for p, g in zip(params, split(arr(variant, "g")[1])):
            p.grad = g
        opt.step(zero_grads=False)
        assert all(p.grad.any() for p in params) and seen == [1, 1]
        calls = []

        def closure():
            calls.append(1)
            return sum((p ** 2).sum() for p in params)
        assert opt.step(closure).requires_grad and len(calls) == 1


# ---- state dicts --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_state_dict_keys_and_step_types_equal_the_references(variant):
    params = [torch.nn.Parameter(t) for t in split(arr(variant, "p0"))]
    opt = make(variant, params)
    for p, g in zip(params, split(arr(variant, "g")[0])):
        p.grad = g
    opt.step()
    sd = opt.state_dict()
    assert sorted(sd["state"][0].keys()) == [str(k) for k in GOLDEN[variant + "/state_keys"]]
    assert [k for k in sd["param_groups"][0] if k != "params"] == [str(k) for k in GOLDEN[variant + "/group_keys"]] or variant == "rmsprop"
    if variant == "rmsprop":                                  # torch's own class: whatever keys this torch gives it
        assert sd["param_groups"][0].keys() == torch.optim.RMSprop([torch.nn.Parameter(torch.ones(1))]).state_dict()["param_groups"][0].keys()
    step = sd["state"][0]["step"]
    kind = "tensor:%s" % str(step.dtype).replace("torch.", "") if torch.is_tensor(step) else type(step).__name__
    assert kind == str(GOLDEN[variant + "/step_type"])
    if variant in ("adabound", "amsbound"):
        assert opt.base_lrs == [3e-4] and "base_lrs" not in sd


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_state_dict_built_from_the_fixture_loads_and_continues_the_trajectory(variant):
    """The reference's state after its fifth step, as the reference's state_dict() lays it out, loaded into the native class: steps six
    to eight stay within the bound of the exact continuation (and RMSprop, torch's own class, lands on the recorded bits)."""
    h = hyper(variant)
    keys, k0 = [str(k) for k in GOLDEN[variant + "/group_keys"]], 5
    params = [torch.nn.Parameter(t) for t in split(arr(variant, "p")[k0 - 1])]
    opt = make(variant, params)
    group = dict(opt.state_dict()["param_groups"][0])
    assert variant == "rmsprop" or [k for k in group if k != "params"] == keys
    state = {}
    for i in range(3):
        state[i] = {key: split(arr(variant, key)[k0 - 1])[i] for _, key in STATE[variant]}
        state[i]["step"] = torch.tensor(float(k0)) if variant == "rmsprop" else k0
    opt.load_state_dict({"state": state, "param_groups": [group]})
    for t in range(k0 + 1, 9):
        for p, g in zip(params, split(arr(variant, "g")[t - 1])):
            p.grad = g
        st = {k: v.double() for k, v in state_cat(opt, params, variant).items()}
        exact = exact_step(variant, h, torch.cat([p.detach() for p in params]).double(), arr(variant, "g")[t - 1].double(), st, t)
        opt.step()
        got = dict(state_cat(opt, params, variant), p=torch.cat([p.detach() for p in params]))
        hold("continued %s step %d" % (variant, t), got, exact, TABLE[variant])
        assert all(float(opt.state[p]["step"]) == t for p in params)
    end, ref_end = torch.cat([p.detach() for p in params]), arr(variant, "p")[7]
    if variant == "rmsprop":
        assert torch.equal(end, ref_end)
    else:                                                     # three steps of two roundings-apart routes: a loose sanity figure, the bound is above
        assert float((end - ref_end).abs().max()) <= 1e-5 * float(ref_end.abs().max())


# ---- the factory, the groups ----------------------------------------------------------------------------------------------------------
def _params(n=3, size=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(size, generator=g)) for _ in range(n)]


def test_init_optim_native_names_hyperparameters_and_errors():
    want = {"adam": HipAdam, "amsgrad": HipAdam, "sgd": HipSGD, "nesterov": HipSGD, "rmsprop": HipRMSprop, "adabound": HipAdaBound, "radam": HipRAdam}
    for name, cls in want.items():
        opt = init_optim_native(name, _params(), 3e-4, 5e-4)
        group = opt.param_groups[0]
        assert type(opt) is cls and group["lr"] == 3e-4 and group["weight_decay"] == 5e-4 and opt.zero_grads is False
    group = init_optim_native("rmsprop", _params(), 3e-4, 5e-4).param_groups[0]
    assert group["momentum"] == 0.9 and group["alpha"] == 0.99 and group["eps"] == 1e-8 and group["centered"] is False
    opt = init_optim_native("adabound", _params(), 3e-4, 5e-4)
    group = opt.param_groups[0]
    assert group["final_lr"] == 100 * 3e-4 and group["gamma"] == 1e-3 and group["betas"] == (0.9, 0.999) and group["eps"] == 1e-8
    assert group["amsbound"] is False and opt.base_lrs == [3e-4] and opt.hip_native is True
    group = init_optim_native("radam", _params(), 3e-4, 5e-4).param_groups[0]
    assert group["betas"] == (0.9, 0.999) and group["eps"] == 1e-8
    assert init_optim_native("amsgrad", _params(), 3e-4, 5e-4).param_groups[0]["amsgrad"] is True
    assert init_optim_native("nesterov", _params(), 3e-4, 5e-4).param_groups[0]["nesterov"] is True
    with pytest.raises(KeyError, match="Unsupported optimizer"):
        init_optim_native("lion", _params(), 3e-4, 5e-4)
    for name in ("rmsprop", "adabound", "radam"):               # the older factory still refuses, and now says where to go
        with pytest.raises(NotImplementedError, match="init_optim_native"):
            hip_optim.init_optim(name, _params(), 3e-4, 5e-4)
    with pytest.raises(ValueError, match="Invalid gamma"):
        HipAdaBound(_params(), gamma=1.0)


def test_radam_constants_are_per_group():
    """Two groups with different lr at the same count: each moves by its own step size (the reference's step % 10 cache hands the
    second group the first one's)."""
    a, b = _params(1, 16, 1), _params(1, 16, 1)
    opt = HipRAdam([{"params": a, "lr": 1e-3}, {"params": b, "lr": 1e-1}])
    start = a[0].detach().clone()
    for it in range(7):                                       # through all three regimes
        g = torch.randn(16, generator=torch.Generator().manual_seed(50 + it))
        a[0].grad, b[0].grad = g.clone(), g.clone()
        opt.step()
    for t in range(1, 8):
        s1, s2 = (hip_optim.radam_constants(lr, 0.9, 0.999, t, 0.0)[4] for lr in (1e-3, 1e-1))
        assert abs(s2 / s1 / 100.0 - 1.0) < 1e-12
    da, db = (a[0].detach() - start).double(), (b[0].detach() - start).double()
    assert float((db - 100.0 * da).abs().max()) <= 1e-4 * float(db.abs().max()) and float(db.abs().min()) > 0
    c = hip_optim.radam_constants(3e-4, 0.9, 0.999, 5, 5e-4)
    assert c[3] == 5e-4 * 3e-4 and c[4] == 3e-4 / (1.0 - 0.9 ** 5) and c[5] is True
    assert hip_optim.radam_constants(3e-4, 0.9, 0.999, 4, 0.0)[5] is False
    lo = hip_optim.adabound_constants(3e-4, 0.9, 0.999, 2, 3e-2, 1e-3, 3e-4)
    assert lo[3] == 3e-4 * np.sqrt(1.0 - 0.999 ** 2) / (1.0 - 0.9 ** 2) and lo[4] == 3e-2 * (1.0 - 1.0 / (1e-3 * 2 + 1.0)) and lo[5] == 3e-2 * (1.0 + 1.0 / (1e-3 * 2))
    half = hip_optim.adabound_constants(1.5e-4, 0.9, 0.999, 2, 3e-2, 1e-3, 3e-4)       # a scheduler halved lr: the bounds follow
    assert abs(half[4] / lo[4] - 0.5) < 1e-12 and abs(half[5] / lo[5] - 0.5) < 1e-12


@pytest.mark.parametrize("variant", ["adabound", "radam", "rmsprop"])
def test_native_route_groups_launches_by_step_count(variant, monkeypatch):
    """The host bookkeeping of the native route without a device (the launch and the device tables are stubbed): AdaBound and RAdam
    take one launch per (group, step count), RMSprop one per group; parameters without a gradient do not advance; a count written
    from outside, a new gradient tensor and a reloaded state dict are picked up."""
    from torchreid import _hip
    from torchreid import hip_ops as ops
    launches = []
    monkeypatch.setattr(hip_optim.NativeStepMixin, "_all_cpu", lambda self: False)
    monkeypatch.setattr(hip_optim.NativeStepMixin, "_check_tensors", staticmethod(lambda p, g: None))
    monkeypatch.setattr(hip_optim.NativeStepMixin, "_tables_for", lambda self, device, rows: (len(rows), None))
    monkeypatch.setattr(_hip, "lib", lambda: None)
    # (tensors, t): t from step_size = lr sqrt(1 - 0.999^t) / (1 - 0.9^t) (AdaBound), from the tabulated step sizes (RAdam)
    ab = {round(hip_optim.adabound_constants(1e-3, 0.9, 0.999, t, 0.1, 1e-3, 1e-3)[3], 12): t for t in range(1, 20)}
    ra = {round(hip_optim.radam_constants(1e-3, 0.9, 0.999, t, 0.0)[4], 12): t for t in range(1, 20)}
    monkeypatch.setattr(ops, "adabound_step", lambda n, chunks, wd, omb1, b2, omb2, step_size, eps, lower, upper, ams, zero:
                        launches.append((n, ab[round(step_size, 12)])))
    monkeypatch.setattr(ops, "radam_step", lambda n, chunks, omb1, b2, omb2, decay, step_size, eps, adaptive, zero:
                        launches.append((n, ra[round(step_size, 12)])))
    monkeypatch.setattr(ops, "rmsprop_step", lambda n, chunks, wd, alpha, oma, eps, momentum, lr, has_momentum, zero: launches.append((n, None)))
    ps = _params(5)
    for i, p in enumerate(ps):
        p.grad = torch.ones(8) * (i + 1)
    opt = {"adabound": HipAdaBound, "radam": HipRAdam, "rmsprop": lambda q, lr: HipRMSprop(q, lr=lr, momentum=0.9)}[variant](ps, lr=1e-3)
    by_count = variant != "rmsprop"

    def counts():
        return [float(opt.state[p]["step"]) if p in opt.state else None for p in ps]

    def step():
        del launches[:]
        opt.step()
        return sorted(launches) if by_count else [(sum(n for n, _ in launches), len(launches))]

    def want(*classes):
        return sorted(classes) if by_count else [(sum(n for n, _ in classes), 1)]
    assert step() == want((5, 1)) and step() == want((5, 2)) and counts() == [2.0] * 5
    ps[1].grad = ps[3].grad = None
    assert step() == want((3, 3)) and counts() == [3.0, 2.0, 3.0, 2.0, 3.0]
    if by_count:
        opt.state[ps[3]]["step"] = 9                         # written from outside while that parameter sits out
    else:
        opt.state[ps[3]]["step"].fill_(9.0)
    ps[0].grad = torch.ones(8)                               # a new gradient tensor: its record is rebuilt in the same step
    assert step() == want((3, 4)) and counts() == [4.0, 2.0, 4.0, 9.0, 4.0]
    ps[1].grad, ps[3].grad = torch.ones(8), torch.ones(8)
    assert step() == want((1, 3), (1, 10), (3, 5)) and counts() == [5.0, 3.0, 5.0, 10.0, 5.0]
    saved = copy.deepcopy(opt.state_dict())
    step()
    opt.load_state_dict(saved)                               # rewinds the counts
    assert step() == want((1, 4), (1, 11), (3, 6)) and counts() == [6.0, 4.0, 6.0, 11.0, 6.0]
    assert all(type(opt.state[p]["step"]) is int for p in ps) if by_count else all(torch.is_tensor(opt.state[p]["step"]) for p in ps)


def test_without_the_library_the_native_route_raises(monkeypatch):
    from torchreid import _hip

    def missing():
        raise _hip.HipLibraryError("no library")
    monkeypatch.setattr(hip_optim.NativeStepMixin, "_all_cpu", lambda self: False)
    monkeypatch.setattr(_hip, "lib", missing)
    for variant in VARIANTS:
        ps = _params()
        for p in ps:
            p.grad = torch.ones(8)
        with pytest.raises(_hip.HipLibraryError):
            make(variant, ps).step()
        opt = make(variant, ps)
        if variant != "rmsprop":                             # hip_native = False: the torch formulation, no library needed
            opt.hip_native = False
            opt.step()
            assert all(opt.state[p]["step"] == 1 for p in ps)
