"""torchreid.hip_optim on the GPU, the other three rules: agrl_rmsprop_step / agrl_adabound_step / agrl_radam_step through HipRMSprop /
HipAdaBound / HipRAdam. The conventions are those of test_gpu_hip_optim.py (its slab, input generators and ``hold`` are imported): before
each step p, g and the state are copied to float64, the rule is evaluated exactly (tests/optim_ref.py, where the n tables are derived)
and every element must satisfy |got - exact| <= n 2^-24 mag + 2^-149; every tensor is a slice of a sentinel-filled slab, so a write
outside a tensor or a sentinel read as data shows."""
import copy

import numpy as np
import pytest
import torch

import optim_ref as R
from test_gpu_hip_optim import DEV, SIZES, Slab, bits, d64, hold, rand_g, rand_p, slab_params
from torchreid import _hip
from torchreid import hip_ops as ops
from torchreid.hip_optim import CHUNK, MAX_GRID, HipAdaBound, HipRAdam, HipRMSprop

pytestmark = pytest.mark.gpu
C = CHUNK
BETAS, EPS, GAMMA, ALPHA = (0.9, 0.999), 1e-8, 1e-3, 0.99
KINDS = ["rmsprop", "adabound", "amsbound", "radam"]
# kind -> [(short name, state key)] in the descriptor's slot order
STATE = {"rmsprop": [("sq", "square_avg"), ("buf", "momentum_buffer")], "rmsprop_plain": [("sq", "square_avg")],
         "adabound": [("m", "exp_avg"), ("v", "exp_avg_sq")], "amsbound": [("m", "exp_avg"), ("v", "exp_avg_sq"), ("vmax", "max_exp_avg_sq")],
         "radam": [("m", "exp_avg"), ("v", "exp_avg_sq")]}
TABLE = {"rmsprop": R.N_RMSPROP, "rmsprop_plain": R.N_RMSPROP, "adabound": R.N_ADABOUND, "amsbound": R.N_ADABOUND, "radam": R.N_RADAM}
ENTRY = {"rmsprop": "agrl_rmsprop_step", "rmsprop_plain": "agrl_rmsprop_step", "adabound": "agrl_adabound_step", "amsbound": "agrl_adabound_step",
         "radam": "agrl_radam_step"}
FILLS = {"m": lambda n, g_: torch.randn(n, generator=g_) * 0.1, "v": lambda n, g_: torch.rand(n, generator=g_) * 0.01,
         "vmax": lambda n, g_: torch.rand(n, generator=g_) * 0.02, "sq": lambda n, g_: torch.rand(n, generator=g_) * 0.01,
         "buf": lambda n, g_: torch.randn(n, generator=g_), "zero": lambda n, g_: torch.zeros(n)}
STREAMS = ("p", "g", "m", "v", "vmax", "sq", "buf")


def make(kind, params, lr, wd, **extra):
    if kind.startswith("rmsprop"):
        return HipRMSprop(params, lr=lr, alpha=ALPHA, eps=EPS, weight_decay=wd, momentum=0.9 if kind == "rmsprop" else 0.0, **extra)
    if kind == "radam":
        return HipRAdam(params, lr=lr, betas=BETAS, eps=EPS, weight_decay=wd, **extra)
    return HipAdaBound(params, lr=lr, betas=BETAS, final_lr=100 * lr, gamma=GAMMA, eps=EPS, weight_decay=wd, amsbound=kind == "amsbound", **extra)


def exact_step(kind, lr, wd, p, g, st, t):
    """st: {short name: float64 tensor}; t: the count of the step being taken."""
    if kind.startswith("rmsprop"):
        return R.rmsprop_exact(p, g, st["sq"], st.get("buf"), lr, ALPHA, EPS, wd, 0.9 if kind == "rmsprop" else 0.0)
    if kind == "radam":
        return R.radam_exact(p, g, st["m"], st["v"], lr, BETAS, EPS, wd, t)
    return R.adabound_exact(p, g, st["m"], st["v"], st.get("vmax", st["v"]), lr, BETAS, EPS, wd, t, 100 * lr, GAMMA, lr, kind == "amsbound")


def state_cat(opt, params, kind):
    return {short: torch.cat([opt.state[p][key].reshape(-1) for p in params]) for short, key in STATE[kind]}


def count_of(kind, t):
    return torch.tensor(float(t)) if kind.startswith("rmsprop") else t


class Guarded(object):
    """An optimiser of ``kind`` whose parameters, gradients and state tensors are all slices of sentinel slabs. offsets: stream -> byte
    offset of every slice of that stream; t0 == 0: the state starts at zero (as the class would create it), else it is random and every
    count is t0."""

    def __init__(self, kind, lr, wd, sizes, offsets, seed, t0=0, **extra):
        self.kind, self.lr, self.wd, self.gen = kind, lr, wd, torch.Generator().manual_seed(seed)
        self.names = ["p", "g"] + [short for short, _ in STATE[kind]]
        self.slabs = {}
        for s in self.names:
            fill = rand_p if s == "p" else rand_g if s == "g" else FILLS[s if t0 else "zero"]
            self.slabs[s] = Slab(sizes, [offsets[s]] * len(sizes)).fill(fill, self.gen)
        self.params = slab_params(self.slabs["p"])
        self.opt = make(kind, self.params, lr, wd, **extra)
        for i, p in enumerate(self.params):
            self.opt.state[p] = dict({key: self.slabs[short].views[i] for short, key in STATE[kind]}, step=count_of(kind, t0))
        self.t = t0

    def arm(self):
        self.slabs["g"].fill(rand_g, self.gen)
        for p, g in zip(self.params, self.slabs["g"].views):
            p.grad = g

    def step(self, name, **kw):
        """One armed step held to the contract -> (exact, launches)."""
        self.t += 1
        before = {s: d64(self.slabs[s].cat()) for s in self.names}
        exact = exact_step(self.kind, self.lr, self.wd, before["p"], before["g"], before, self.t)
        _hip.PROFILE = []
        try:
            self.opt.step(**kw)
        finally:
            launches, _hip.PROFILE = [r[0] for r in _hip.PROFILE], None
        got = {s: self.slabs[s].cat() for s in self.names if s != "g"}
        hold("%s step %d" % (name, self.t), got, exact, TABLE[self.kind])
        assert all(float(self.opt.state[p]["step"]) == self.t for p in self.params)
        return exact, launches

    def check_guards(self):
        torch.cuda.synchronize()
        for s in self.names:
            assert self.slabs[s].outside_intact(), s
            assert bool(torch.isfinite(self.slabs[s].cat()).all()), s

    def vec_words(self):
        return next(iter(self.opt._tables.values()))[2][:, 6].tolist()


def offsets_for(offset):
    return dict(zip(STREAMS, (0, 4, 8, 12, 4, 12, 8))) if offset == "mixed" else {s: offset for s in STREAMS}


# ---- the contract over eight steps ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, "mixed"])
@pytest.mark.parametrize("lr,wd", [(3e-4, 5e-4), (1e-2, 0.0)])
@pytest.mark.parametrize("kind", KINDS + ["rmsprop_plain"])
def test_the_elementwise_contract_holds_over_eight_steps(kind, lr, wd, offset):
    """Each step from the device's own previous state, over the edge sizes (20496 elements in eight tensors). RAdam: the eight steps
    visit all three regimes. AdaBound: every step has elements in each of the three clamp outcomes (a property of the input
    generators, established on the CPU with the reference's class: at least 50 elements per outcome and step; this seed on the CPU
    route: at least 56)."""
    run = Guarded(kind, lr, wd, SIZES, offsets_for(offset), seed=111)
    regimes, outcomes = [], []
    for t in range(1, 9):
        run.arm()
        exact, launches = run.step("%s lr %g wd %g offset %s" % (kind, lr, wd, offset))
        assert launches == [ENTRY[kind]]
        if kind == "radam":
            regimes.append(R.radam_regime(lr, BETAS, t))
        if kind in ("adabound", "amsbound"):
            outcomes.append(R.adabound_clamp_counts(exact["vmax" if kind == "amsbound" else "v"][0], lr, BETAS, EPS, t, 100 * lr, GAMMA, lr))
    run.check_guards()
    assert run.vec_words() == [1 if offset == 0 else 0] * len(SIZES) and len(run.opt._tables) == 1
    if kind == "radam":
        assert regimes == ["momentum"] * 4 + ["unrectified"] + ["rectified"] * 3
    if outcomes:
        print("%s lr %g wd %g: clamp outcomes (lower, inside, upper) per step %s" % (kind, lr, wd, outcomes))
        assert all(min(o) >= 1 for o in outcomes), outcomes


# ---- nothing outside the tensors is written ----------------------------------------------------------------------------------------
def guarded_step(kind, sizes, offset, t0=5):
    """One step from a random state at count t0 with zero_grads: one launch, the contract, the guards, +0.0 in every gradient."""
    run = Guarded(kind, 1e-3, 5e-4, sizes, offsets_for(offset), seed=303, t0=t0)
    run.arm()
    _, launches = run.step("guarded %s offset %s" % (kind, offset), zero_grads=True)
    assert launches == [ENTRY[kind]]                              # one launch for all the tensors
    run.check_guards()
    assert not run.slabs["g"].cat().view(torch.int32).any()
    assert run.vec_words() == [1 if offset == 0 else 0] * len(sizes)
    return run


@pytest.mark.parametrize("kind", KINDS + ["rmsprop_plain"])
@pytest.mark.parametrize("offset", [0, 4, 8, 12, "mixed"])
def test_edge_sizes_write_nothing_outside_the_tensors(kind, offset):
    guarded_step(kind, SIZES, offset)


@pytest.mark.parametrize("t0", [2, 4])
def test_radam_forms_on_a_running_state(t0):
    """The momentum-only form (count 3) and the unrectified adaptive form (count 5) from a non-zero state."""
    assert R.radam_regime(1e-3, BETAS, t0 + 1) == {2: "momentum", 4: "unrectified"}[t0]
    guarded_step("radam", SIZES, "mixed", t0=t0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("offset", [0, 4])
def test_300_small_tensors_in_one_call(kind, offset):
    sizes = [int(v) for v in np.random.RandomState(0).randint(1, 8, size=300)]
    guarded_step(kind, sizes, offset)


@pytest.mark.parametrize("kind,offset", [("amsbound", 0), ("radam", 12), ("rmsprop", 0)])
def test_one_tensor_longer_than_the_grid(kind, offset):
    """grid x chunk + 5 elements: every workgroup takes a second trip through the stride loop, the last chunk is ragged."""
    guarded_step(kind, [MAX_GRID * C + 5], offset)


# ---- skip semantics, zero_grads, run to run ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["adabound", "radam"])
def test_parameters_without_gradient_are_skipped_and_counts_split_the_launches(kind):
    gen = torch.Generator().manual_seed(404)
    sizes = [C + 9, 17, 2 * C, 5, 33]
    P, G = Slab(sizes, [0] * 5).fill(rand_p, gen), Slab(sizes, [0] * 5)
    params = slab_params(P)
    opt = make(kind, params, 1e-3, 5e-4)

    def arm(active):
        G.fill(rand_g, gen)
        for i, p in enumerate(params):
            p.grad = G.views[i] if i in active else None

    arm({0, 1, 2, 3})                                     # the fifth parameter has no gradient yet
    opt.step()
    assert params[4] not in opt.state and all(opt.state[params[i]]["step"] == 1 for i in range(4))
    for _ in range(4):
        arm({0, 2})
        frozen = {i: (bits(params[i]), bits(opt.state[params[i]]["exp_avg"]), bits(opt.state[params[i]]["exp_avg_sq"])) for i in (1, 3)}
        p4 = bits(params[4])
        opt.step()
        for i, (bp, bm, bv) in frozen.items():
            st = opt.state[params[i]]
            assert torch.equal(bits(params[i]), bp) and torch.equal(bits(st["exp_avg"]), bm) and torch.equal(bits(st["exp_avg_sq"]), bv)
            assert st["step"] == 1
        assert torch.equal(bits(params[4]), p4) and params[4] not in opt.state
    assert opt.state[params[0]]["step"] == opt.state[params[2]]["step"] == 5
    # the same active set again: the cached tables serve it -- no rebuild, no allocation
    del frozen, p4, bp, bm, bv
    arm({0, 2})
    tables, allocated = len(opt._tables), torch.cuda.memory_allocated()
    opt.step()
    assert len(opt._tables) == tables == 2 and torch.cuda.memory_allocated() == allocated
    # now everything has a gradient: step counts 7, 2, 7, 2, 1 -> three launch classes, each held to the contract with ITS count
    arm({0, 1, 2, 3, 4})
    zeros = lambda i: torch.zeros(sizes[i], dtype=torch.float64, device=DEV)
    before = {i: (d64(params[i]), d64(G.views[i])) + tuple(d64(opt.state[params[i]][k]) if params[i] in opt.state else zeros(i)
                                                            for k in ("exp_avg", "exp_avg_sq")) for i in range(5)}
    _hip.PROFILE = []
    try:
        opt.step()
    finally:
        launches, _hip.PROFILE = [r[0] for r in _hip.PROFILE], None
    assert launches == [ENTRY[kind]] * 3
    for i, t in enumerate([7, 2, 7, 2, 1]):
        p0, g0, m0, v0 = before[i]
        st = opt.state[params[i]]
        assert st["step"] == t and type(st["step"]) is int
        hold("%s mixed step counts, tensor %d (t = %d)" % (kind, i, t), {"p": params[i], "m": st["exp_avg"], "v": st["exp_avg_sq"]},
             exact_step(kind, 1e-3, 5e-4, p0, g0, {"m": m0, "v": v0}, t), TABLE[kind])
    assert P.outside_intact() and G.outside_intact()


@pytest.mark.parametrize("kind", KINDS)
def test_zero_grads_and_run_to_run(kind):
    """zero_grads=True: every consumed gradient is bitwise +0.0 afterwards; off: bitwise unchanged. Two runs from one state are bitwise
    equal in p and state, with the flag on or off."""
    sizes = [2 * C + 3, 7, C]
    runs = []
    for zero in (False, False, True):
        gen = torch.Generator().manual_seed(505)
        P, G = Slab(sizes, [0, 4, 0]).fill(rand_p, gen), Slab(sizes, [0, 4, 0])
        params = slab_params(P)
        opt = make(kind, params, 1e-3, 5e-4, zero_grads=zero)
        for _ in range(6):                                        # RAdam: past the change of form
            G.fill(rand_g, gen)
            G.views[1][0] = -0.0
            for p, g in zip(params, G.views):
                p.grad = g
            gbits = bits(G.cat())
            opt.step()
            if zero:
                assert not bits(G.cat()).any()
            else:
                assert torch.equal(bits(G.cat()), gbits)
            assert all(p.grad.data_ptr() == g.data_ptr() for p, g in zip(params, G.views))
        state = [bits(t) for p in params for _, t in sorted(opt.state[p].items()) if torch.is_tensor(t) and t.is_cuda]
        assert len(state) == len(STATE[kind]) * len(sizes)
        runs.append([bits(P.cat())] + state)
    for other in runs[1:]:
        assert len(other) == len(runs[0]) and all(torch.equal(a, b) for a, b in zip(runs[0], other))


# ---- state dicts on the device -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", ["native_to_torch", "torch_to_native"])
@pytest.mark.parametrize("kind", KINDS)
def test_state_dict_moves_between_the_native_and_the_torch_route(kind, direction):
    """AdaBound / RAdam: the same class with hip_native = False; RMSprop: torch.optim.RMSprop. Three steps on one route, the state dict
    into the other, and the fourth step of both lands within the bound of the exact continuation."""
    gen = torch.Generator().manual_seed(606)
    sizes = [C + 37, 129]
    lr, wd = 1e-3, 5e-4

    def build(params, native):
        if kind == "rmsprop" and not native:
            return torch.optim.RMSprop(params, lr=lr, alpha=ALPHA, eps=EPS, weight_decay=wd, momentum=0.9, foreach=False)
        opt = make(kind, params, lr, wd)
        if not native:
            opt.hip_native = False
        return opt
    a = [torch.nn.Parameter(rand_p(n, gen).to(DEV)) for n in sizes]
    first = build(a, direction == "native_to_torch")
    for _ in range(3):
        for p in a:
            p.grad = rand_g(p.numel(), gen).to(DEV)
        first.step()
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    second = build(b, direction != "native_to_torch")
    second.load_state_dict(copy.deepcopy(first.state_dict()))
    assert first.state_dict()["state"][0].keys() == second.state_dict()["state"][0].keys() == {"step"} | {key for _, key in STATE[kind]}
    grads = [rand_g(p.numel(), gen).to(DEV) for p in a]
    exact = exact_step(kind, lr, wd, d64(torch.cat(list(a))), d64(torch.cat(grads)), {k: d64(v) for k, v in state_cat(first, a, kind).items()}, 4)
    _hip.PROFILE = []
    try:
        for params, opt, name in ((a, first, "first"), (b, second, "second")):
            for p, g in zip(params, grads):
                p.grad = g.clone()
            opt.step()
            assert all(float(opt.state[p]["step"]) == 4 for p in params)
            hold("%s %s, %s optimiser" % (kind, direction, name), dict(state_cat(opt, params, kind), p=torch.cat(list(params))), exact, TABLE[kind])
    finally:
        launches, _hip.PROFILE = [r[0] for r in _hip.PROFILE], None
    assert launches == [ENTRY[kind]]                              # the native side: one launch; the torch side: none of the library's


# ---- host errors: raised before anything is launched ---------------------------------------------------------------------------------
def test_unsupported_inputs_raise_before_any_launch(monkeypatch):
    launched = []
    monkeypatch.setattr(ops, "call", lambda name, *args: launched.append(name))

    def param(t):
        p = torch.nn.Parameter(t)
        p.grad = torch.ones_like(t)
        return p
    good = param(torch.ones(8, device=DEV))
    cases = [
        (NotImplementedError, lambda: HipRMSprop([good], centered=True)),
        (NotImplementedError, lambda: HipRMSprop([good], maximize=True)),
        (NotImplementedError, lambda: HipRMSprop([good], capturable=True)),
        (NotImplementedError, lambda: HipRMSprop([good], differentiable=True)),
        (TypeError, lambda: HipRMSprop([good, param(torch.ones(8, device=DEV, dtype=torch.float64))])),
        (TypeError, lambda: HipAdaBound([good, param(torch.ones(8, device=DEV, dtype=torch.float16))])),
        (TypeError, lambda: HipRAdam([param(torch.ones(8, device=DEV, dtype=torch.bfloat16))])),
        (ValueError, lambda: HipAdaBound([good, param(torch.ones(4, 6, device=DEV).t())])),
        (ValueError, lambda: HipRAdam([param(torch.ones(4, 6, device=DEV)[:, ::2])])),
        (ValueError, lambda: HipRMSprop([good, param(torch.ones(8))])),            # CPU and CUDA parameters in one optimiser
    ]
    for exc, build in cases:
        opt = build()
        with pytest.raises(exc):
            opt.step()
    sparse = torch.nn.Parameter(torch.ones(8, device=DEV))
    sparse.grad = torch.sparse_coo_tensor(torch.tensor([[1, 3]]), torch.tensor([1.0, 2.0]), (8,)).to(DEV)
    for opt in (HipRMSprop([good, sparse]), HipAdaBound([good, sparse]), HipRAdam([sparse])):
        with pytest.raises(NotImplementedError, match="sparse"):
            opt.step()
    assert launched == [] and bool((good == 1).all())
    for cls, entry in ((HipRMSprop, "agrl_rmsprop_step"), (HipAdaBound, "agrl_adabound_step"), (HipRAdam, "agrl_radam_step")):
        del launched[:]
        cls([good]).step()
        assert launched == [entry]                                # (the stub sees the launch of a supported step)
