"""torchreid.hip_optim on the GPU: agrl_adam_step / agrl_sgd_step through HipAdam / HipSGD.

The arithmetic contract is elementwise. Before each step p, g and the state are copied to float64 and the update formulas of
csrc/optim.hip are evaluated exactly, with the same host constants (formed in double, each rounded once to fp32); ``mag`` is the same
chain on magnitudes:

    mag_gd = |g| + wd |p|      mag_m = |m| + (1 - b1)(mag_gd + |m|)      mag_v = b2 v + (1 - b2) mag_gd^2      mag_p = |p| + step_size mag_m / den
    SGD: mag_buf = mu |buf| + mag_gd,  mag_d = mag_gd + mu mag_buf (Nesterov) | mag_buf,  mag_p = |p| + lr mag_d

and every element must satisfy |got - exact| <= n 2^-24 mag + 2^-149 with n = the rounding count of the chain plus two (contracted
FMAs only remove roundings): Adam m 8, v / vmax 12, p 12; SGD buf 6, p 8. Stock torch (single-tensor fp32, CPU) on the same inputs
stays below 2.8 / 5.7 / 4.1 / 2.4 / 2.7 -- inside half of each bound."""
import copy

import numpy as np
import pytest
import torch

from bounds import U32, check_rounded, log_record
from torchreid import _hip
from torchreid import hip_ops as ops
from torchreid.hip_optim import CHUNK, MAX_GRID, HipAdam, HipSGD, adam_constants

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = CHUNK
SIZES = [1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 3]
SENTINEL = 0x7FC5A5A5                    # a NaN pattern: a sentinel read as data would also show in the finiteness check
N_ADAM = {"m": 8, "v": 12, "vmax": 12, "p": 12}
N_SGD = {"buf": 6, "p": 8}
TINY = 2.0 ** -149


def f32(x):
    return float(np.float32(x))


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def rand_p(n, gen):
    x = torch.randn(n, generator=gen) * 10.0 ** (torch.rand(n, generator=gen) * 4.0 - 3.0)
    x[torch.rand(n, generator=gen) < 0.02] = 0.0
    return x


def rand_g(n, gen):
    x = torch.randn(n, generator=gen) * 10.0 ** (torch.rand(n, generator=gen) * 10.0 - 8.0)
    x[torch.rand(n, generator=gen) < 0.05] = 0.0
    return x


class Slab(object):
    """Tensors of ``sizes`` as slices of ONE device buffer pre-filled with a sentinel; slice i starts ``offsets[i]`` bytes past a 16-byte
    boundary and has at least eight sentinel words on either side."""

    def __init__(self, sizes, offsets):
        pos, self.spans = 8, []
        for n, off in zip(sizes, offsets):
            assert off in (0, 4, 8, 12)
            start = pos + off // 4
            self.spans.append((start, n))
            pos = (start + n + 3) // 4 * 4 + 8
        self.buf = torch.empty(pos + 8, dtype=torch.float32, device=DEV)
        self.buf.view(torch.int32).fill_(SENTINEL)
        assert self.buf.data_ptr() % 16 == 0
        self.views = [self.buf[a:a + n] for a, n in self.spans]
        for v, (n, off) in zip(self.views, zip(sizes, offsets)):
            assert v.data_ptr() % 16 == off

    def fill(self, fn, gen):
        for v in self.views:
            v.copy_(fn(v.numel(), gen))
        return self

    def cat(self):
        return torch.cat(self.views)

    def outside_intact(self):
        mask = torch.ones(self.buf.numel(), dtype=torch.bool, device=DEV)
        for a, n in self.spans:
            mask[a:a + n] = False
        return bool((self.buf.view(torch.int32)[mask] == SENTINEL).all())


def slab_params(slab):
    return [torch.nn.Parameter(v) for v in slab.views]


# ---- the exact evaluation -------------------------------------------------------------------------------------------------------
def adam_exact(p, g, m, v, vmax, lr, betas, eps, wd, t, amsgrad):
    """float64 tensors in -> {name: (exact, mag)}."""
    omb1, b2, omb2, step_size, inv = (f32(c) for c in adam_constants(lr, betas[0], betas[1], t))
    wd, eps = f32(wd), f32(eps)
    gd = g + wd * p
    m2 = m + omb1 * (gd - m)
    v2 = b2 * v + omb2 * gd * gd
    vv = torch.maximum(vmax, v2) if amsgrad else v2
    den = vv.sqrt() * inv + eps
    p2 = p - step_size * m2 / den
    mag_gd = g.abs() + wd * p.abs()
    mag_m = m.abs() + omb1 * (mag_gd + m.abs())
    mag_v = b2 * v + omb2 * mag_gd * mag_gd
    out = {"p": (p2, p.abs() + step_size * mag_m / den), "m": (m2, mag_m), "v": (v2, mag_v)}
    if amsgrad:
        out["vmax"] = (vv, mag_v)
    return out


def sgd_exact(p, g, buf, lr, mu, wd, nesterov):
    """buf None: a tensor's first step. -> {name: (exact, mag)}."""
    lr, mu, wd = f32(lr), f32(mu), f32(wd)
    gd = g + wd * p
    mag_gd = g.abs() + wd * p.abs()
    b2 = gd if buf is None else mu * buf + gd
    mag_buf = mag_gd if buf is None else mu * buf.abs() + mag_gd
    d = gd + mu * b2 if nesterov else b2
    mag_d = mag_gd + mu * mag_buf if nesterov else mag_buf
    return {"p": (p - lr * d, p.abs() + lr * mag_d), "buf": (b2, mag_buf)}


def ratio_on_device(got, exact, mag, n):
    """max over the elements of |got - exact| / (n 2^-24 mag + 2^-149) as a device scalar (a non-finite output counts as inf)."""
    g = got.detach().double().reshape(-1)
    r = (g - exact.reshape(-1)).abs() / (n * U32 * mag.reshape(-1) + TINY)
    return torch.where(torch.isfinite(g), r, torch.full_like(r, float("inf"))).max()


def hold(name, got, exact, table):
    """Every element of every quantity inside its bound; the figures are printed before anything is asserted."""
    worst = {key: float(ratio_on_device(got[key], ex, mag, table[key])) for key, (ex, mag) in exact.items()}
    print("%s: worst |got - exact| / bound %s" % (name, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    log_record({"name": name, "ratio": worst})
    for key, (ex, mag) in exact.items():
        if not worst[key] <= 1.0:      # the element-by-element form names the offending element
            check_rounded(got[key].reshape(-1), ex.reshape(-1), mag.reshape(-1), table[key], torch.float32,
                          slack=torch.full(ex.reshape(-1).shape, TINY, dtype=torch.float64), name="%s %s" % (name, key))
            raise AssertionError("%s %s: worst ratio %.3f" % (name, key, worst[key]))
    return worst


def d64(t):
    return t.detach().double()


def adam_state_cat(opt, params, amsgrad):
    keys = [("m", "exp_avg"), ("v", "exp_avg_sq")] + ([("vmax", "max_exp_avg_sq")] if amsgrad else [])
    return {k: torch.cat([opt.state[p][name].reshape(-1) for p in params]) for k, name in keys}


# ---- the contract over six steps ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("amsgrad", [False, True], ids=["adam", "amsgrad"])
@pytest.mark.parametrize("lr,wd", [(1e-4, 5e-4), (1e-2, 0.0)])
def test_adam_meets_the_elementwise_contract_over_six_steps(lr, wd, amsgrad):
    n = 3 * C + 37
    gen = torch.Generator().manual_seed(101)
    offs = [0, 0, 4]                                    # the third tensor goes through the dword path
    P, G = Slab([n] * 3, offs).fill(rand_p, gen), Slab([n] * 3, offs)
    params = slab_params(P)
    opt = HipAdam(params, lr=lr, weight_decay=wd, amsgrad=amsgrad)
    zeros = torch.zeros(3 * n, dtype=torch.float64, device=DEV)
    for t in range(1, 7):
        G.fill(rand_g, gen)
        for p, g in zip(params, G.views):
            p.grad = g
        st = adam_state_cat(opt, params, amsgrad) if t > 1 else {}
        exact = adam_exact(d64(P.cat()), d64(G.cat()), d64(st["m"]) if st else zeros, d64(st["v"]) if st else zeros,
                           d64(st["vmax"]) if st and amsgrad else zeros, lr, (0.9, 0.999), 1e-8, wd, t, amsgrad)
        opt.step()
        got = dict(adam_state_cat(opt, params, amsgrad), p=P.cat())
        hold("adam lr %g wd %g amsgrad %d step %d" % (lr, wd, amsgrad, t), got, exact, N_ADAM)
        assert all(float(opt.state[p]["step"]) == t for p in params)
    assert P.outside_intact() and G.outside_intact()
    vec = next(iter(opt._tables.values()))[2][:, 6].tolist()
    assert vec == [1, 1, 0] and len(opt._tables) == 1      # the same pointers six times: one table, built once


@pytest.mark.parametrize("nesterov", [False, True], ids=["sgd", "nesterov"])
@pytest.mark.parametrize("lr,wd", [(0.1, 5e-4), (1e-4, 5e-4)])
def test_sgd_meets_the_elementwise_contract_over_six_steps(lr, wd, nesterov):
    n = 3 * C + 37
    gen = torch.Generator().manual_seed(202)
    offs = [0, 0, 4]
    P, G = Slab([n] * 3, offs).fill(rand_p, gen), Slab([n] * 3, offs)
    params = slab_params(P)
    opt = HipSGD(params, lr=lr, momentum=0.9, weight_decay=wd, nesterov=nesterov)
    for t in range(1, 7):
        G.fill(rand_g, gen)
        for p, g in zip(params, G.views):
            p.grad = g
        buf = d64(torch.cat([opt.state[p]["momentum_buffer"] for p in params])) if t > 1 else None
        exact = sgd_exact(d64(P.cat()), d64(G.cat()), buf, lr, 0.9, wd, nesterov)
        opt.step()
        got = {"p": P.cat(), "buf": torch.cat([opt.state[p]["momentum_buffer"] for p in params])}
        hold("sgd lr %g wd %g nesterov %d step %d" % (lr, wd, nesterov, t), got, exact, N_SGD)
    assert P.outside_intact() and G.outside_intact()


def test_sgd_without_momentum_keeps_no_state():
    gen = torch.Generator().manual_seed(7)
    P, G = Slab([C + 5, 3], [0, 8]).fill(rand_p, gen), Slab([C + 5, 3], [0, 8]).fill(rand_g, gen)
    params = slab_params(P)
    for p, g in zip(params, G.views):
        p.grad = g
    exact = sgd_exact(d64(P.cat()), d64(G.cat()), None, 0.05, 0.0, 5e-4, False)
    opt = HipSGD(params, lr=0.05, weight_decay=5e-4)
    opt.step()
    hold("sgd without momentum", {"p": P.cat()}, {"p": exact["p"]}, N_SGD)
    assert len(opt.state) == 0 and P.outside_intact() and G.outside_intact()


# ---- nothing outside the tensors is written ------------------------------------------------------------------------------------
def _guarded_step(kind, sizes, offsets):
    """One step with every parameter, gradient and state tensor inside a sentinel slab. offsets: stream -> byte offset of every slice."""
    gen = torch.Generator().manual_seed(303)
    adam = kind in ("adam", "amsgrad")
    streams = ["p", "g"] + (["m", "v"] + (["vmax"] if kind == "amsgrad" else []) if adam else (["buf"] if kind == "sgd" else []))
    fills = {"p": rand_p, "g": rand_g, "m": lambda n, g_: torch.randn(n, generator=g_) * 0.1, "v": lambda n, g_: torch.rand(n, generator=g_) * 0.01,
             "vmax": lambda n, g_: torch.rand(n, generator=g_) * 0.02, "buf": lambda n, g_: torch.randn(n, generator=g_)}
    slabs = {s: Slab(sizes, [offsets[s]] * len(sizes)).fill(fills[s], gen) for s in streams}
    params = slab_params(slabs["p"])
    for p, g in zip(params, slabs["g"].views):
        p.grad = g
    before = {s: d64(slabs[s].cat()) for s in streams}
    if adam:
        opt = HipAdam(params, lr=1e-3, weight_decay=5e-4, amsgrad=kind == "amsgrad")
        for i, p in enumerate(params):
            opt.state[p] = {"step": torch.tensor(2.0), "exp_avg": slabs["m"].views[i], "exp_avg_sq": slabs["v"].views[i]}
            if kind == "amsgrad":
                opt.state[p]["max_exp_avg_sq"] = slabs["vmax"].views[i]
        exact = adam_exact(before["p"], before["g"], before["m"], before["v"], before.get("vmax", before["v"]), 1e-3, (0.9, 0.999), 1e-8, 5e-4, 3,
                           kind == "amsgrad")
        table = N_ADAM
    else:
        opt = HipSGD(params, lr=0.1, momentum=0.9, weight_decay=5e-4, nesterov=kind == "nesterov_first")
        if kind == "sgd":
            for i, p in enumerate(params):
                opt.state[p] = {"momentum_buffer": slabs["buf"].views[i]}
        exact = sgd_exact(before["p"], before["g"], before.get("buf"), 0.1, 0.9, 5e-4, kind == "nesterov_first")
        table = N_SGD
    _hip.PROFILE = []
    try:
        opt.step(zero_grads=True)
    finally:
        launches, _hip.PROFILE = [r[0] for r in _hip.PROFILE], None
    torch.cuda.synchronize()
    assert launches == ["agrl_adam_step" if adam else "agrl_sgd_step"]          # one launch for all the tensors
    for s in streams:
        assert slabs[s].outside_intact(), s
        assert bool(torch.isfinite(slabs[s].cat()).all()), s
    assert not slabs["g"].cat().view(torch.int32).any()
    got = {s: slabs[s].cat() for s in streams if s != "g"}
    if kind == "nesterov_first":
        got["buf"] = torch.cat([opt.state[p]["momentum_buffer"] for p in params])
    hold("guarded %s" % kind, got, exact, table)
    aligned = all(o == 0 for o in offsets.values())
    # the state tensors the optimiser allocates itself (nesterov_first) are aligned: the parameter / gradient offsets decide
    assert next(iter(opt._tables.values()))[2][:, 6].tolist() == [1 if aligned else 0] * len(sizes)


@pytest.mark.parametrize("kind", ["adam", "amsgrad", "sgd", "nesterov_first"])
@pytest.mark.parametrize("offset", [0, 4, 8, 12, "mixed"])
def test_edge_sizes_write_nothing_outside_the_tensors(kind, offset):
    offsets = dict(zip(("p", "g", "m", "v", "vmax", "buf"), (0, 4, 8, 12, 4, 8))) if offset == "mixed" else {s: offset for s in ("p", "g", "m", "v", "vmax", "buf")}
    _guarded_step(kind, SIZES, offsets)


@pytest.mark.parametrize("kind", ["adam", "sgd"])
@pytest.mark.parametrize("offset", [0, 4])
def test_300_small_tensors_in_one_call(kind, offset):
    sizes = [int(v) for v in np.random.RandomState(0).randint(1, 8, size=300)]
    _guarded_step(kind, sizes, {s: offset for s in ("p", "g", "m", "v", "vmax", "buf")})


@pytest.mark.parametrize("offset", [0, 12])
def test_one_tensor_longer_than_the_grid(offset):
    """grid x chunk + 5 elements: every workgroup takes a second trip through the stride loop, the last chunk is ragged."""
    _guarded_step("adam", [MAX_GRID * C + 5], {s: offset for s in ("p", "g", "m", "v")})


# ---- skip semantics, zero_grads, run to run -------------------------------------------------------------------------------------
def bits(t):
    return t.detach().view(torch.int32).clone()


def test_parameters_without_gradient_are_skipped_like_in_torch():
    gen = torch.Generator().manual_seed(404)
    sizes = [C + 9, 17, 2 * C, 5, 33]
    P, G = Slab(sizes, [0] * 5).fill(rand_p, gen), Slab(sizes, [0] * 5)
    params = slab_params(P)
    opt = HipAdam(params, lr=1e-3, weight_decay=5e-4)

    def arm(active):
        G.fill(rand_g, gen)
        for i, p in enumerate(params):
            p.grad = G.views[i] if i in active else None

    arm({0, 1, 2, 3})                                     # the fifth parameter has no gradient yet
    opt.step()
    assert params[4] not in opt.state and all(float(opt.state[params[i]]["step"]) == 1 for i in range(4))
    arm({0, 2})
    frozen = {i: (bits(params[i]), bits(opt.state[params[i]]["exp_avg"]), bits(opt.state[params[i]]["exp_avg_sq"])) for i in (1, 3)}
    p4 = bits(params[4])
    opt.step()
    for i, (bp, bm, bv) in frozen.items():
        st = opt.state[params[i]]
        assert torch.equal(bits(params[i]), bp) and torch.equal(bits(st["exp_avg"]), bm) and torch.equal(bits(st["exp_avg_sq"]), bv)
        assert float(st["step"]) == 1
    assert torch.equal(bits(params[4]), p4) and params[4] not in opt.state
    assert float(opt.state[params[0]]["step"]) == float(opt.state[params[2]]["step"]) == 2
    # the same active set again: the cached tables serve it -- no rebuild, no allocation
    arm({0, 2})
    tables, allocated = len(opt._tables), torch.cuda.memory_allocated()
    opt.step()
    assert len(opt._tables) == tables and torch.cuda.memory_allocated() == allocated
    # now everything has a gradient: step counts 4, 2, 4, 2, 1 -> three launch classes, each held to the contract with ITS count
    arm({0, 1, 2, 3, 4})
    before = {i: (d64(params[i]), d64(G.views[i])) + tuple(d64(opt.state[params[i]][k]) if params[i] in opt.state else torch.zeros(sizes[i], dtype=torch.float64, device=DEV)
                                                            for k in ("exp_avg", "exp_avg_sq")) for i in range(5)}
    _hip.PROFILE = []
    try:
        opt.step()
    finally:
        launches, _hip.PROFILE = [r[0] for r in _hip.PROFILE], None
    assert launches == ["agrl_adam_step"] * 3
    for i, t in enumerate([4, 2, 4, 2, 1]):
        p0, g0, m0, v0 = before[i]
        st = opt.state[params[i]]
        assert float(st["step"]) == t
        hold("mixed step counts, tensor %d (t = %d)" % (i, t), {"p": params[i], "m": st["exp_avg"], "v": st["exp_avg_sq"]},
             adam_exact(p0, g0, m0, v0, v0, 1e-3, (0.9, 0.999), 1e-8, 5e-4, t, False), N_ADAM)
    assert P.outside_intact() and G.outside_intact()


@pytest.mark.parametrize("kind", ["adam", "amsgrad", "sgd", "nesterov"])
def test_zero_grads_and_run_to_run(kind):
    """zero_grads=True: every consumed gradient is bitwise +0.0 afterwards; off: bitwise unchanged. Two runs from one state are bitwise
    equal in p and state, with the flag on or off."""
    sizes = [2 * C + 3, 7, C]
    runs = []
    for zero in (False, False, True):
        gen = torch.Generator().manual_seed(505)
        P, G = Slab(sizes, [0, 4, 0]).fill(rand_p, gen), Slab(sizes, [0, 4, 0])
        params = slab_params(P)
        if kind in ("adam", "amsgrad"):
            opt = HipAdam(params, lr=1e-3, weight_decay=5e-4, amsgrad=kind == "amsgrad", zero_grads=zero)
        else:
            opt = HipSGD(params, lr=0.1, momentum=0.9, weight_decay=5e-4, nesterov=kind == "nesterov", zero_grads=zero)
        for _ in range(3):
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
        runs.append([bits(P.cat())] + state)
    for other in runs[1:]:
        assert len(other) == len(runs[0]) and all(torch.equal(a, b) for a, b in zip(runs[0], other))


def test_new_gradient_tensors_a_reloaded_state_dict_and_an_edited_count_are_picked_up():
    """The step trusts what it validated only while the same tensors sit at the same addresses: re-allocated .grad tensors get a new
    table, load_state_dict() rewinds state and counts, and a count somebody else wrote is read again."""
    gen = torch.Generator().manual_seed(707)
    sizes = [C + 11, 6]
    params = [torch.nn.Parameter(rand_p(n, gen).to(DEV)) for n in sizes]
    opt = HipAdam(params, lr=1e-3, weight_decay=5e-4)

    def fresh_grads(seed):
        g_ = torch.Generator().manual_seed(seed)
        for p in params:
            p.grad = rand_g(p.numel(), g_).to(DEV)              # a new tensor every time, as after zero_grad(set_to_none=True)

    def snapshot():
        return [bits(p) for p in params] + [bits(opt.state[p][k]) for p in params for k in ("exp_avg", "exp_avg_sq")]

    fresh_grads(1)
    opt.step()
    saved, p_saved = copy.deepcopy(opt.state_dict()), [p.detach().clone() for p in params]
    fresh_grads(2)
    keep = [p.grad for p in params]                              # (keeps the first step's addresses from being reused)
    before = [(d64(p), d64(p.grad), d64(opt.state[p]["exp_avg"]), d64(opt.state[p]["exp_avg_sq"])) for p in params]
    opt.step()
    for i, (p0, g0, m0, v0) in enumerate(before):
        st = opt.state[params[i]]
        hold("re-allocated gradients, tensor %d" % i, {"p": params[i], "m": st["exp_avg"], "v": st["exp_avg_sq"]},
             adam_exact(p0, g0, m0, v0, v0, 1e-3, (0.9, 0.999), 1e-8, 5e-4, 2, False), N_ADAM)
    second = snapshot()
    assert len(opt._tables) == 2 and all(float(opt.state[p]["step"]) == 2 for p in params)
    # rewind: the saved state and parameters, the same gradients -> the same bits, and the counts say 2 again
    opt.load_state_dict(saved)
    with torch.no_grad():
        for p, q in zip(params, p_saved):
            p.copy_(q)
    fresh_grads(2)
    opt.step()
    assert all(torch.equal(a, b) for a, b in zip(snapshot(), second)) and all(float(opt.state[p]["step"]) == 2 for p in params)
    # a count written from outside is what the next step uses
    opt.state[params[1]]["step"].fill_(7.0)
    g_ = torch.Generator().manual_seed(3)
    for p in params:
        p.grad.copy_(rand_g(p.numel(), g_))                     # the same tensors: nothing but the count changed
    before = [(d64(p), d64(p.grad), d64(opt.state[p]["exp_avg"]), d64(opt.state[p]["exp_avg_sq"])) for p in params]
    opt.step()
    for i, t in enumerate([3, 8]):
        p0, g0, m0, v0 = before[i]
        st = opt.state[params[i]]
        assert float(st["step"]) == t
        hold("edited count, tensor %d (t = %d)" % (i, t), {"p": params[i], "m": st["exp_avg"], "v": st["exp_avg_sq"]},
             adam_exact(p0, g0, m0, v0, v0, 1e-3, (0.9, 0.999), 1e-8, 5e-4, t, False), N_ADAM)
    del keep


# ---- state dicts on the device ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", ["native_to_torch", "torch_to_native"])
def test_state_dict_moves_between_the_native_and_the_stock_optimiser(direction):
    gen = torch.Generator().manual_seed(606)
    sizes = [C + 37, 129]
    kw = dict(lr=1e-3, weight_decay=5e-4)
    a = [torch.nn.Parameter(rand_p(n, gen).to(DEV)) for n in sizes]
    first = HipAdam(a, **kw) if direction == "native_to_torch" else torch.optim.Adam(a, foreach=False, **kw)
    for _ in range(3):
        for p in a:
            p.grad = rand_g(p.numel(), gen).to(DEV)
        first.step()
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    second = torch.optim.Adam(b, foreach=False, **kw) if direction == "native_to_torch" else HipAdam(b, **kw)
    second.load_state_dict(copy.deepcopy(first.state_dict()))
    assert first.state_dict()["state"][0].keys() == second.state_dict()["state"][0].keys() == {"step", "exp_avg", "exp_avg_sq"}
    grads = [rand_g(p.numel(), gen).to(DEV) for p in a]
    cat = lambda params, key: torch.cat([first.state[p][key] for p in params])
    exact = adam_exact(d64(torch.cat(list(a))), d64(torch.cat(grads)), d64(cat(a, "exp_avg")), d64(cat(a, "exp_avg_sq")), d64(cat(a, "exp_avg_sq")),
                       1e-3, (0.9, 0.999), 1e-8, 5e-4, 4, False)
    for params, opt, name in ((a, first, "first"), (b, second, "second")):
        for p, g in zip(params, grads):
            p.grad = g.clone()
        opt.step()
        assert all(float(opt.state[p]["step"]) == 4 for p in params)
        got = {"p": torch.cat(list(params)), "m": torch.cat([opt.state[p]["exp_avg"] for p in params]),
               "v": torch.cat([opt.state[p]["exp_avg_sq"] for p in params])}
        hold("%s, %s optimiser (%s)" % (direction, name, type(opt).__name__), got, exact, N_ADAM)


# ---- inside parallel.train_step ---------------------------------------------------------------------------------------------------
def test_native_optimiser_inside_the_bucketed_train_step():
    """One xent + htri step of the smallest vmgn (B = 4, S = 4, 64 x 32 frames, 16 classes) under GradientBuckets with HipAdam, against
    a deep copy stepped by torch.optim.Adam(foreach=False) on the plain path: the native gradients are run-to-run bit-equal, so both
    sides must land within the p bound of the exact update of THOSE gradients; the bucket buffers are bitwise zero afterwards. Then an
    htri-only step with a fresh optimiser: the classifiers keep their bits and get no state."""
    from recipe import recipe_state_dict, synthetic_adj, synthetic_clips
    from torchreid import losses, models, parallel
    m = models.init_model("vmgn", num_classes=16, loss={"xent", "htri"}, last_stride=1, num_split=4, num_gb=2, num_scale=1,
                          pyramid_part=True, use_pose=True, learn_graph=True, consistent_loss=False)
    m.load_state_dict(recipe_state_dict(m.state_dict(), seed=3))
    m = m.to(DEV)
    assert m.hip_train
    twin = copy.deepcopy(m)
    pids = torch.arange(2).repeat_interleave(2)
    x = synthetic_clips(4, 4, H=64, W=32, seed=9, identities=pids.tolist()).to(DEV)
    adj, pids = synthetic_adj(4, 4, seed=9).to(DEV), pids.to(DEV)
    ce, tri = losses.CrossEntropyLabelSmooth(num_classes=16, use_gpu=True), losses.TripletLoss(margin=0.3, soft=True)
    kw = dict(lr=1e-3, weight_decay=5e-4)
    buckets = parallel.GradientBuckets(m.parameters(), bucket_bytes=8 << 20)
    opt, opt_twin = HipAdam(m.parameters(), **kw), torch.optim.Adam(twin.parameters(), foreach=False, **kw)
    seen = {}

    def snapshot(model, tag):
        def hook(optimizer, args, kwargs):
            seen[tag] = {k: (d64(p), d64(p.grad)) for k, p in model.named_parameters() if p.grad is not None}
        return hook
    opt.register_step_pre_hook(snapshot(m, "native"))
    opt_twin.register_step_pre_hook(snapshot(twin, "twin"))
    loss = parallel.train_step(m, x, adj, pids, ce, tri, opt, buckets=buckets)
    loss_twin = parallel.train_step(twin, x, adj, pids, ce, tri, opt_twin)
    torch.cuda.synchronize()
    assert loss == loss_twin and set(seen["native"]) == set(seen["twin"]) and len(seen["native"]) > 100
    assert all(not flat.view(torch.int32).any() for flat, _ in buckets.buckets) and buckets._clean
    after, after_twin = dict(m.named_parameters()), dict(twin.named_parameters())
    worst, same = [], []
    for k, (p0, g0) in seen["native"].items():
        same.append((g0 == seen["twin"][k][1]).all())                       # run-to-run bit-equal gradients
        zero = torch.zeros_like(p0).reshape(-1)
        ex, mag = adam_exact(p0.reshape(-1), g0.reshape(-1), zero, zero, zero, 1e-3, (0.9, 0.999), 1e-8, 5e-4, 1, False)["p"]
        worst += [ratio_on_device(after[k], ex, mag, N_ADAM["p"]), ratio_on_device(after_twin[k], ex, mag, N_ADAM["p"])]
    worst = torch.stack(worst).view(-1, 2).cpu()
    same = torch.stack(same).cpu()
    print("train_step under buckets: %d tensors, %d with bit-equal gradients; worst |p - exact| / bound: native %.3f, torch %.3f"
          % (len(same), int(same.sum()), float(worst[:, 0].max()), float(worst[:, 1].max())))
    log_record({"name": "hip_optim train_step worst p ratio", "native": float(worst[:, 0].max()), "torch": float(worst[:, 1].max())})
    names = list(seen["native"])
    assert bool(same.all()), [names[i] for i in torch.nonzero(~same).view(-1).tolist()][:5]
    assert bool((worst <= 1.0).all()), [(names[i], worst[i].tolist()) for i in torch.nonzero(~(worst <= 1.0).all(1)).view(-1).tolist()][:5]
    untouched = [k for k, p in m.named_parameters() if p.requires_grad and k not in seen["native"]]
    assert all(after[k] not in opt.state for k in untouched)
    # htri-only: the classifiers receive no gradient
    heads = [k for k in after if "classifier" in k]
    assert len(heads) >= 2
    kept = {k: bits(after[k]) for k in heads}
    opt2 = HipAdam(m.parameters(), **kw)
    parallel.train_step(m, x, adj, pids, ce, tri, opt2, htri_only=True, buckets=buckets)
    torch.cuda.synchronize()
    for k in heads:
        assert torch.equal(bits(after[k]), kept[k]) and after[k] not in opt2.state, k
    assert len(opt2.state) > 100 and all(not flat.view(torch.int32).any() for flat, _ in buckets.buckets)
    assert all(p.grad is not None for p in m.parameters() if p.requires_grad)      # the views are back
    buckets.remove()


# ---- host errors: raised before anything is launched -----------------------------------------------------------------------------
def test_unsupported_inputs_raise_before_any_launch(monkeypatch):
    launched = []
    monkeypatch.setattr(ops, "call", lambda name, *args: launched.append(name))

    def param(t):
        p = torch.nn.Parameter(t)
        p.grad = torch.ones_like(t)
        return p
    good = param(torch.ones(8, device=DEV))
    cases = [
        (TypeError, lambda: HipAdam([good, param(torch.ones(8, device=DEV, dtype=torch.float64))])),
        (TypeError, lambda: HipSGD([param(torch.ones(8, device=DEV, dtype=torch.float16))], lr=0.1)),
        (ValueError, lambda: HipAdam([good, param(torch.ones(4, 6, device=DEV).t())])),
        (ValueError, lambda: HipSGD([param(torch.ones(4, 6, device=DEV)[:, ::2])], lr=0.1)),
        (NotImplementedError, lambda: HipAdam([good], maximize=True)),
        (NotImplementedError, lambda: HipAdam([good], capturable=True)),
        (NotImplementedError, lambda: HipAdam([good], differentiable=True)),
        (NotImplementedError, lambda: HipSGD([good], lr=0.1, maximize=True)),
        (NotImplementedError, lambda: HipSGD([good], lr=0.1, differentiable=True)),
        (NotImplementedError, lambda: HipSGD([good], lr=0.1, momentum=0.9, dampening=0.1)),
    ]
    for exc, make in cases:
        opt = make()
        with pytest.raises(exc):
            opt.step()
    sparse = torch.nn.Parameter(torch.ones(8, device=DEV))
    sparse.grad = torch.sparse_coo_tensor(torch.tensor([[1, 3]]), torch.tensor([1.0, 2.0]), (8,)).to(DEV)
    for opt in (HipAdam([good, sparse]), HipSGD([sparse], lr=0.1)):
        with pytest.raises(NotImplementedError, match="sparse"):
            opt.step()
    assert launched == [] and bool((good == 1).all())
    HipAdam([good]).step()
    assert launched == ["agrl_adam_step"]            # (the stub sees the launch of a supported step)
