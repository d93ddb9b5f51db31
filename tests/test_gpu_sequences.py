"""Sequences of calls that share state, on the GPU: an eval forward after the native training path wrote the model.

The eval forward keeps its BN-folded, re-laid-out weights on the model (``_resnet_hip.pack_weights``, ``model._hip_packs``) for as long as
``fingerprint(model)`` -- (data_ptr, _version) of every parameter and buffer -- stands. The native optimisers (torchreid.hip_optim) and the
native train-mode BatchNorm (``hip_ops.bn_fold_train``) write those tensors through raw pointers; torch's version counters only see
the writes because the wrappers bump them (``torch.autograd.graph.increment_version``). Without the bump every eval forward after the first
serves the first one's pack: the driver's second ``test()`` reports the first one's Rank-1 again, and nothing raises.

Everything runs at the smallest model the suite uses (16 classes, recipe seed 3, B = 4 tracklets x S = 4 frames of 64 x 32, clips and
pose graph of seed 9, xent + htri, weight decay 5e-4).

The one oracle for "fresh": a second model object on the device, loaded with ``load_state_dict`` from the trained model's
``state_dict()`` -- the bytes the kernels really wrote --, whose ``_hip_packs`` is empty. Its eval embedding must be ``torch.equal`` to the
trained model's: the same kernels on the same weights, and eval forwards are run-to-run bit-equal, so there is no tolerance.

The tests can tell: bit-equality with a fresh model would also hold on a model nothing had written. So every case first asserts that
the embedding moved, between the forward that built the pack and the forward that must not reuse it, by at least 100 x the mode's
parity bar (tests/test_gpu_model.py: fp32 and bf16x3 1e-3, fp16x3 1e-4, the 16-bit mode lp16.LP_EMBED_TOL) relative to its maximum. That is a
condition on the inputs: on the CPU the stock module path moves it, buffers restored, by 0.17 (adam, amsgrad, lr 1e-3), 0.17
(adabound 1e-3), 0.20 (rmsprop 1e-4), 0.22 (sgd 0.03), 0.62 (nesterov 0.02), 0.57 (radam 0.05: its first four steps are plain
momentum steps) after two steps, gsta 0.16 and ganet 0.20 under adam; one train-mode forward alone moves it by 0.18; the driver's
loop by 0.44 and 0.32 between its evaluations. The learning rates are chosen for that and for nothing else (sgd at 0.05 and rmsprop
at 1e-3 leave the recipe's weights for infinity within three steps).

What holds which bump. The fingerprint covers parameters AND buffers, and every ``parallel.train_step`` runs a native train-mode forward,
whose BatchNorm bump alone renews it. So in the cases that train through ``train_step`` (a, c, d, f) the embeddings hold the sequence end
to end -- some bump renewed the pack, and the pack is right -- but not the optimiser's bump in particular. That one is held by
  * ``hold_parameter_versions`` inside every ``train()``: each parameter the optimiser stepped stands exactly ``steps`` versions higher,
    each other one where it was (all seven names, gsta, ganet, the bucketed route);
  * case a', on the embeddings: the pack is built AFTER the forward + backward that leaves the gradients, then two bare ``step()`` and
    nothing else, so no buffer moves between the two evaluations (all seven names, gsta, ganet: on the CPU 0.20 .. 0.41);
  * case g (autograd reads the parameter versions only) and, without a GPU, tests/test_hip_optim.py (all seven names, stubbed launch).
The BatchNorm bump is held by case b, where nothing but running statistics is written.

Case (a) restores the running statistics before the second evaluation so that the embedding's MOVEMENT is the parameter writes' alone. It
restores the bits through ``buffer.data.copy_``; the versions the train forwards gave the buffers stay, see above.

Measured on an MI355X: profiles/sequences.txt."""
import copy
import ctypes

import pytest
import torch

from bounds import log_record
from lp16 import LP16, LP_EMBED_TOL
from oracle import vmgn_oracle as O
from recipe import recipe_state_dict, synthetic_adj, synthetic_clips

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WD = 5e-4
BAR = {"fp32": 1e-3, "bf16x3": 1e-3, "fp16x3": 1e-4, LP16: LP_EMBED_TOL}     # the eval bars of tests/test_gpu_model.py
LR = {"adam": 1e-3, "amsgrad": 1e-3, "sgd": 0.03, "nesterov": 0.02, "rmsprop": 1e-4, "adabound": 1e-3, "radam": 0.05}
KW = dict(num_classes=16, loss={"xent", "htri"}, last_stride=1, num_split=4, num_gb=2, num_scale=1, pyramid_part=True, use_pose=True,
          learn_graph=True, consistent_loss=False)
EXTRA = {"vmgn": {}, "gsta": {}, "ganet": {"knn": 4, "pretrained": False}}
_BASE, _INPUTS = {}, {}


# ---- models, inputs, the two forwards ------------------------------------------------------------------------------------------
def build(name, device=DEV):
    """A new model object with the recipe's weights (seed 3) on ``device``; nothing cached on it."""
    from torchreid import models
    if name not in _BASE:
        m = models.init_model(name, **dict(KW, **EXTRA[name]))
        m.load_state_dict(recipe_state_dict(m.state_dict(), seed=3))
        _BASE[name] = m
    m = copy.deepcopy(_BASE[name]).to(device)
    assert not m._hip_packs
    return m


def inputs(device=DEV):
    if device not in _INPUTS:
        pids = torch.arange(2).repeat_interleave(2)
        x = synthetic_clips(4, 4, H=64, W=32, seed=9, identities=pids.tolist())
        _INPUTS[device] = (x.to(device), synthetic_adj(4, 4, seed=9).to(device), pids.to(device))
    return _INPUTS[device]


def criteria(use_gpu=True):
    from torchreid import losses
    return losses.CrossEntropyLabelSmooth(num_classes=16, use_gpu=use_gpu), losses.TripletLoss(margin=0.3, soft=True)


def embed(m, precision="fp32"):
    """The eval forward as the driver's test() runs it: no invalidation, whatever is cached on the model is used."""
    x, adj, _ = inputs()
    m.eval()
    m.hip_precision = precision
    with torch.no_grad():
        out = m(x, adj)
    torch.cuda.synchronize()
    assert out.is_cuda and bool(torch.isfinite(out).all())
    return out.clone()


def fresh_embed(name, trained, precision="fp32"):
    """THE oracle for "fresh": another model object, loaded from the bytes in ``trained``'s tensors, with nothing cached."""
    fresh = build(name)
    fresh.load_state_dict(trained.state_dict())
    assert not fresh._hip_packs and fresh is not trained
    return embed(fresh, precision)


def train(m, opt, steps, buckets=None):
    from torchreid import parallel
    x, adj, pids = inputs()
    ce, tri = criteria()
    assert m.hip_train
    versions = {k: p._version for k, p in m.named_parameters()}
    for _ in range(steps):
        parallel.train_step(m, x, adj, pids, ce, tri, opt, buckets=buckets)
    torch.cuda.synchronize()
    hold_parameter_versions(m, opt, versions, steps)


def hold_parameter_versions(m, opt, versions, steps):
    """THE guard of the optimiser's own bump: nothing else in a train step touches a parameter's version, so every parameter the
    optimiser stepped (it has state) stands exactly ``steps`` above ``versions`` and every other one where it was. The embeddings
    cannot show this once a train forward ran: the running statistics' bump alone renews the fingerprint."""
    stepped = {k: p._version - versions[k] for k, p in m.named_parameters() if p in opt.state}
    rest = {k: p._version - versions[k] for k, p in m.named_parameters() if p not in opt.state}
    assert len(stepped) > 100
    assert all(d == steps for d in stepped.values()), "parameter versions moved by %s, not %d: %s" % (
        sorted(set(stepped.values())), steps, [k for k, d in stepped.items() if d != steps][:5])
    assert not any(rest.values()), [k for k, d in rest.items() if d][:5]


def native_optimiser(optim, m):
    from torchreid.hip_optim import NativeStepMixin, init_optim_native
    opt = init_optim_native(optim, m.parameters(), LR[optim], WD)
    assert isinstance(opt, NativeStepMixin)
    return opt


def moved(before, after):
    return float((after.double() - before.double()).abs().max() / before.double().abs().max())


def hold_to_fresh(case, before, after, fresh, bar, packs=None):
    """What every case asserts. before / after: the embeddings around the writes (the pack was built for ``before``), fresh: the fresh
    model's on the written weights, packs: (the pack object before, after) where a rebuild is expected. Figures first."""
    move, differ = moved(before, after), int((after != fresh).sum())
    print("%s: embedding moved by %.3f of its maximum (needs %.3g); %d of %d elements differ from the fresh model's; pack %s" % (
        case, move, 100 * bar, differ, after.numel(), "-" if packs is None else ("kept" if packs[0] is packs[1] else "rebuilt")))
    log_record({"name": "sequences " + case, "moved": move, "differ": differ})
    assert torch.equal(after, fresh), "%s: the evaluation did not see the written weights -- %d of %d elements differ from a fresh model's%s" % (
        case, differ, after.numel(), " (bit-equal to the evaluation BEFORE the writes: a stale pack)" if torch.equal(after, before) else "")
    assert packs is None or packs[0] is not packs[1], "%s: the pack object survived the writes" % case
    assert move >= 100 * bar, "%s: the inputs cannot tell a stale pack from a fresh one (moved %.3g)" % (case, move)


# ---- a. parameters -----------------------------------------------------------------------------------------------------------------
CASES_A = [("vmgn", optim, False) for optim in ("adam", "amsgrad", "sgd", "nesterov", "rmsprop", "adabound", "radam")]
CASES_A += [("gsta", "adam", False), ("ganet", "adam", False), ("vmgn", "adam", True)]


@pytest.mark.parametrize("name,optim,bucketed", CASES_A, ids=["%s-%s%s" % (n, o, "-buckets" if b else "") for n, o, b in CASES_A])
def test_eval_after_native_steps_sees_the_stepped_parameters(name, optim, bucketed):
    """eval (pack built and kept) -> two parallel.train_step with the native optimiser -> running statistics' bits put back -> eval.
    The optimiser's bump is asserted on the parameter versions inside train(); the embeddings hold the sequence as a whole."""
    from torchreid import parallel
    m = build(name)
    before = embed(m)
    pack = m._hip_packs[(0, "fp32")]
    buffers = [b.detach().clone() for b in m.buffers()]
    opt = native_optimiser(optim, m)
    buckets = parallel.GradientBuckets(m.parameters(), bucket_bytes=8 << 20) if bucketed else None      # the zero_grads=True route
    train(m, opt, 2, buckets)
    if buckets is not None:
        assert all(not flat.view(torch.int32).any() for flat, _ in buckets.buckets)
        buckets.remove()
    for b, saved in zip(m.buffers(), buffers):
        b.data.copy_(saved)               # the bits only: the movement below is the parameters' alone (module docstring)
    after = embed(m)
    hold_to_fresh("a %s %s%s fp32" % (name, optim, " buckets" if bucketed else ""), before, after, fresh_embed(name, m), BAR["fp32"],
                  (pack, m._hip_packs[(0, "fp32")]))


@pytest.mark.parametrize("name,optim", [(n, o) for n, o, b in CASES_A if not b], ids=["%s-%s" % (n, o) for n, o, b in CASES_A if not b])
def test_eval_after_bare_native_steps_sees_the_stepped_parameters(name, optim):
    """Where the embeddings themselves hold the optimiser's bump: one native forward + backward leaves gradients, THEN the pack is built,
    then two bare ``step()`` on those gradients and nothing else -- no forward, so no running statistic and no buffer version moves
    between the two evaluations. Without the step's bump the second evaluation is the first one's, bit for bit. (Two steps on one
    gradient move the embedding on the CPU by 0.29 adam / amsgrad / adabound, 0.23 sgd, 0.27 nesterov, 0.41 rmsprop, 0.35 radam.)"""
    from torchreid import losses
    m = build(name)
    x, adj, pids = inputs()
    ce, tri = criteria()
    opt = native_optimiser(optim, m)
    m.train()
    outs, feats = m(x, adj)
    outs, feats = (outs, feats) if isinstance(outs, (list, tuple)) else ([outs], [feats])
    (losses.DeepSupervision(ce, outs, pids) + losses.DeepSupervision(tri, feats, pids)).backward()
    before = embed(m)
    pack = m._hip_packs[(0, "fp32")]
    versions = {k: p._version for k, p in m.named_parameters()}
    buffers = [(b._version, b.detach().clone()) for b in m.buffers()]
    opt.step()
    opt.step()
    torch.cuda.synchronize()
    hold_parameter_versions(m, opt, versions, 2)
    assert all(b._version == v and torch.equal(b, saved) for b, (v, saved) in zip(m.buffers(), buffers))      # the parameters alone
    after = embed(m)
    hold_to_fresh("a' %s %s bare steps fp32" % (name, optim), before, after, fresh_embed(name, m), BAR["fp32"], (pack, m._hip_packs[(0, "fp32")]))


# ---- b. running statistics -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vmgn", "gsta", "ganet"])
def test_eval_after_a_native_train_forward_sees_the_running_statistics(name):
    """eval -> ONE native train-mode forward, no backward, no step -> eval: only agrl_bn_fold_train wrote anything."""
    m = build(name)
    before = embed(m)
    pack = m._hip_packs[(0, "fp32")]
    norms = [mod for mod in m.modules() if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm)]
    counts = [int(mod.num_batches_tracked) for mod in norms]
    params = [p.detach().clone() for p in m.parameters()]
    x, adj, _ = inputs()
    m.train()
    assert m.hip_train
    m(x, adj)
    torch.cuda.synchronize()
    assert len(norms) > 50 and [int(mod.num_batches_tracked) for mod in norms] == [c + 1 for c in counts]
    assert all(torch.equal(p, q) for p, q in zip(m.parameters(), params))
    after = embed(m)
    hold_to_fresh("b %s train forward fp32" % name, before, after, fresh_embed(name, m), BAR["fp32"], (pack, m._hip_packs[(0, "fp32")]))


# ---- c. every precision's pack ---------------------------------------------------------------------------------------------------
def test_every_precisions_pack_follows_two_native_steps():
    # the cache is host code and does not depend on the 16-bit type: its mode is held in the default build, whose bar a movement can meet
    modes = ["fp32", "bf16x3", "fp16x3"] + ([LP16] if LP16 == "fp16" else [])
    if LP16 not in modes:
        print("c vmgn adam %s: left out on this build (100 x its bar of %g is no movement an embedding can make)" % (LP16, BAR[LP16]))
        log_record({"name": "sequences c vmgn adam " + LP16, "left_out": True})
    m = build("vmgn")
    before = {mode: embed(m, mode) for mode in modes}
    packs = {mode: m._hip_packs[(0, mode)] for mode in modes}
    assert len(set(id(p) for p in packs.values())) == len(modes)
    train(m, native_optimiser("adam", m), 2)
    for mode in modes:
        after = embed(m, mode)
        hold_to_fresh("c vmgn adam %s" % mode, before[mode], after, fresh_embed("vmgn", m, mode), BAR[mode], (packs[mode], m._hip_packs[(0, mode)]))


# ---- d. the driver's loop --------------------------------------------------------------------------------------------------------
def test_the_drivers_loop_evaluates_the_weights_it_trained():
    """eval -> 2 steps -> eval -> 1 step -> eval on a model nobody invalidates, against a twin (a deep copy, the same steps) whose
    cache is dropped by hand before each evaluation: bit-equal three times. The last embedding against oracle.vmgn_eval in float64 on
    the trained state dict, at the fp32 bar of tests/test_gpu_model.py: "fresh" is also right."""
    m = build("vmgn")
    twin = copy.deepcopy(m)
    opt, opt_twin = native_optimiser("adam", m), native_optimiser("adam", twin)
    got, want = [embed(m)], []
    twin.invalidate_hip_cache()
    want.append(embed(twin))
    for steps in (2, 1):
        train(m, opt, steps)
        train(twin, opt_twin, steps)
        got.append(embed(m))
        twin.invalidate_hip_cache()
        want.append(embed(twin))
    moves = [moved(got[i], got[i + 1]) for i in range(2)]
    differ = [int((a != b).sum()) for a, b in zip(got, want)]
    x, adj, _ = inputs("cpu")
    with torch.no_grad():
        ref = O.vmgn_eval(x.double(), adj.double(), {k: v.detach().cpu().double() for k, v in m.state_dict().items()})
    err = float((got[2].cpu().double() - ref).abs().max() / ref.abs().max())
    err_twin = float((want[2].cpu().double() - ref).abs().max() / ref.abs().max())
    print("d vmgn adam fp32: elements that differ from the invalidated twin's at the three evaluations %s of %d; moved %.3f then %.3f; "
          "after the last step max-normalised error against the float64 oracle %.3e (twin %.3e, bar %.0e)" % (
              differ, got[0].numel(), moves[0], moves[1], err, err_twin, BAR["fp32"]))
    log_record({"name": "sequences d vmgn adam fp32", "differ": differ, "moved": moves, "oracle_err": err, "oracle_err_twin": err_twin})
    assert torch.equal(got[0], want[0])
    assert all(mv >= 100 * BAR["fp32"] for mv in moves), moves
    for i in (1, 2):
        assert torch.equal(got[i], want[i]), "evaluation %d: %d of %d elements differ from the invalidated twin's%s" % (
            i + 1, differ[i], got[i].numel(), " (bit-equal to the FIRST evaluation: a stale pack)" if torch.equal(got[i], got[0]) else "")
    assert err < BAR["fp32"] and err_twin < BAR["fp32"]


# ---- e. the check can tell ------------------------------------------------------------------------------------------------------
class RawWritten(torch.nn.Module):
    """torch only: a Linear whose eval forward keeps its transposed weight under _resnet_hip's fingerprint rule, and whose ``step``
    writes the weight as a raw kernel does -- bytes through a pointer (tests/test_parallel_gloo.py fakes one the same way)."""

    def __init__(self):
        super().__init__()
        self.linear = torch.nn.Linear(8, 8, bias=False)
        self.hip_static_weights = False
        self._hip_packs = {}

    def forward(self, x):
        from torchreid.models._resnet_hip import fingerprint
        pack = self._hip_packs.get((0, "fp32"))
        if pack is None or not (self.hip_static_weights or pack["fingerprint"] == fingerprint(self)):
            pack = self._hip_packs[(0, "fp32")] = {"w": self.linear.weight.detach().t().contiguous(), "fingerprint": fingerprint(self)}
        return x @ pack["w"]

    def step(self, bump):
        w = self.linear.weight
        new = (w.detach() * 1.5 + 0.25).contiguous()
        ctypes.memmove(w.data_ptr(), new.data_ptr(), new.numel() * new.element_size())
        if bump:
            torch.autograd.graph.increment_version(w)


@pytest.mark.parametrize("bump", [False, True], ids=["raw write", "raw write and version bump"])
def test_the_check_fails_on_a_model_whose_step_torch_does_not_see(bump):
    """Case (a)'s check on a model whose step is a memmove: it fails, and names the stale pack; with the bump it passes."""
    torch.manual_seed(5)
    m, x = RawWritten().eval(), torch.randn(4, 8)
    with torch.no_grad():
        before = m(x).clone()
        pack, version = m._hip_packs[(0, "fp32")], m.linear.weight._version
        m.step(bump)
        assert m.linear.weight._version == version + (1 if bump else 0)
        after = m(x).clone()
        fresh = RawWritten().eval()
        fresh.load_state_dict(m.state_dict())
        want = fresh(x).clone()
    assert moved(before, want) >= 100 * BAR["fp32"]
    args = ("e torch-only memmove", before, after, want, BAR["fp32"], (pack, m._hip_packs[(0, "fp32")]))
    if bump:
        hold_to_fresh(*args)
    else:
        with pytest.raises(AssertionError, match="a stale pack"):
            hold_to_fresh(*args)


# ---- f. hip_static_weights keeps its meaning ---------------------------------------------------------------------------------------
def test_static_weights_keep_the_pack_across_a_step():
    """``hip_static_weights = True`` is the caller's word that the weights do not change: the pack object survives a native step and
    serves the next forward (the first one's bits); taking the word back rebuilds it."""
    m = build("vmgn")
    m.hip_static_weights = True
    before = embed(m)
    pack = m._hip_packs[(0, "fp32")]
    train(m, native_optimiser("adam", m), 1)
    after = embed(m)
    assert m._hip_packs[(0, "fp32")] is pack and torch.equal(after, before)
    m.hip_static_weights = False
    hold_to_fresh("f vmgn adam fp32, static weights taken back", before, embed(m), fresh_embed("vmgn", m), BAR["fp32"], (pack, m._hip_packs[(0, "fp32")]))


# ---- g. autograd misuse ----------------------------------------------------------------------------------------------------------
def test_backward_after_a_native_step_raises_as_stock_torch_does():
    """forward -> step() -> backward differentiates against weights that changed underneath the graph. Stock torch refuses it through
    the saved tensors' versions; the native nodes keep their weights in save_for_backward, so the native step's bump makes them refuse it too."""
    from torchreid import losses
    from torchreid.hip_optim import HipAdam
    raised = {}
    for side, device in (("stock", "cpu"), ("native", DEV)):
        m = build("vmgn", device)
        x, adj, pids = inputs(device)
        ce, tri = criteria(use_gpu=device != "cpu")
        opt = torch.optim.Adam(m.parameters(), lr=LR["adam"], weight_decay=WD) if side == "stock" else HipAdam(m.parameters(), lr=LR["adam"], weight_decay=WD)
        m.train()
        assert side == "stock" or (m.hip_train and m.hip_train_tail)
        for p in m.parameters():
            if p.requires_grad:
                p.grad = torch.zeros_like(p)        # something for step() to consume
        outs, feats = m(x, adj)
        loss = losses.DeepSupervision(ce, outs, pids) + losses.DeepSupervision(tri, feats, pids)
        opt.step()
        with pytest.raises(RuntimeError, match="modified by an inplace operation") as info:
            loss.backward()
        raised[side] = str(info.value)
        print("g %s: %s" % (side, raised[side].splitlines()[0]))
    assert all("is at version" in msg and "expected version" in msg for msg in raised.values())
