"""ganet's position-attention part nodes under train(), the part that needs no GPU: the folded backward the kernels implement
(hip_ops.pam_nodes_backward_reference: the value conv as ONE matrix-vector product per node, csrc/pam.hip) against float64
autograd through the package's literal PAM_Module -- value conv on every position, ``pam(piece) + piece`` average pooled, per
pyramid slice, as GANet.forward does it -- and the routing of CPU tensors, which the native train step must not change."""
import numpy as np
import pytest
import torch


def literal_nodes(pam, fm, splits):
    """GANet.forward's part nodes (ganet.py:384-400 of the reference): fm (F,C,h,w) -> (F,P,C)."""
    F_, c, h, w = fm.shape
    nodes = []
    for n in splits:
        step = h // n
        for i in range(n):
            piece = fm[:, :, step * i: step * (i + 1)]
            pam_f, _ = pam(piece)
            nodes.append(torch.nn.functional.adaptive_avg_pool2d(pam_f + piece, 1).view(F_, c))
    return torch.stack(nodes, dim=2).transpose(1, 2).contiguous()


@pytest.mark.parametrize("shape,splits", [((2, 6, 5, 24, 8), [4, 2, 1]), ((1, 4, 3, 16, 8), [1])])
def test_folded_backward_equals_float64_autograd_through_the_literal_module(shape, splits):
    """Every gradient: map, Wq, bq, Wk, Wv, bv, gamma to 1e-12 relative (float64 against float64), the key bias -- identically
    zero, since it shifts every energy of a row alike -- to 1e-12 absolute."""
    from torchreid import hip_ops as ops
    from torchreid.models.ganet import PAM_Module
    F_, h, w, C, Cq = shape
    assert C // 8 * 8 == C
    torch.manual_seed(sum(shape))
    pam = PAM_Module(C).double()
    assert pam.query_conv.weight.shape[0] == C // 8
    if Cq != C // 8:   # the issue's shapes ask for Cq = 8 whatever C is
        pam.query_conv = torch.nn.Conv2d(C, Cq, 1).double()
        pam.key_conv = torch.nn.Conv2d(C, Cq, 1).double()
    with torch.no_grad():
        for p in pam.parameters():
            p.copy_(torch.randn_like(p) * 0.5)
        pam.gamma.fill_(0.7)
    fm = torch.randn((F_, C, h, w), dtype=torch.float64, requires_grad=True)
    nodes = literal_nodes(pam, fm, splits)
    dnodes = torch.randn_like(nodes)
    nodes.backward(dnodes)
    ref = ops.pam_nodes_backward_reference(
        fm.detach().permute(0, 2, 3, 1).contiguous(), pam.query_conv.weight.detach().view(Cq, C), pam.query_conv.bias.detach(),
        pam.key_conv.weight.detach().view(Cq, C), pam.key_conv.bias.detach(), pam.value_conv.weight.detach().view(C, C),
        pam.value_conv.bias.detach(), pam.gamma.detach(), splits, dnodes)

    def close(got, want, name):
        err = float((got - want).abs().max() / want.abs().max())
        assert err <= 1e-12, (name, err)
    close(ref["nodes"], nodes.detach(), "nodes")
    close(ref["dx"].permute(0, 3, 1, 2), fm.grad, "map")
    close(ref["dwq"], pam.query_conv.weight.grad.view(Cq, C), "Wq")
    close(ref["dbq"], pam.query_conv.bias.grad, "bq")
    close(ref["dwk"], pam.key_conv.weight.grad.view(Cq, C), "Wk")
    close(ref["dwv"], pam.value_conv.weight.grad.view(C, C), "Wv")
    close(ref["dbv"], pam.value_conv.bias.grad, "bv")
    close(ref["dgamma"].view(1), pam.gamma.grad, "gamma")
    assert float(ref["dbk"].abs().max()) <= 1e-12 and float(pam.key_conv.bias.grad.abs().max()) <= 1e-12
    if splits == [4, 2, 1]:   # h = 6: the four-slice level drops rows 4 and 5, which still carry the other levels' gradient
        assert h % 4 and float(ref["dx_pool"][:, 4:].abs().min()) > 0 and float(ref["dqk"][:, 4:].abs().max()) > 0


def test_dgamma_is_not_zero_at_gamma_zero():
    """The eval shortcut 'gamma 0: means only' does not carry over to training."""
    from torchreid import hip_ops as ops
    g = torch.Generator().manual_seed(3)
    F_, h, w, C, Cq = 1, 4, 3, 16, 8
    r = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)
    ref = ops.pam_nodes_backward_reference(r(F_, h, w, C), r(Cq, C), r(Cq), r(Cq, C), r(Cq), r(C, C), r(C), torch.zeros((), dtype=torch.float64),
                                           [2, 1], r(F_, 3, C))
    assert abs(float(ref["dgamma"])) > 1e-3 and float(ref["dqk"].abs().max()) == 0 and float(ref["dwv"].abs().max()) == 0


def test_ganet_cpu_train_forward_does_not_depend_on_hip_train():
    """CPU tensors in train() take the stock module tree whatever hip_train says: the same seeds give the same outputs."""
    from recipe import recipe_state_dict, synthetic_adj, synthetic_clips
    from torchreid import models
    kw = dict(num_classes=5, loss={"xent", "htri"}, last_stride=1, num_split=4, num_gb=2, num_scale=1, knn=4, pyramid_part=True,
              use_pose=True, learn_graph=True, consistent_loss=True, pretrained=False)
    m = models.init_model("ganet", **kw)
    assert m.hip_train and m.hip_train_precision == "fp32"
    sd = recipe_state_dict(m.state_dict(), seed=5)
    x, adj = synthetic_clips(2, 5, H=64, W=32, seed=17), synthetic_adj(2, 5, seed=17)
    res = []
    for flag in (True, False):
        m.load_state_dict(sd)
        m.hip_train = flag
        m.train()
        np.random.seed(11)
        torch.manual_seed(11)
        outs, feats = m(x, adj)
        res.append([t.detach() for t in list(outs) + list(feats)])
    assert len(res[0]) == 4
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_train_entry_points_validate_before_any_launch():
    """Argument validation precedes every launch, so it is checkable without a GPU (as test_boundary.py does for the distance
    matrix): null pointers, Cq % 32, at most 16 parts, at most 128 positions per slice, dtype, workspace sizes."""
    import ctypes as C
    from torchreid import _hip
    lib = _hip.lib()
    b = 4096   # a non-null pointer no rejected call dereferences

    def arr(*v):
        return (C.c_int * len(v))(*v)

    def fwd(x=b, F=1, h=4, w=4, Cq=32, sp=arr(2, 1), n=2, dt=_hip.F32):
        return lib.agrl_pam_pool_train(x, b, b, b, b, F, h, w, 64, Cq, sp, n, dt, None), lib.agrl_last_error().decode()

    def bwd(x=b, F=1, h=4, w=4, Cq=32, sp=arr(2, 1), n=2, dt=_hip.F32):
        return lib.agrl_pam_pool_backward(x, b, b, b, b, b, b, F, h, w, 64, Cq, sp, n, dt, None), lib.agrl_last_error().decode()
    for fn in (fwd, bwd):
        for kw, text in ((dict(x=None), "null pointer"), (dict(Cq=24), "multiple of 32"), (dict(h=32, w=1, sp=arr(16, 1)), "at most 16 parts"),
                         (dict(h=17, w=8, sp=arr(1), n=1), "at most 128 supported"), (dict(dt=_hip.LP16), "bad dtype"), (dict(F=0), "bad shape")):
            status, msg = fn(**kw)
            assert status != 0 and text in msg, (kw, msg)
    assert lib.agrl_pam_combine_train(b, b, b, None, b, 4, 64, None) != 0 and b"null pointer" in lib.agrl_last_error()
    need = lib.agrl_col_sum_workspace(64, 64)
    assert need == (2 * 2 + 1) * 64 * 4 and lib.agrl_col_sum_workspace(8192, 512) == (2 * 64 + 1) * 512 * 4
    assert lib.agrl_pam_combine_backward(b, b, b, b, b, b, b, b, 64, 64, b, need - 1, None) != 0 and b"workspace too small" in lib.agrl_last_error()
    assert lib.agrl_col_sum(b, b, 64, 64, b, need - 1, None) != 0 and b"workspace too small" in lib.agrl_last_error()
