"""The sibling ``ganet`` in train mode on the GPU: the native step (_train_hip.forward_train_ganet: conv trunk, position-attention
part nodes forward and backward, diagonal-masked graph layers, concatenated attention pooling, one BNNeck, the one-frame-dropped
consistent loss) against the stock-torch module tree on the CPU, modelled on test_gpu_train.test_gsta_native_train_step_matches_
cpu_module: same inputs (B = 4, S = 6, 128 x 64 clips, recipe weights, synthetic pose graph) and the same tolerances (outputs
1e-3, loss 1e-4, gradient norm 2e-2, named gradients 5e-2)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (pam_layer.gamma, every graph layer's gamma): as constructed | attention and graph carry gradient
SETTINGS = {"constructed": (0.0, 0.0), "live": (0.5, 0.1)}


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-30)).item()


def build(consistent, setting):
    from recipe import recipe_state_dict, synthetic_adj, synthetic_clips
    from torchreid import models
    kw = dict(num_classes=5, loss={"xent", "htri"}, last_stride=1, num_split=4, num_gb=2, num_scale=1, knn=4, pyramid_part=True,
              use_pose=True, learn_graph=True, consistent_loss=consistent, pretrained=False)
    ref = models.init_model("ganet", **kw)
    sd = recipe_state_dict(ref.state_dict(), seed=5)
    ref.load_state_dict(sd)
    dev = models.init_model("ganet", **kw)
    dev.load_state_dict(sd)
    pam_gamma, layer_gamma = SETTINGS[setting]
    for m in (ref, dev):
        with torch.no_grad():
            m.pam_layer.gamma.fill_(pam_gamma)
        for layer in m.graph_layers:
            layer.gamma = layer_gamma
    pids = torch.tensor([0, 0, 1, 1])
    x, adj = synthetic_clips(4, 6, H=128, W=64, seed=17, identities=pids.tolist()), synthetic_adj(4, 6, seed=17)
    return ref, dev.to(DEV), x, adj, pids


def step(model, x_, adj_, y_, use_gpu):
    from torchreid import losses
    ce = losses.CrossEntropyLabelSmooth(num_classes=5, use_gpu=use_gpu)
    htri = losses.TripletLoss(margin=0.3, soft=True)
    model.train()
    model.zero_grad(set_to_none=True)
    np.random.seed(77)
    outs, feats = model(x_, adj_)
    outs, feats = (outs, feats) if isinstance(outs, (list, tuple)) else ([outs], [feats])
    loss = losses.DeepSupervision(ce, outs, y_) + losses.DeepSupervision(htri, feats, y_)
    loss.backward()
    grads = {k: p.grad.detach().double().cpu() for k, p in model.named_parameters() if p.grad is not None}
    return loss.item(), [o.detach().double().cpu() for o in outs], grads


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("consistent", [False, True])
def test_ganet_native_train_step_matches_cpu_module(consistent, setting, monkeypatch):
    from torchreid import hip_ops as ops
    ref, dev, x, adj, pids = build(consistent, setting)
    assert dev.hip_train
    calls = []
    real = ops.pam_pool_backward
    monkeypatch.setattr(ops, "pam_pool_backward", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    l_ref, o_ref, g_ref = step(ref, x, adj, pids, False)
    l_dev, o_dev, g_dev = step(dev, x.to(DEV), adj.to(DEV), pids.to(DEV), True)
    torch.cuda.synchronize()
    assert len(calls) == 1, "the native position-attention node ran (its backward wrapper was called once)"
    assert len(o_ref) == len(o_dev) == (2 if consistent else 1) and set(g_ref) == set(g_dev)
    assert "cam_layer.gamma" not in g_dev and "pam_layer.gamma" in g_dev
    for a, b in zip(o_dev, o_ref):
        assert rel(a, b) < 1e-3
    assert abs(l_ref - l_dev) < 1e-4 * abs(l_ref)
    gn_ref = torch.sqrt(sum((g ** 2).sum() for g in g_ref.values())).item()
    gn_dev = torch.sqrt(sum((g ** 2).sum() for g in g_dev.values())).item()
    print("ganet train step (consistent=%s, %s): loss cpu %.6f gpu %.6f | grad norm cpu %.4e gpu %.4e" % (consistent, setting, l_ref, l_dev, gn_ref, gn_dev))
    assert abs(gn_ref - gn_dev) < 2e-2 * gn_ref
    named = ["classifier.weight", "layer4.2.conv3.weight", "pam_layer.gamma"]
    if setting == "live":
        named += ["pam_layer.query_conv.weight", "pam_layer.key_conv.weight", "pam_layer.value_conv.weight", "pam_layer.value_conv.bias",
                  "graph_layers.1.linear.weight"]
        # the key bias shifts every energy of a row alike: its gradient is identically zero, noise on both sides -> absolute
        bar = 1e-6 * float(g_ref["pam_layer.query_conv.bias"].abs().max())
        assert bar > 0 and float(g_ref["pam_layer.key_conv.bias"].abs().max()) <= bar and float(g_dev["pam_layer.key_conv.bias"].abs().max()) <= bar
    else:
        assert float(g_ref["pam_layer.gamma"].abs()) > 0 and float(g_dev["pam_layer.gamma"].abs()) > 0
    for k in named:
        print("    %-34s %.2e" % (k, rel(g_dev[k], g_ref[k])))
    for k in named:
        assert rel(g_dev[k], g_ref[k]) < 5e-2, k
    # running statistics moved like nn.BatchNorm's -- the graph layers' too, although gamma = 0 discards their message
    for k in ("bn1.running_mean", "layer4.2.bn3.running_var", "bottleneck.running_mean", "bottleneck.num_batches_tracked",
              "graph_layers.0.bn.running_mean", "graph_layers.0.bn.num_batches_tracked"):
        a, b = dev.state_dict()[k].double().cpu(), ref.state_dict()[k].double()
        assert rel(a, b) < 1e-3 if b.abs().max() > 0 else torch.equal(a, b), k
    assert float(ref.state_dict()["graph_layers.0.bn.running_mean"].abs().max()) > 0


def test_ganet_opt_out_and_split_precision():
    """hip_train = False on the same model and inputs: the stock module tree on the GPU, the same loss (as test_gpu_train.py does
    for vmgn). One 'bf16x3' step: the loss within the 1e-4 test_gpu_train.py allows the split mode. Non-fp32 frames are refused."""
    _, dev, x, adj, pids = build(False, "live")
    xd, ad, yd = x.to(DEV), adj.to(DEV), pids.to(DEV)
    sd = {k: v.clone() for k, v in dev.state_dict().items()}
    l1, _, _ = step(dev, xd, ad, yd, True)
    dev.load_state_dict(sd)
    dev.hip_train_precision = "bf16x3"
    l3, _, _ = step(dev, xd, ad, yd, True)
    dev.load_state_dict(sd)
    dev.hip_train_precision = "fp32"
    dev.hip_train = False
    l2, _, _ = step(dev, xd, ad, yd, True)
    print("ganet train step: native %.7f, stock on the GPU %.7f, bf16x3 %.7f" % (l1, l2, l3))
    assert abs(l1 - l2) < 1e-4 * abs(l2) and abs(l3 - l1) < 1e-4 * abs(l1)
    dev.hip_train = True
    with pytest.raises(TypeError, match="float32 frames"):
        dev(xd.double(), ad)
