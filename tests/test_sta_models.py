"""The three baselines ``res50tp``, ``simple_sta`` and ``sta`` on the CPU: this build's module trees and tests/sta_ref.py's float64
restatements against fixtures captured from the reference implementation itself (tests/golden/make_sta_golden.py). No GPU, no
reference needed at test time."""
import os

import numpy as np
import pytest
import torch

import sta_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = ("res50tp", "simple_sta", "sta")
# the keyword set the reference driver passes to EVERY architecture (train_vidreid_xent_htri.py:250-254, without save_dir)
DRIVER_KW = dict(num_classes=5, loss={"xent", "htri"}, last_stride=1, num_parts=3, num_scale=1, num_split=4, pyramid_part=True,
                 num_gb=2, use_pose=True, learn_graph=True, consistent_loss=False, bnneck=True)
_CACHE = {}


def gold(kind):
    return np.load(os.path.join(GOLD, kind + "_b2s4.npz"))


def close(a, b, tol):
    a, b = torch.as_tensor(np.asarray(a)).double(), torch.as_tensor(np.asarray(b)).double()
    err = ((a - b).abs().max() / b.abs().max().clamp(min=1e-30)).item()
    assert err < tol, err
    return err


def built(kind):
    """(model with the fixture's weights, fixture, state dict); built once per kind."""
    if kind not in _CACHE:
        from torchreid import models
        z = gold(kind)
        m = models.init_model(kind, **DRIVER_KW)
        calib = (float(z["fc1_mean"]), float(z["fc1_var"])) if "fc1_mean" in z.files else None
        sd = sta_ref.sta_state_dict(m.state_dict(), int(z["meta"][3]), calib=calib)
        m.load_state_dict(sd)
        _CACHE[kind] = (m, z, sd)
    return _CACHE[kind]


def test_registry_lists_all_six_names(tmp_path):
    from torchreid import models
    assert set(models.get_names()) == {"vmgn", "gsta", "ganet", "res50tp", "simple_sta", "sta"}
    # the driver's save_dir copy of the model definition (models/__init__.py) works for the new factories as well
    models.init_model("simple_sta", save_dir=str(tmp_path), **DRIVER_KW)
    assert os.path.isfile(os.path.join(str(tmp_path), "simple_sta.py"))


@pytest.mark.parametrize("kind", KINDS)
def test_state_dict_matches_reference(kind):
    m, z, _ = built(kind)
    own = m.state_dict()
    assert sorted(own.keys()) == list(z["keys"])
    assert [str(tuple(own[k].shape)) for k in sorted(own.keys())] == list(z["shapes"])
    if kind == "res50tp":
        assert not m.bottleneck.bias.requires_grad and m.classifier.bias is None and not hasattr(m, "fc1")
    else:
        assert "fc1.0.weight" in own and "fc1.1.running_var" in own and m.classifier.bias is not None and not hasattr(m, "bottleneck")
        assert isinstance(m.dropout, torch.nn.Dropout)
    for attr in ("hip_precision", "hip_static_weights", "_hip_packs", "pixel_mean", "pixel_std", "invalidate_hip_cache"):
        assert hasattr(m, attr), attr


@pytest.mark.parametrize("kind", KINDS)
def test_eval_and_train_outputs_match_reference(kind):
    m, z, sd = built(kind)
    B, S, seed, _, train_off = [int(v) for v in z["meta"]]
    x = sta_ref.sta_clips(B, S, seed)
    m.eval()
    with torch.no_grad():
        out = m(x, None)
        close(out, z["out"], 1e-5)
        assert torch.equal(out, m(x))                       # the adjacency is optional and ignored
        # the float64 restatement of the tail, on this build's layer-4 map
        r = sta_ref.tail_ref(kind, m.featuremaps(x.view(B * S, 3, 256, 128)), B, S, sd)
    close(r["out"], z["out"], 1e-5)
    close(r["t_a"], z["t_a"], 1e-5)
    if kind == "res50tp":
        close(r["f"], z["f"], 1e-5)
    else:
        assert float(z["gaps"].min()) >= 1e-3               # the generator's selection rule
        assert np.array_equal(r["idx"].numpy(), z["idx"])
        close(r["f_g"], z["f_g"], 1e-5)
        f_g, t_a, idx = m.fused_feature(x)
        assert np.array_equal(idx.numpy(), z["idx"])
        close(f_g.detach(), z["f_g"], 1e-5)
        close(t_a.detach(), z["t_a"], 1e-5)
        # the fixture's output sees the input: not relu(BatchNorm shift)
        assert 0.3 < float((z["out"] != 0).mean()) < 0.7 and float(np.abs(z["out"][0] - z["out"][1]).max()) > 0.1
    m.train()
    y, f = m(sta_ref.sta_clips(2, 8, seed + train_off), None)
    close(y.detach(), z["train_logits"], 1e-4)
    close(f.detach(), z["train_feats"], 1e-4)
    m.loss = {"xent"}
    y1 = m(sta_ref.sta_clips(2, 8, seed + train_off))
    assert torch.is_tensor(y1) and tuple(y1.shape) == (2, 5)
    m.loss = {"htri"}
    with pytest.raises(KeyError):
        m(sta_ref.sta_clips(2, 2, 1, H=64, W=32))
    m.loss = {"xent", "htri"}
    m.eval()


@pytest.mark.parametrize("kind", KINDS)
def test_pretrained_flag_never_touches_the_network(kind, monkeypatch):
    from torch.utils import model_zoo
    from torchreid import models

    def boom(*a, **k):
        raise AssertionError("the factory tried to download weights")

    monkeypatch.delenv("AGRL_PRETRAINED_RESNET50", raising=False)
    monkeypatch.setattr(model_zoo, "load_url", boom)
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", boom)
    flag = "pretrain" if kind == "res50tp" else "pretrained"
    m = models.init_model(kind, **dict(DRIVER_KW, **{flag: True}))
    assert next(m.parameters()).numel() > 0


def test_pretrained_flag_honours_the_local_checkpoint(tmp_path, monkeypatch):
    """AGRL_PRETRAINED_RESNET50 exactly as gsta() reads it: matching keys / shapes are taken, the rest is left alone."""
    from torchreid import models
    ckpt = {"bn1.weight": torch.full((64,), 3.0), "fc.weight": torch.zeros(1000, 2048), "conv1.weight": torch.zeros(1, 1)}
    path = os.path.join(str(tmp_path), "resnet50.pth")
    torch.save(ckpt, path)
    monkeypatch.setenv("AGRL_PRETRAINED_RESNET50", path)
    for kind, flag in (("res50tp", "pretrain"), ("simple_sta", "pretrained"), ("sta", "pretrained")):
        m = models.init_model(kind, **dict(DRIVER_KW, **{flag: True}))
        assert float(m.bn1.weight.detach().min()) == 3.0 and tuple(m.conv1.weight.shape) == (64, 3, 7, 7)
        m = models.init_model(kind, **dict(DRIVER_KW, **{flag: False}))
        assert float(m.bn1.weight.detach().max()) == 1.0


def test_uint8_frames_on_the_cpu_are_normalised_first():
    from torchreid import hip_ops as ops
    m, _, _ = built("sta")
    m.eval()
    u8 = sta_ref.clips_u8(sta_ref.sta_clips(1, 2, 3, H=64, W=32))
    with torch.no_grad():
        assert torch.equal(m(u8), m(ops.clips_to_float(u8, m.pixel_mean, m.pixel_std)))


def test_unknown_precision_fails_at_construction(monkeypatch):
    from torchreid import models
    monkeypatch.setenv("AGRL_HIP_PRECISION", "fp8")
    with pytest.raises(Exception):
        models.init_model("sta", **DRIVER_KW)
