"""uint8 frames on the CPU: the normalisation table is the reference's ToTensor + Normalize bit for bit, the three models take uint8
clips in either layout and give exactly what they give for the table-normalised fp32 tensor, and the new attributes stay out of
the state dict. The GPU half (the kernels that fuse the table into the stem) is tests/test_gpu_u8_ingest.py."""
import numpy as np
import pytest
import torch

from recipe import recipe_state_dict, synthetic_adj

KW = dict(num_classes=5, loss={"xent", "htri"}, last_stride=1, num_split=4, num_gb=2, num_scale=1, pyramid_part=True,
          use_pose=True, learn_graph=True)
MODELS = {"vmgn": {}, "gsta": dict(pretrained=False), "ganet": dict(knn=4, pretrained=False)}
OTHER = ((0.41, 0.5, 0.37), (0.31, 0.2, 0.27))   # a non-default mean / std


def build(name):
    from torchreid import models
    m = models.init_model(name, **dict(KW, **MODELS[name]))
    m.load_state_dict(recipe_state_dict(m.state_dict(), seed=0))
    return m.eval()


def torch_transform(u8_nchw, mean, std):
    """F.to_tensor (uint8 -> float, div(255)) + F.normalize (sub_(mean), div_(std)) as torchvision writes them."""
    m = torch.as_tensor(mean, dtype=torch.float32).view(1, 3, 1, 1)
    s = torch.as_tensor(std, dtype=torch.float32).view(1, 3, 1, 1)
    return u8_nchw.to(torch.float32).div(255).sub_(m).div_(s)


@pytest.mark.parametrize("norm", [None, OTHER])
def test_frame_table_is_to_tensor_and_normalize_bit_for_bit(norm):
    from torchreid import hip_ops as ops
    mean, std = norm if norm is not None else (ops.PIXEL_MEAN, ops.PIXEL_STD)
    T = ops.frame_table(mean, std) if norm is not None else ops.frame_table()
    assert T.shape == (3, 256) and T.dtype == torch.float32 and not T.is_cuda
    # every byte value in every channel through the torchvision expression
    u = torch.arange(256, dtype=torch.uint8).view(1, 1, 256, 1).expand(1, 3, 256, 1).contiguous()
    assert torch.equal(T, torch_transform(u, mean, std).view(3, 256))
    # the stepwise numpy evaluation: correctly rounded fp32 operations on fp32-rounded constants
    m32, s32 = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
    v = np.arange(256, dtype=np.float32)
    step = np.stack([((v / np.float32(255)) - m32[c]) / s32[c] for c in range(3)])
    assert step.dtype == np.float32 and np.array_equal(T.numpy(), step)
    # random images, both layouts, through the table lookup the CPU paths use
    img = torch.randint(0, 256, (4, 3, 256, 128), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    ref = torch_transform(img, mean, std)
    assert torch.equal(ops.frames_normalize_reference(img, mean, std), ref)
    assert torch.equal(ops.frames_normalize_reference(img.permute(0, 2, 3, 1).contiguous(), mean, std), ref)
    if norm is None:
        assert len(torch.unique(T.to(torch.float16), dim=1)[0]) == 256   # distinct after rounding to fp16
        assert -2.118 < T.min().item() and T.max().item() < 2.6401


@pytest.mark.parametrize("name", sorted(MODELS))
def test_models_take_uint8_clips_in_both_layouts_on_the_cpu(name):
    from torchreid import hip_ops as ops
    m = build(name)
    B, S, H, W = 2, 4, 64, 32
    u8 = torch.randint(0, 256, (B, S, 3, H, W), dtype=torch.uint8, generator=torch.Generator().manual_seed(7))
    adj = synthetic_adj(B, S, seed=1)
    x32 = ops.frames_normalize_reference(u8)
    assert x32.shape == (B, S, 3, H, W) and x32.dtype == torch.float32
    with torch.no_grad():
        ref = m(x32, adj)
        first = m(u8, adj)
        last = m(u8.permute(0, 1, 3, 4, 2).contiguous(), adj)
        assert torch.isfinite(ref).all() and torch.equal(first, ref) and torch.equal(last, ref)
        # the attributes are what is applied
        m.pixel_mean, m.pixel_std = OTHER
        assert torch.equal(m(u8, adj), m(ops.frames_normalize_reference(u8, *OTHER), adj)) and not torch.equal(m(u8, adj), ref)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_pixel_constants_are_plain_attributes(name):
    m = build(name)
    assert tuple(m.pixel_mean) == (0.485, 0.456, 0.406) and tuple(m.pixel_std) == (0.229, 0.224, 0.225)
    keys = list(m.state_dict().keys())
    assert not [k for k in keys if "pixel" in k]
    assert not [k for k, _ in m.named_parameters() if "pixel" in k] and not [k for k, _ in m.named_buffers() if "pixel" in k]
    if name == "vmgn":
        assert len(keys) == 402


@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("shape", [(2, 4, 4, 16, 8), (2, 4, 16, 8, 4), (8, 3, 16, 8), (2, 4, 1, 16, 8), (1, 2, 4, 3, 16, 8)])
def test_bad_uint8_shapes_raise_value_error(name, shape):
    m = build(name)
    with pytest.raises(ValueError):
        m(torch.zeros(shape, dtype=torch.uint8), synthetic_adj(2, 4, seed=1))


@pytest.mark.parametrize("name", sorted(MODELS))
def test_eval_forwards_check_shape_and_dtype_before_any_launch(name):
    """The GPU eval forwards validate the frames before they touch the device, so this half runs here: a uint8 tensor in neither layout
    is a ValueError, and any dtype other than float32 / uint8 is still the TypeError it was."""
    from torchreid.models import _ganet_hip, _vmgn_hip
    fwd = {"vmgn": _vmgn_hip.hip_forward, "gsta": _vmgn_hip.hip_forward_gsta, "ganet": _ganet_hip.hip_forward_ganet}[name]
    m = build(name)
    adj = synthetic_adj(2, 4, seed=1)
    for dtype in (torch.int16, torch.float64, torch.float16, torch.int8):
        with pytest.raises(TypeError, match="frames must be float32"):
            fwd(m, torch.zeros((2, 4, 3, 64, 32), dtype=dtype), adj)
    for shape in ((2, 4, 4, 64, 32), (8, 3, 64, 32), (2, 4, 64, 32, 4)):
        with pytest.raises(ValueError):
            fwd(m, torch.zeros(shape, dtype=torch.uint8), adj)
