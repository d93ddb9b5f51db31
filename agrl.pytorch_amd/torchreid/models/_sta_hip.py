"""MI355X execution of the eval forwards of the three baselines ``res50tp``, ``simple_sta`` and ``sta`` (reference
torchreid/models/res50tp.py:186-200, simple_sta.py:202-219, sta.py:206-243) through the C-ABI of libagrl_hip.so. Same stem, conv
kernels, data layout and host path as vmgn (``_resnet_hip``); what is specific:

    res50tp      gsta's route with no graph layers: the part means (splits [4]) out of layer 4's last conv where the pool-fused
                 epilogue applies (16-bit storage, 16 x 8 maps), else ``agrl_part_pool``; ``agrl_row_sqnorm`` +
                 ``agrl_attn_pool_bnneck`` with a zero global half. No kernel of its own.
    simple_sta   the same part means v_g (F,4,C) -- the 2048-channel map is never written where the fused pooling applies --,
                 ``agrl_sta_fuse`` in its norm mode (scores = channel norms of the part means, formed inside the kernel), then the head.
    sta          the attention map needs every channel of every pixel, so layer 4's last block stores its map; ``agrl_sta_frame_stats``
                 reads it ONCE for the part means and the attention partials, ``agrl_sta_fuse`` in its map mode, then the head.
    head         fc1 = Linear(4096, 1024, no bias) + eval BatchNorm1d + ReLU as ``agrl_linear_bn_relu`` (weight streamed once; fp32
                 weight in 'fp32' / 'bf16x3' / 'fp16x3', the 16-bit type in the 16-bit mode; x and all sums fp32).

The packs are cached on the model per (device, precision) under ``_resnet_hip``'s fingerprint rule. ``stages``: an optional dict that
receives v_g, t_a, idx, f_g (and the map's h, w) -- the selected frames are inspectable.
"""
from __future__ import annotations

import torch

from torchreid import hip_ops as ops
from torchreid import _hip
import torchreid.models._resnet_hip as R


def _pack_entries(model, pack, dtype, s16):
    """The tail's weights: ``bottleneck`` for res50tp, ``fc1`` for the STA pair."""
    if hasattr(model, 'fc1'):
        if not isinstance(model.fc1[2], torch.nn.ReLU):
            raise NotImplementedError('the HIP head is Linear + BatchNorm1d + ReLU; fc1 ends in {}'.format(type(model.fc1[2]).__name__))
        scale, shift = R.fold_bn1d(model.fc1[1])
        pack['fc'] = (R.own_copy(model.fc1[0].weight, dtype), scale, shift)
    else:
        pack['bnneck'] = R.single_bnneck(model.bottleneck)


def pack_weights(model, device, precision):
    """BN-fold + re-layout the trunk and the tail's weights; cached on the model (_resnet_hip.pack_weights)."""
    return R.pack_weights(model, device, precision, _pack_entries, type(model).__name__)


def _features(frames, pack, norm, pooled):
    """stem .. layer 4. ``pooled``: return the part means (F,4,C) fp32 -- out of the last conv's epilogue where that applies --
    else the NHWC map. -> (v_g or None, map or None, (h, w))"""
    lp = pack['dtype'] == ops.LP_DTYPE
    a = R.run_trunk(R.run_stem(frames, pack, norm), pack['trunk'])
    if pooled and lp and tuple(a.shape[1:3]) == (16, 8) and pack['l4'][0]['stride'] == 1:   # exactly 16 x 8 maps
        return R.run_layer4(a, pack['l4'], pool=([4], True)), None, (16, 8)
    a = R.run_layer4(a, pack['l4'])
    hw = (a.shape[1], a.shape[2])
    if not pooled:
        return None, a, hw
    _, v_g, _ = ops.part_pool(a, a, [4], want_lp=False)
    return v_g, None, hw


def hip_forward_res50tp(model, x, stages=None):
    """Eval forward of ``res50tp`` on the GPU: (B,S,3,H,W) fp32 (or uint8 frames, see _vmgn_hip.hip_forward) -> (B,2048) fp32. The
    attention tail kernel writes cat(BN(global), BN(attention)); only its second half exists for this model."""
    _hip.lib()
    frames, B, S, norm = R.eval_frames(model, x)
    pack = pack_weights(model, x.device, model.hip_precision)
    P = model.part
    with torch.no_grad(), ops.f32_split(model.hip_precision == 'bf16x3'):
        v_g, _, (h, w) = _features(frames, pack, norm, pooled=True)
        C = v_g.shape[-1]
        out = R.single_branch_tail(v_g.view(B, S * P, C), pack['bnneck'], B, S, P, h * w)
        if stages is not None:
            stages.update(v_g=v_g, hw=(h, w))
        return out


def hip_forward_sta(model, x, stages=None):
    """Eval forward of ``sta`` / ``simple_sta`` (``model.score`` = 'map' / 'norm') on the GPU: (B,S,3,H,W) fp32 (or uint8 frames)
    -> (B,1024) fp32."""
    _hip.lib()
    frames, B, S, norm = R.eval_frames(model, x)
    pack = pack_weights(model, x.device, model.hip_precision)
    with torch.no_grad(), ops.f32_split(model.hip_precision == 'bf16x3'):
        if model.score == 'map':
            _, fmap, (h, w) = _features(frames, pack, norm, pooled=False)
            v_g, nsum, nsq = ops.sta_frame_stats(fmap)
            del fmap
            f_g, t_a, idx = ops.sta_fuse(v_g, B, S, nsum, nsq, (h, w))
        else:
            v_g, _, (h, w) = _features(frames, pack, norm, pooled=True)
            f_g, t_a, idx = ops.sta_fuse(v_g, B, S)
        if stages is not None:
            stages.update(v_g=v_g, t_a=t_a, idx=idx, f_g=f_g, hw=(h, w))
        return ops.linear_bn_relu(f_g, pack['fc'][0], pack['fc'][1], pack['fc'][2])
