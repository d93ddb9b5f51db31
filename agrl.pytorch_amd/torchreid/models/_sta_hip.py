"""MI355X execution of the eval forwards of the three baselines ``res50tp``, ``simple_sta`` and ``sta`` (reference
torchreid/models/res50tp.py:186-200, simple_sta.py:202-219, sta.py:206-243) through the C-ABI of libagrl_hip.so. Same stem, conv
kernels and data layout as vmgn (``_vmgn_hip``); what is specific:

    res50tp      gsta's route with no graph layers: the part means (splits [4]) out of layer 4's last conv where the pool-fused
                 epilogue applies (16-bit storage, 16 x 8 maps), else ``agrl_part_pool``; ``agrl_row_sqnorm`` +
                 ``agrl_attn_pool_bnneck`` with a zero global half. No kernel of its own.
    simple_sta   the same part means v_g (F,4,C) -- the 2048-channel map is never written where the fused pooling applies --,
                 ``agrl_sta_fuse`` in its norm mode (scores = channel norms of the part means, formed inside the kernel), then the head.
    sta          the attention map needs every channel of every pixel, so layer 4's last block stores its map; ``agrl_sta_frame_stats``
                 reads it ONCE for the part means and the attention partials, ``agrl_sta_fuse`` in its map mode, then the head.
    head         fc1 = Linear(4096, 1024, no bias) + eval BatchNorm1d + ReLU as ``agrl_linear_bn_relu`` (weight streamed once; fp32
                 weight in 'fp32' / 'bf16x3' / 'fp16x3', the 16-bit type in the 16-bit mode; x and all sums fp32).

The packs are cached on the model per (device, precision) under ``_vmgn_hip``'s fingerprint rule. ``stages``: an optional dict that
receives v_g, t_a, idx, f_g (and the map's h, w) -- the selected frames are inspectable.
"""
from __future__ import annotations

import torch

from torchreid import hip_ops as ops
from torchreid import _hip
from torchreid.models._vmgn_hip import (_PRECISIONS, eval_frames, run_stem, _fingerprint, _fold_bn1d, _fold_conv_bn, _pack_stage, _run_block,
                                         _run_trunk, check_packed_range)


def pack_weights(model, device, precision):
    """BN-fold + re-layout the trunk and the tail's weights (``bottleneck`` for res50tp, ``fc1`` for the STA pair); cached on the model."""
    ops.check_precision(precision)
    key = (device.index if device.index is not None else torch.cuda.current_device(), precision)
    cached = model._hip_packs.get(key)
    if cached is not None and (model.hip_static_weights or cached['fingerprint'] == _fingerprint(model)):
        return cached
    first = next(model.parameters())
    if first.device != device:
        raise RuntimeError('model parameters live on {} but the input is on {}'.format(first.device, device))
    dtype = _PRECISIONS[precision]
    s16 = precision == 'fp16x3'
    with torch.no_grad():
        stem_w, stem_b = _fold_conv_bn(model.conv1, model.bn1, torch.float32)
        pack = {
            'dtype': dtype,
            'stem': (stem_w, stem_b),
            'stem_lp': ops.pack_stem_weights_lp16(stem_w) if dtype == ops.LP_DTYPE else None,
            'stem_s16': ops.pack_stem_weights_split16(stem_w) if s16 else None,
            'trunk': (_pack_stage(model.layer1, dtype, split16=s16) + _pack_stage(model.layer2, dtype, split16=s16)
                      + _pack_stage(model.layer3, dtype, seam=True, split16=s16)),
            'l4': _pack_stage(model.layer4, dtype, split16=s16),
        }
        if hasattr(model, 'fc1'):
            if not isinstance(model.fc1[2], torch.nn.ReLU):
                raise NotImplementedError('the HIP head is Linear + BatchNorm1d + ReLU; fc1 ends in {}'.format(type(model.fc1[2]).__name__))
            scale, shift = _fold_bn1d(model.fc1[1])
            pack['fc'] = (model.fc1[0].weight.detach().to(dtype).contiguous(), scale, shift)
        else:
            pack['bn'] = _fold_bn1d(model.bottleneck)
    if s16:
        for blk in pack['trunk'] + pack['l4']:   # the scaled fp32 copies were for packers this model does not use
            for name in ('c1', 'c2', 'c3', 'ds', 'dual16'):
                if blk.get(name) is not None and hasattr(blk[name][0], 'agrl_scaled'):
                    del blk[name][0].agrl_scaled
    if dtype == ops.LP_DTYPE:
        check_packed_range(pack, type(model).__name__)
    pack['fingerprint'] = _fingerprint(model)
    model._hip_packs[key] = pack
    return pack


def _features(frames, pack, norm, pooled):
    """stem .. layer 4. ``pooled``: return the part means (F,4,C) fp32 -- out of the last conv's epilogue where that applies --
    else the NHWC map. -> (v_g or None, map or None, (h, w))"""
    lp = pack['dtype'] == ops.LP_DTYPE
    a = run_stem(frames, pack, norm)
    a = _run_trunk(a, pack['trunk'])
    if pooled and lp and tuple(a.shape[1:3]) == (16, 8) and pack['l4'][0]['stride'] == 1:
        for blk in pack['l4'][:-1]:
            a = _run_block(a, blk)
        return _run_block(a, pack['l4'][-1], pool=([4], True)), None, (16, 8)
    for blk in pack['l4']:
        a = _run_block(a, blk)
    hw = (a.shape[1], a.shape[2])
    if not pooled:
        return None, a, hw
    _, v_g, _ = ops.part_pool(a, a, [4], want_lp=False)
    return v_g, None, hw


def hip_forward_res50tp(model, x, stages=None):
    """Eval forward of ``res50tp`` on the GPU: (B,S,3,H,W) fp32 (or uint8 frames, see _vmgn_hip.hip_forward) -> (B,2048) fp32. The
    attention tail kernel writes cat(BN(global), BN(attention)); only its second half exists for this model."""
    _hip.lib()
    frames, B, S, norm = eval_frames(model, x)
    pack = pack_weights(model, x.device, model.hip_precision)
    P = model.part
    with torch.no_grad(), ops.f32_split(model.hip_precision == 'bf16x3'):
        v_g, _, (h, w) = _features(frames, pack, norm, pooled=True)
        C = v_g.shape[-1]
        nodes = v_g.view(B, S * P, C)
        sqn = ops.row_sqnorm(nodes.view(B * S * P, C))
        gsum = torch.zeros((B * S, C), dtype=torch.float32, device=x.device)
        ident = (torch.ones_like(pack['bn'][0]), torch.zeros_like(pack['bn'][1]))
        out = ops.attn_pool_bnneck(nodes, sqn, gsum, ident[0], ident[1], pack['bn'][0], pack['bn'][1], B, S, P, h * w)
        if stages is not None:
            stages.update(v_g=v_g, hw=(h, w))
        return out[:, C:].contiguous()


def hip_forward_sta(model, x, stages=None):
    """Eval forward of ``sta`` / ``simple_sta`` (``model.score`` = 'map' / 'norm') on the GPU: (B,S,3,H,W) fp32 (or uint8 frames)
    -> (B,1024) fp32."""
    _hip.lib()
    frames, B, S, norm = eval_frames(model, x)
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
