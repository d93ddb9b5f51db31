"""The ResNet-50 host path all six models share, above the C-ABI of libagrl_hip.so: BatchNorm folding and weight re-layout, the one
pack cache, the stem, the layer1..layer3 runner, the Bottleneck runners, the layer-4 runner and the single-branch attention tail.
A model's own file (``_vmgn_hip``: vmgn and gsta, ``_ganet_hip``, ``_sta_hip``) adds its pack entries and what follows layer 4.

Data layout in HBM
    frames        fp32 NCHW (B*S,3,H,W)  as handed over by the driver (read once by the stem kernel); or uint8, (B*S,3,H,W) / (B*S,H,W,3)
    activations   NHWC (B*S, h, w, C) in the compute dtype (fp32 parity mode / bf16 throughput mode)
    conv weights  OHWI (Cout, R, S, Cin), eval BatchNorm folded in, compute dtype; bias fp32

The packed weights are cached per (device, precision) and rebuilt when any parameter / buffer changed
(data pointer or in-place version), unless ``model.hip_static_weights`` is set. The library's own writers of these tensors -- the
native optimiser steps, the train-mode BatchNorm -- bump the versions themselves (hip_ops.written); a pack entry never aliases a
parameter (own_copy).
"""
from __future__ import annotations

import os

import torch

from torchreid import hip_ops as ops

# 'bf16x3': fp32 tensors and layouts of the parity mode, conv / Linear products as three bf16 MFMAs (hip_ops.f32_split)
# 'fp16x3' (round 6): the same fp32 tensors, conv products and the GraphLayer's Linear as three FP16 MFMAs on fp16 high / low halves (22 bits
# per operand), their weights pre-scaled by a power of two and pre-split at pack time (ops.split16_inloop_weights); graph matrix, pooling
# and attention tail: exact fp32 (the distance matrix of this mode: metrics.distance.hip_distmat_device)
PRECISIONS = {'fp32': torch.float32, ops.LP_NAME: ops.LP_DTYPE, 'bf16x3': torch.float32, 'fp16x3': torch.float32}   # ops.LP_NAME: 'fp16' (default build) or 'bf16'


def init_hip_attributes(model, train=False, train_tail=False):
    """The MI355X path's configuration of a model, set by its constructor. Plain attributes: not parameters, not buffers, not in the
    state dict. ``train`` / ``train_tail``: the model has a native train step / a switch for the tail of it."""
    model.hip_precision = os.environ.get('AGRL_HIP_PRECISION', 'fp32')
    ops.check_precision(model.hip_precision)   # a precision the loaded library cannot serve fails HERE, not at the first forward
    model.hip_static_weights = False
    if train:
        model.hip_train = os.environ.get('AGRL_HIP_TRAIN', '1') != '0'   # train-mode forward + backward on the HIP kernels
        model.hip_train_precision = os.environ.get('AGRL_HIP_TRAIN_PRECISION', 'fp32')   # 'fp32' exact | 'bf16x3' split-bf16 MFMA
    if train_tail:
        model.hip_train_tail = os.environ.get('AGRL_HIP_TRAIN_TAIL', '1') != '0'   # tail of the train forward native as well
    model._hip_packs = {}
    # uint8 frames (B,S,3,H,W) / (B,S,H,W,3) are normalised with these -- the reference's transform_test -- inside the stem kernels
    # (GPU eval) or in front of the path (training, CPU)
    model.pixel_mean = (0.485, 0.456, 0.406)
    model.pixel_std = (0.229, 0.224, 0.225)


def fold_conv_bn(conv, bn, dtype, split16=False):
    """conv (no bias) followed by eval BatchNorm2d -> (OHWI weight in dtype, fp32 bias). ``split16``: the fp32 weight pre-scaled by a
    power of two and pre-split for the split-fp16 convolution (ops.split16_inloop_weights; the un-scaling factor rides on the tensor)."""
    w = conv.weight.detach().float()
    scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
    shift = bn.bias.detach().float() - bn.running_mean.detach().float() * scale
    w = (w * scale.view(-1, 1, 1, 1)).permute(0, 2, 3, 1).contiguous()
    if split16:
        assert dtype == torch.float32
        return ops.split16_inloop_weights(w), shift.contiguous()
    return w.to(dtype).contiguous(), shift.contiguous()


def own_copy(param, dtype):
    """A parameter as ``dtype`` for a pack, in memory of the pack's own. ``.to(dtype)`` and ``.contiguous()`` hand back the parameter's
    storage where they have nothing to do (fp32 modes): a pack entry made with them alone follows a raw write of the parameter while
    the folded entries beside it do not -- under ``hip_static_weights`` a forward on half-stepped weights."""
    return param.detach().to(dtype, copy=True).contiguous()


def fold_bn1d(bn):
    scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
    shift = bn.bias.detach().float() - bn.running_mean.detach().float() * scale
    return scale.contiguous(), shift.contiguous()


def check_packed_range(pack, where="vmgn"):
    """BatchNorm-folded weights are cast to the library's 16-bit type at pack time: with fp16 a checkpoint with a tiny
    running_var or a large gamma can fold to inf (|w| > 65504). Checked once per pack, with the layer named -- the end-of-
    extraction check would blame the activations."""
    def walk(obj, path):
        if torch.is_tensor(obj):
            if obj.dtype == ops.LP_DTYPE and obj.numel() and not bool(torch.isfinite(obj).all()):
                raise FloatingPointError("%s: the BatchNorm-folded weights of %s overflow %s (abs-max of the fp32 fold is beyond its "
                                         "range): load the bf16 build (AGRL_HIP_LP16=bf16) or use hip_precision='fp32'" % (where, path, ops.LP_NAME))
        elif isinstance(obj, dict):
            for k, v in obj.items():
                walk(v, "%s.%s" % (path, k))
        elif isinstance(obj, (list, tuple)):
            for i, v in enumerate(obj):
                walk(v, "%s[%d]" % (path, i))
    walk({k: v for k, v in pack.items() if k != 'fingerprint'}, "pack")


def pack_tensors(obj):
    """every tensor of a pack (dicts, lists and tuples walked)"""
    if torch.is_tensor(obj):
        yield obj
    elif isinstance(obj, (dict, list, tuple)):
        for v in (obj.values() if isinstance(obj, dict) else obj):
            yield from pack_tensors(v)


def dual_weights(blk, wd=None, w3=None):
    """conv3 + downsample of a block as ONE GEMM over the concatenated K axis: ([w_ds | w3] (Cout, Kd + K3), b_ds + b3). ``wd`` / ``w3``:
    other forms of the block's two weights (the fp16x3 packers pass the true, un-scaled ones)."""
    wd, w3 = blk['ds'][0] if wd is None else wd, blk['c3'][0] if w3 is None else w3
    cout = w3.shape[0]
    return torch.cat([wd.view(cout, -1), w3.view(cout, -1)], dim=1).contiguous(), (blk['ds'][1] + blk['c3'][1]).contiguous()


def pack_stage(stage, dtype, seam=False, split16=False):
    blocks = []
    for unit in stage:
        blk = {
            'c1': fold_conv_bn(unit.conv1, unit.bn1, dtype, split16),
            'c2': fold_conv_bn(unit.conv2, unit.bn2, dtype, split16),
            'c3': fold_conv_bn(unit.conv3, unit.bn3, dtype, split16),
            'stride': unit.conv2.stride[0],
            'ds': None,
        }
        if unit.downsample is not None:
            blk['ds'] = fold_conv_bn(unit.downsample[0], unit.downsample[1], dtype, split16)
            blk['ds_stride'] = unit.downsample[0].stride[0]
            if split16 and blk['ds_stride'] == blk['stride'] and blk['ds'][0].shape[3] % 32 == 0 and blk['c3'][0].shape[3] % 32 == 0:
                # conforming mode: conv3 + downsample as ONE in-loop split GEMM over [block input sampled at the stride | conv2's output]
                # (ops.conv1x1_dual_split16): the fp32 shortcut map -- 537 MB written and read back in layer 1 -- no longer exists
                w, b = dual_weights(blk, ops.split16_true_weights(blk['ds'][0]), ops.split16_true_weights(blk['c3'][0]))
                blk['dual16'] = (ops.split16_inloop_weights(w), b)
            if dtype == ops.LP_DTYPE and blk['ds_stride'] == 1 and blk['stride'] == 1:
                # conv3 + downsample as ONE GEMM over the concatenated K axis (ops.conv1x1_dual): [w_ds | w3], b_ds + b3
                blk['dual'] = dual_weights(blk)
                if (ops.conv1x1_packed_supported(blk['dual'][0]) and blk['dual'][0].shape[1] >= 1536
                        and blk['ds'][0].shape[3] % 128 == 0 and blk['c3'][0].shape[3] % 128 == 0):   # K1, K2 % 128 each
                    blk['dualp'] = ops.conv1x1_pack(blk['dual'][0])     # the same GEMM through the four-wave kernel
            if dtype == ops.LP_DTYPE and blk['ds_stride'] > 1 and blk['ds_stride'] == blk['stride']:
                # first block of layers 2 / 3: the same one-GEMM form with the block input sampled at the stride (ops.conv1x1_packed_dual_strided)
                dual_w, dual_b = dual_weights(blk)
                if (ops.conv1x1_packed_supported(dual_w) and blk['ds'][0].shape[3] % 128 == 0 and blk['c3'][0].shape[3] % 128 == 0):
                    blk['dualps'] = ops.conv1x1_pack(dual_w)
                    blk['dualps_bias'] = dual_b
        if dtype == ops.LP_DTYPE and ops.conv1x1_packed_supported(blk['c1'][0]) and blk['c1'][0].shape[3] >= 1024:
            # layer 4's 2048 -> 512 / 1024 -> 512 convs: the shapes where the packed-weight kernels are ahead of the 8-wave tile
            # (_conv1: ops.conv1x1_packed_res without a residual)
            blk['c1p'] = ops.conv1x1_pack(blk['c1'][0])
        if (dtype == ops.LP_DTYPE and blk['ds'] is None and ops.conv1x1_packed_supported(blk['c3'][0])
                and blk['c3'][0].shape[0] >= 2048):
            # the pool-fused last conv of a layer-4 branch (512 -> 2048 + identity shortcut): two workgroups per CU (ops.conv1x1_packed_res_pool)
            blk['c3p'] = ops.conv1x1_pack(blk['c3'][0])
        if dtype == ops.LP_DTYPE and blk['stride'] == 1 and ops.conv3x3_packed_supported(blk['c2'][0]):
            # layers 3 / 4: the 3x3 weights as per-wave fragment streams for the four-wave kernel (ops.conv3x3_packed)
            blk['c2p'] = ops.conv3x3_pack(blk['c2'][0])
        blocks.append(blk)
    if seam and dtype == ops.LP_DTYPE:
        # conv3 + residual of block i back to back with conv1 of block i + 1 (ops.bottleneck_seam, layer 3): the two static
        # weight matrices re-ordered once into the fragment streams the kernel's waves load straight into registers
        for blk, nxt in zip(blocks[:-1], blocks[1:]):
            if ops.bottleneck_seam_supported(blk['c3'][0], nxt['c1'][0]):
                blk['seam'] = ops.bottleneck_seam_pack(blk['c3'][0], nxt['c1'][0])
                blk['seam_dims'] = (blk['c3'][0].shape[3], blk['c3'][0].shape[0], nxt['c1'][0].shape[0])
                blk['seam_b1n'] = nxt['c1'][1]
        # runs of consecutive blocks that one ops.bottleneck_chain launch can take (layer 3's blocks 1-4): the first block of a run
        # carries the run's device table of per-block pointers, built here once (it lives and dies with the pack)
        i = 0
        while i < len(blocks):
            run = chain_run(blocks, i)
            if run:
                blocks[i]['chain'] = (run, ops.bottleneck_chain_table(blocks[i:i + run]))
            i += max(run, 1)
    return blocks


def chain_run(blocks, i):
    """Length of the run of consecutive blocks from ``i`` on that ops.bottleneck_chain can take in one launch (0: none)."""
    n = 0
    while i + n < len(blocks) and n < ops.CHAIN_MAX and ops.bottleneck_chain_block_ok(blocks[i + n]):
        n += 1
    return n


def pack_planes(blk):
    """The split-fp16 plane operands of one Bottleneck (blk: fp32 folded weights, pre-scaled for the in-loop split) -> blk['p3'];
    False when a shape does not fit the four-wave kernels (the caller then keeps the whole model on the in-loop split).
    The block's input and output -- the wide tensors the 1x1 kernels are HBM-bound on -- are plane PAIRS [hi | lo 2^11]
    (the third plane repeats the first: ops.split16_plane_weights(pair_first=True)); conv1's and conv2's outputs are triples."""
    def true_w(pair):
        return ops.split16_true_weights(pair[0])    # undo the per-tensor pre-scale (exact)

    w1, w2, w3 = true_w(blk['c1']), true_w(blk['c2']), true_w(blk['c3'])
    K1, K3c, mid, cout = w1.shape[3], w3.shape[3], w1.shape[0], w3.shape[0]
    if blk['stride'] != 1 or mid % 256 or cout % 256 or K1 % 128 or K3c % 128 or tuple(w2.shape[1:3]) != (3, 3) or w2.shape[3] % 64:
        return False
    p3 = {}
    t, u = ops.split16_plane_weights(w1.view(mid, K1), pair_first=True)
    p3['c1'] = (ops.conv1x1_pack(t), u, blk['c1'][1], mid)
    t, u = ops.split16_plane_weights(w2)
    p3['c2'] = (ops.conv3x3_pack(t), u, blk['c2'][1], w2.shape[0])
    if blk['ds'] is not None:
        if blk['ds_stride'] != 1:
            return False
        wd = true_w(blk['ds'])
        Kd = wd.shape[3]
        if Kd % 128:
            return False
        w, b = dual_weights(blk, wd, w3)
        t, u = ops.split16_plane_weights(w, segments=[Kd, K3c], pair_first=True)
        p3['dual'] = (ops.conv1x1_pack(t), u, b, cout)
    else:
        t, u = ops.split16_plane_weights(w3.view(cout, K3c))
        p3['c3'] = (ops.conv1x1_pack(t), u, blk['c3'][1], cout)
    blk['p3'] = p3
    return True


def fingerprint(model):
    return tuple((t.data_ptr(), t._version) for t in list(model.parameters()) + list(model.buffers()))


def pack_weights(model, device, precision, entries, where):
    """The one pack cache: BN-fold + re-layout every weight of ``model``'s eval forward for ``device``, cached on the model per
    (device, precision). Packs the stem, layer1..layer3 (pack['trunk']) and layer 4 (pack['l4'], or 'l4_1' / 'l4_2' for a model with two
    branches); ``entries(model, pack, dtype, split16)`` adds the model's own entries; then the finish every model gets: the fp16x3
    attribute check, the plane packs of a two-branch model, no fp32 ``agrl_scaled`` copy kept, the 16-bit range check (``where`` names the
    model in its message), the fingerprint."""
    ops.check_precision(precision)
    key = (device.index if device.index is not None else torch.cuda.current_device(), precision)
    cached = model._hip_packs.get(key)
    if cached is not None and (model.hip_static_weights or cached['fingerprint'] == fingerprint(model)):
        return cached
    first = next(model.parameters())
    if first.device != device:
        raise RuntimeError('model parameters live on {} but the input is on {}'.format(first.device, device))
    dtype = PRECISIONS[precision]
    s16 = precision == 'fp16x3'
    two = hasattr(model, 'layer4_1')   # vmgn: two layer4 branches
    with torch.no_grad():
        stem_w, stem_b = fold_conv_bn(model.conv1, model.bn1, torch.float32)
        pack = {
            'dtype': dtype,
            'stem': (stem_w, stem_b),
            'stem_lp': ops.pack_stem_weights_lp16(stem_w) if dtype == ops.LP_DTYPE else None,
            'stem_s16': ops.pack_stem_weights_split16(stem_w) if s16 else None,   # conforming mode: the stem in split-fp16 arithmetic
            'trunk': pack_stage(model.layer1, dtype, split16=s16) + pack_stage(model.layer2, dtype, split16=s16) + pack_stage(model.layer3, dtype, seam=True, split16=s16),
        }
        for name in (('l4_1', 'l4_2') if two else ('l4',)):
            pack[name] = pack_stage(getattr(model, 'layer4' + name[2:]), dtype, split16=s16)
        stages = pack['trunk'] + (pack['l4_1'] + pack['l4_2'] if two else pack['l4'])
        entries(model, pack, dtype, s16)
        if s16:
            # the un-scaling factor rides on the weight TENSOR OBJECT (ops.split16_inloop_weights): a copy made behind its back (.to / .contiguous /
            # .clone) would silently run as a 2^k-times-too-large exact-fp32 weight -- checked once per pack
            for blk in stages:
                for name in ('c1', 'c2', 'c3', 'ds'):
                    if blk.get(name) is not None and not (hasattr(blk[name][0], 'agrl_unscale') and getattr(blk[name][0], 'agrl_presplit', False)):
                        raise RuntimeError("fp16x3 pack: %s lost its pre-scale attributes" % name)
            if two and ops.split16_planes_available():
                # the conforming mode at speed: behind layer 3's first block every Bottleneck runs on split-fp16 PLANES through the throughput
                # mode's four-wave kernels (ops.conv1x1_split16 / conv3x3_split16); the stem .. layer 3's first block keep fp32 tensors and the
                # in-loop split (agrl_conv2d_bn_act_split16)
                first = len(model.layer1) + len(model.layer2) + 1
                pack['planes_from'] = first if all(pack_planes(blk) for blk in stages[first:]) else None
            for t in pack_tensors(pack):   # the scaled fp32 copies were for the packers above
                if hasattr(t, 'agrl_scaled'):
                    del t.agrl_scaled
    if dtype == ops.LP_DTYPE:
        check_packed_range(pack, where)
    pack['fingerprint'] = fingerprint(model)
    model._hip_packs[key] = pack
    return pack


def run_block_planes(x3, blk, pool=None):
    """One Bottleneck on split-fp16 planes (x3: (F,h,w,2 C) fp16 = the pair [hi | lo 2^11]; the result is a pair as well); ``pool`` =
    (splits, mean): the frame pooling in the last conv's epilogue, returns the pooled fp32 tensor instead of the map. vmgn.py:45-65."""
    p3 = blk['p3']
    xp, rop = 1, 2   # layout bits: x3 is a pair / residual and result are pairs
    y = ops.conv1x1_split16(x3, p3['c1'][0], p3['c1'][1], p3['c1'][2], p3['c1'][3], layout=xp)
    y = ops.conv3x3_split16(y, p3['c2'][0], p3['c2'][1], p3['c2'][2], p3['c2'][3])
    if 'dual' in p3:
        assert pool is None
        d = p3['dual']
        return ops.conv1x1_split16(x3, d[0], d[1], d[2], d[3], x2=y, layout=xp | rop)
    c = p3['c3']
    if pool is not None:
        return ops.conv1x1_split16_pool(y, c[0], c[1], c[2], c[3], x3, pool[0], pool[1], layout=rop)
    return ops.conv1x1_split16(y, c[0], c[1], c[2], c[3], residual3=x3, layout=rop)


def _conv2(y, blk):
    """conv2 / bn2 / relu of a Bottleneck (vmgn.py:52-54): the packed-weight kernel where it was packed and the map is made of
    whole 16 x 8 blocks, else the general conv."""
    if 'c2p' in blk and y.shape[1] % 16 == 0 and y.shape[2] % 8 == 0:
        return ops.conv3x3_packed(y, blk['c2p'], blk['c2'][1], blk['c2'][0].shape[0], True)
    return ops.conv_bn_act(y, blk['c2'][0], blk['c2'][1], blk['stride'], 1, True)


def _conv1(x, blk):
    """conv1 / bn1 / relu of a Bottleneck (vmgn.py:48-50)."""
    # (layer 4's conv1s through conv1x1_duo_kernel: ahead back to back -- 2048 -> 512 69 us against 73 --; inside the step it measured equal
    # in the middle of round 5 and, on the final tree, 7-13 us ahead per step on two boxes (eight A/B pairs, profiles/r05_ab_conv1_through_duo.txt))
    if 'c1p' in blk and x.is_contiguous():
        return ops.conv1x1_packed_res(x, blk['c1p'], blk['c1'][1], blk['c1'][0].shape[0], None, True)
    return ops.conv_bn_act(x, blk['c1'][0], blk['c1'][1], 1, 0, True)


def shortcut(x, blk):
    """A Bottleneck's shortcut operand: its input, or the downsample conv / bn of it (vmgn.py:60-61)."""
    return x if blk['ds'] is None else ops.conv_bn_act(x, blk['ds'][0], blk['ds'][1], blk['ds_stride'], 0, False)


def run_block_inloop(x, blk, out_planes=0):
    """One Bottleneck of the conforming mode on fp32 tensors (weights from ops.split16_inloop_weights): conv1's and conv2's outputs are read
    by one GEMM each and never as numbers, so they are stored with their fp16 halves already formed -- the 3x3 conv's k-loop has no
    VALU work left (bit-identical to splitting in the loop)."""
    y = ops.conv_bn_act(x, blk['c1'][0], blk['c1'][1], 1, 0, True, out_presplit=True)
    y = ops.conv_bn_act(y, blk['c2'][0], blk['c2'][1], blk['stride'], 1, True, x_presplit=True, out_presplit=True)
    if 'dual16' in blk and x.is_contiguous():
        # conv3 + the downsample conv as ONE GEMM over [x sampled at the stride | y]: no shortcut map in HBM
        # (``out_planes``: the last block in front of the plane kernels writes their input layout itself)
        return ops.conv1x1_dual_split16(x, y, blk['dual16'][0], blk['dual16'][1], blk['stride'], True, x2_presplit=True, out_planes=out_planes)
    out = ops.conv_bn_act(y, blk['c3'][0], blk['c3'][1], 1, 0, True, residual=shortcut(x, blk), x_presplit=True)
    return ops.to_split16_planes(out, out_planes) if out_planes else out


def is_inloop(blk):
    return getattr(blk['c1'][0], 'agrl_presplit', False)


def run_trunk(a, blocks):
    """layer1..layer3 Bottlenecks. Where the fused kernel exists (layer 1, bf16) the last conv of block i also
    produces the first conv of block i+1 from the tile it still holds in LDS (ops.bottleneck_tail)."""
    z = None  # conv1 output of the current block, when the previous block's tail already computed it
    skip = 0  # blocks a chain launch has already run
    for i, blk in enumerate(blocks):
        if skip:
            skip -= 1
            continue
        if is_inloop(blk):
            a = run_block_inloop(a, blk)
            continue
        nxt = blocks[i + 1] if i + 1 < len(blocks) else None
        y = z if z is not None else ops.conv_bn_act(a, blk['c1'][0], blk['c1'][1], 1, 0, True)
        if 'chain' in blk and ops.bottleneck_chain_supported(y, a, blocks[i:i + blk['chain'][0]]):
            # layer 3's blocks 1-4: 3x3 + conv3 + residual + next conv1 of the whole run in ONE launch, a frame per workgroup
            # (ops.bottleneck_chain); z is then the conv1 output of the block behind the run
            n, table = blk['chain']
            a, z = ops.bottleneck_chain(y, a, table, n)
            skip = n - 1
            continue
        if nxt is not None:
            # layer 1: 3x3 + conv3 (+ shortcut) + next conv1 in ONE pass over 8 x 8 pixel tiles (ops.bottleneck_block)
            ds = None if blk['ds'] is None else (blk['ds'][0], blk['ds_stride'])
            if ops.bottleneck_block_supported(y, blk['c2'][0], blk['stride'], blk['c3'][0], nxt['c1'][0], ds) and (
                    ds is None or a.shape[3] == 64):
                if ds is None:
                    a, z = ops.bottleneck_block(y, blk['c2'][0], blk['c2'][1], blk['c3'][0], blk['c3'][1], a,
                                                nxt['c1'][0], nxt['c1'][1])
                else:
                    a, z = ops.bottleneck_block(y, blk['c2'][0], blk['c2'][1], blk['c3'][0], blk['c3'][1], None,
                                                nxt['c1'][0], nxt['c1'][1], shortcut=(a, blk['ds'][0], blk['ds'][1]))
                continue
        y = _conv2(y, blk)
        fusable = nxt is not None and ops.bottleneck_tail_supported(y, blk['c3'][0], nxt['c1'][0])
        if fusable and blk['ds'] is not None and ops.bottleneck_tail_supported(
                y, blk['c3'][0], nxt['c1'][0], (blk['ds'][0], blk['ds_stride'])) and a.shape[3] == 64:
            # first block of layer 1: the downsample conv rides along as a second k-tile (no shortcut map in HBM)
            a, z = ops.bottleneck_tail(y, blk['c3'][0], blk['c3'][1], None, nxt['c1'][0], nxt['c1'][1],
                                       shortcut=(a, blk['ds'][0], blk['ds'][1]))
            continue
        if ('dualps' in blk and a.is_contiguous() and y.is_contiguous() and a.dtype == y.dtype and a.shape[0] == y.shape[0]
                and tuple(y.shape[1:3]) == tuple((d - 1) // blk['stride'] + 1 for d in a.shape[1:3])):
            # first block of layers 2 / 3: conv3 + the stride-2 downsample conv as ONE GEMM over [a sampled | y]: the shortcut map is
            # neither written nor read back (the next block's conv1 then runs on its own)
            a = ops.conv1x1_packed_dual_strided(a, y, blk['dualps'], blk['dualps_bias'], blk['c3'][0].shape[0], blk['stride'], True)
            z = None
            continue
        sc = shortcut(a, blk)
        if nxt is not None and 'seam' in blk and (y.numel() // y.shape[-1]) % 128 == 0:
            a, z = ops.bottleneck_seam(y, blk['seam'], blk['c3'][1], sc, nxt['c1'][1], blk['seam_dims'])
            continue
        if fusable:
            a, z = ops.bottleneck_tail(y, blk['c3'][0], blk['c3'][1], sc, nxt['c1'][0], nxt['c1'][1])
        else:
            a = ops.conv_bn_act(y, blk['c3'][0], blk['c3'][1], 1, 0, True, residual=sc)
            z = None
    return a


def run_block(x, blk, pool=None):
    """One Bottleneck. ``pool`` = (splits, mean): fuse the frame pooling into the last conv's epilogue and return the pooled
    fp32 tensor instead of the activation map (which is then never written to HBM)."""
    if is_inloop(blk):
        assert pool is None
        return run_block_inloop(x, blk)
    y = _conv1(x, blk)
    y = _conv2(y, blk)
    if (pool is None and 'dualp' in blk
            and x.shape[:3] == y.shape[:3] and x.dtype == y.dtype and x.is_contiguous() and y.is_contiguous()):
        return ops.conv1x1_packed(x, blk['dualp'], blk['dual'][1], blk['dual'][0].shape[0], True, x2=y, duo=True)   # (two workgroups per CU: 167 us against conv1x1_fat_kernel's 185)
    if pool is None and 'dual' in blk and ops.conv1x1_dual_supported(x, y, blk['dual'][0]):
        return ops.conv1x1_dual(x, y, blk['dual'][0], blk['dual'][1], True)
    sc = shortcut(x, blk)
    duo = 'c3p' in blk and blk['ds'] is None and sc.is_contiguous() and y.is_contiguous()
    if pool is not None:
        if duo and tuple(y.shape[1:3]) == (16, 8):
            return ops.conv1x1_packed_res_pool(y, blk['c3p'], blk['c3'][1], blk['c3'][0].shape[0], sc, pool[0], pool[1], False)[0]
        return ops.conv1x1_bn_act_pool(y, blk['c3'][0], blk['c3'][1], sc, pool[0], pool[1], False)[0]
    if duo:   # the same kernel with the map stored (in the step: the layer-4 pointwise family 0.968-0.981 ms with it, 0.984-0.993 without, three A/B pairs on one box)
        return ops.conv1x1_packed_res(y, blk['c3p'], blk['c3'][1], blk['c3'][0].shape[0], sc)
    return ops.conv_bn_act(y, blk['c3'][0], blk['c3'][1], 1, 0, True, residual=sc)


def run_layer4(a, blocks, pool=None, planes=False):
    """One layer-4 branch: every block, -> the map; with ``pool`` = (splits, mean) the last block's conv3 pools in its epilogue, -> the
    pooled fp32 tensor (the caller decides where that applies). ``planes``: ``a`` and the blocks are split-fp16 planes."""
    run = run_block_planes if planes else run_block
    for blk in blocks[:-1]:
        a = run(a, blk)
    return run(a, blocks[-1]) if pool is None else run(a, blocks[-1], pool=pool)


def run_stem(frames, pack, norm=None):
    """conv1 / bn1 / relu / maxpool (vmgn.py:281-284) in the pack's arithmetic: the 16-bit MFMA stem, the split-fp16 one of the conforming
    mode, or the exact-fp32 one. ``frames``: fp32 NCHW, or uint8 (F,3,H,W) / (F,H,W,3) -- then every stem normalises inside its input
    staging with ``norm`` = (pixel_mean, pixel_std) (None: the ImageNet defaults) and no fp32 frame tensor exists."""
    mean, std = norm if norm is not None else (ops.PIXEL_MEAN, ops.PIXEL_STD)
    if pack['stem_lp'] is not None:
        return ops.stem_lp16(frames, pack['stem_lp'], pack['stem'][1], mean, std)
    if pack.get('stem_s16') is not None:
        return ops.stem_split16(frames, pack['stem_s16'][0], pack['stem_s16'][1], pack['stem_s16'][2], pack['stem'][1], mean, std)
    return ops.stem(frames, pack['stem'][0], pack['stem'][1], pack['dtype'], mean, std)


def eval_frames(model, x):
    """The frames argument of the eval forwards: (B,S,3,H,W) fp32, or uint8 (B,S,3,H,W) / (B,S,H,W,3) as a decoder produces them
    -> (frames (B*S, ...) in x's dtype and layout, B, S, norm for run_stem). Any other dtype is a TypeError, a uint8 tensor in neither
    layout a ValueError."""
    if x.dtype == torch.uint8:
        _, B, S, _, _ = ops.clip_frames(x)
        norm = (getattr(model, 'pixel_mean', ops.PIXEL_MEAN), getattr(model, 'pixel_std', ops.PIXEL_STD))
        return x.reshape((B * S,) + tuple(x.shape[2:])), B, S, norm
    if x.dtype != torch.float32:
        raise TypeError('frames must be float32, got {}'.format(x.dtype))
    B, S, Cc, H, W = x.shape
    return x.reshape(B * S, Cc, H, W), B, S, None


def frame_size(frames):
    """(H, W) of fp32 NCHW or uint8 NCHW / NHWC frames."""
    if frames.dtype == torch.uint8 and ops.frames_layout(frames.shape) == 'nhwc':
        return frames.shape[1], frames.shape[2]
    return frames.shape[2], frames.shape[3]


def single_bnneck(bn):
    """The folded BNNeck pair of a model with one branch, built at pack time for single_branch_tail: (an identity for the global half
    that nothing feeds, ``bn`` folded)."""
    a_bn = fold_bn1d(bn)
    return (torch.ones_like(a_bn[0]), torch.zeros_like(a_bn[1])), a_bn


def single_branch_tail(nodes, bnneck, B, S, P, hw):
    """Attention pooling over the frames + BNNeck of a model with one branch: nodes (B, S*P, C) fp32, ``bnneck`` from single_bnneck
    -> the attention half (B, C) fp32. The tail kernel writes cat(BN(global), BN(attention)); the global half is fed zeros and dropped."""
    g_bn, a_bn = bnneck
    C = nodes.shape[-1]
    sqn = ops.row_sqnorm(nodes.view(B * S * P, C))
    gsum = torch.zeros((B * S, C), dtype=torch.float32, device=nodes.device)
    out = ops.attn_pool_bnneck(nodes, sqn, gsum, g_bn[0], g_bn[1], a_bn[0], a_bn[1], B, S, P, hw)
    return out[:, C:].contiguous()
