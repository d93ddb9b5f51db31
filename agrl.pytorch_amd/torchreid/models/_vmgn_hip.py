"""MI355X execution of the VMGN eval forward (reference call site: train_vidreid_xent_htri.py:469/:499
-> GSTA.forward, vmgn.py:292-321) and of its single-branch predecessor ``gsta`` through the C-ABI of libagrl_hip.so, on the shared
ResNet-50 host path (``_resnet_hip``: data layout, pack cache, stem, trunk and Bottleneck runners). What is these two models' own:

    part nodes    fp32 (B, V = S*P, 2048)
    graph         fp32 (B, V, V)
    embedding     fp32 (B, 4096) = cat(BN(global), BN(attention)); gsta: (B, 2048), the attention half
"""
from __future__ import annotations

import torch

from torchreid import hip_ops as ops
from torchreid import _hip
import torchreid.models._resnet_hip as R


def whole_k_tiles(w):
    """The in-loop split GEMM needs whole 32-element k-tiles."""
    return w.dim() == 2 and w.shape[1] % 32 == 0


def _pack_entries(model, pack, dtype, s16):
    """The BNNeck(s) and the graph layers."""
    if hasattr(model, 'layer4_1'):   # vmgn: two layer4 branches, two BNNecks
        pack['g_bn'] = R.fold_bn1d(model.global_bottleneck)
        pack['a_bn'] = R.fold_bn1d(model.att_bottleneck)
    else:                            # gsta: one branch, one BNNeck (the unused global half gets an identity)
        pack['bnneck'] = R.single_bnneck(model.bottleneck)
    pack['graph'] = []
    for layer in model.graph_layers:
        scale, shift = R.fold_bn1d(layer.bn)
        gw = R.own_copy(layer.linear.weight, dtype)
        if s16 and whole_k_tiles(gw):
            # the GraphLayer's Linear in the split-fp16 arithmetic as well (182 -> ~70 us per layer at 32 tracklets): weight times
            # 2^k, the 2^-k folded into the BatchNorm scale the GEMM's epilogue multiplies the accumulator with (exact)
            gw = ops.split16_inloop_weights(gw)
            scale = (scale * gw.agrl_unscale).contiguous()
            scale.agrl_folded_unscale = gw.agrl_unscale
        pack['graph'].append({
            'w': gw,
            'scale': scale, 'shift': shift,
            'gamma': float(layer.gamma), 'slope': float(layer.relu.negative_slope),
            'use_pose': bool(layer.use_pose), 'learn_graph': bool(layer.learn_graph),
        })


def pack_weights(model, device, precision):
    """BN-fold + re-layout every weight of the eval forward for ``device``; cached on the model (_resnet_hip.pack_weights)."""
    return R.pack_weights(model, device, precision, _pack_entries, 'vmgn')


def hip_featuremaps(frames, pack, norm=None):
    """(F,3,H,W) fp32 NCHW (or uint8 frames, see run_stem) -> x4_1, x4_2 NHWC (F,h,w,2048). reference vmgn.py:280-290."""
    a = R.run_trunk(R.run_stem(frames, pack, norm), pack['trunk'])
    return R.run_layer4(a, pack['l4_1']), R.run_layer4(a, pack['l4_2'])


def hip_features_pooled(frames, pack, splits, norm=None):
    """Conv stages with the global / part pooling fused into the last conv of each layer4 branch, on 16-bit tensors or -- in the
    conforming mode with planes -- on split-fp16 planes behind layer 3's first block (16x8 maps): -> gsum (F,C) per-frame sums,
    nodes (F,P,C) fp32. None when the fusion does not apply."""
    first = pack.get('planes_from')
    if (pack['dtype'] != ops.LP_DTYPE and first is None) or pack['l4_1'][0]['stride'] != 1:
        return None
    # applicability is decided from the input size BEFORE anything is launched (a late bail-out would make the caller
    # recompute stem + trunk): the fused epilogue needs 16 x 8 = 128-pixel layer-4 maps, i.e. frames of 256 x 128
    H, W = R.frame_size(frames)
    h4, w4 = H, W
    for _ in range(4):   # stem conv /2, maxpool /2, layer2 /2, layer3 /2 (kernel 7 pad 3 / kernel 3 pad 1: ceil halving)
        h4, w4 = (h4 + 1) // 2, (w4 + 1) // 2
    if (h4, w4) != (16, 8):
        return None
    a = R.run_stem(frames, pack, norm)
    planes = first is not None
    if not planes:
        a = R.run_trunk(a, pack['trunk'])
    else:
        a = R.run_trunk(a, pack['trunk'][:first - 1])
        a = R.run_block_inloop(a, pack['trunk'][first - 1], out_planes=2)
        for blk in pack['trunk'][first:]:
            a = R.run_block_planes(a, blk)
    assert a.shape[1] == 16 and a.shape[2] == 8
    splits = list(splits)
    # (the two branches on two HIP streams, and the graph matrix on a side stream under the Linear, were options until round 4:
    # both measured no faster -- every kernel here fills the chip -- and were retired)
    gsum = R.run_layer4(a, pack['l4_1'], pool=([1], False), planes=planes)
    nodes = R.run_layer4(a, pack['l4_2'], pool=(splits, True), planes=planes)
    return gsum.view(gsum.shape[0], gsum.shape[2]), nodes


def gcn_commute_enabled(model=None):
    """Always True: the GraphLayer runs commuted (hip_graph_layers). Kept for bench.py's labels."""
    return True


def hip_graph_layers(nodes, nodes_lp, adj, pack, stages=None, commute=True):
    """GraphLayer x num_gb on (B,V,C) fp32 nodes. reference vmgn.py:311-312 -> :142-172. The Linear runs commuted behind the message
    pass, G (f W^T) = (G f) W^T. ``nodes_lp`` and ``commute`` stay for bench.py's call: the former is not read, and commute=False
    (Linear -> message pass, retired) raises."""
    if not commute:
        raise ValueError("hip_graph_layers runs the commuted GraphLayer only ((G f) W^T): the Linear -> message pass form is retired")
    for i, g in enumerate(pack['graph']):
        # graph -> P = G f (written once, in the GEMM's operand dtype) -> ONE GEMM whose epilogue applies BatchNorm1d + LeakyReLU
        # + the residual mix. h never exists; f and out cross HBM once each.
        pre = False
        if ops.graph_tracklet_operand_supported(nodes):   # many tracklets per GPU: one workgroup per tracklet, one launch
            P, G = ops.graph_tracklet_operand(nodes, adj, g['use_pose'], g['learn_graph'], pack['dtype'], want_graph=stages is not None)
        else:
            G = ops.graph_matrix(nodes, adj, g['use_pose'], g['learn_graph'])
            # conforming mode: P is read by the GEMM only -- written with its fp16 halves already formed
            pre = getattr(g['w'], 'agrl_presplit', False) and ops.graph_apply_presplit_supported(nodes)
            P = ops.graph_apply_operand(G, nodes, pack['dtype'], presplit=pre)
        if stages is not None:
            stages['G%d' % i] = G
        nodes = ops.graph_linear_mix(P, g['w'], nodes, g['scale'], g['shift'], g['gamma'], g['slope'], p_presplit=pre)
    return nodes


def hip_forward(model, x, adj, return_feats=False, stages=None):
    """Eval forward on the GPU: (B,S,3,H,W) fp32 -- or uint8 frames, (B,S,3,H,W) / (B,S,H,W,3), normalised with model.pixel_mean /
    pixel_std inside the stem kernel -- and (B,V,V) fp32 -> (B,4096) fp32. ``stages``: an optional dict that
    receives the intermediate tensors of the path (per-frame sums of x4_1, part nodes, graphs, graph output, pre-BN
    features) for the stage-by-stage parity tests."""
    _hip.lib()  # fail loudly before touching anything if the extension is missing
    frames, B, S, norm = R.eval_frames(model, x)
    P = model.total_split
    V = S * P
    packed_adj = ops.adjacency_is_packed(adj)   # int32 (B, V, ceil(V/32)): the bit-packed graph (hip_ops.adjacency_pack*)
    if tuple(adj.shape) != ((B, V, (V + 31) // 32) if packed_adj else (B, V, V)):
        raise ValueError('adj must be {} (fp32) or {} (bit-packed int32) for S={} and {} parts, got {}'.format(
            (B, V, V), (B, V, (V + 31) // 32), S, P, tuple(adj.shape)))
    pack = pack_weights(model, x.device, model.hip_precision)
    lp = pack['dtype'] == ops.LP_DTYPE
    with torch.no_grad(), ops.f32_split(model.hip_precision == 'bf16x3'):
        fused = hip_features_pooled(frames, pack, model.total_split_list, norm)
        if fused is not None:
            gsum, nodes = fused
            hw = 128
        else:
            x4_1, x4_2 = hip_featuremaps(frames, pack, norm)
            hw = x4_1.shape[1] * x4_1.shape[2]
            gsum, nodes, _ = ops.part_pool(x4_1, x4_2, model.total_split_list, want_lp=False)
            del x4_1, x4_2
        C = nodes.shape[-1]
        nodes = nodes.view(B, V, C)
        adj32 = adj.detach().contiguous() if packed_adj else adj.detach().to(torch.float32).contiguous()
        if stages is not None:
            stages.update(gsum=gsum, hw=hw, nodes=nodes)
        nodes = hip_graph_layers(nodes, None, adj32, pack, stages)
        model._hip_query = None
        if ops.attn_tail_supported(S, P, C, B):
            # many tracklets per GPU: node norms + attention pooling + BNNeck + the distance matrix's query operand in one launch
            want = return_feats or stages is not None
            out, feats, query, _ = ops.attn_tail(nodes, gsum, pack['g_bn'][0], pack['g_bn'][1], pack['a_bn'][0], pack['a_bn'][1],
                                                 B, S, P, hw, want_feats=want, query_dtype=ops.LP_DTYPE if lp else torch.float32)
            model._hip_query = ops.QueryOperandCache(out, query)
            res = (out, feats[0], feats[1]) if want else out
        else:
            sqn = ops.row_sqnorm(nodes.view(B * V, C))
            res = ops.attn_pool_bnneck(nodes, sqn, gsum, pack['g_bn'][0], pack['g_bn'][1], pack['a_bn'][0],
                                       pack['a_bn'][1], B, S, P, hw, want_feats=return_feats or stages is not None)
        if stages is not None:
            stages.update(nodes_out=nodes, out=res[0], g_f=res[1], att_f=res[2])
            return res if return_feats else res[0]
        return res


def hip_forward_gsta(model, x, adj):
    """Eval forward of the single-branch ``gsta`` on the GPU: (B,S,3,H,W) fp32 (or uint8 frames, see hip_forward), (B,V,V) fp32 -> (B,2048) fp32.
    reference gsta.py:273-298. Same kernels as vmgn; the attention tail kernel writes cat(BN(global), BN(attention)) and
    only its second half exists for this model (the global half is fed zeros)."""
    _hip.lib()
    frames, B, S, norm = R.eval_frames(model, x)
    P = model.total_split
    V = S * P
    if tuple(adj.shape) != (B, V, V):
        raise ValueError('adj must be {} for S={} and {} parts, got {}'.format((B, V, V), S, P, tuple(adj.shape)))
    pack = pack_weights(model, x.device, model.hip_precision)
    lp = pack['dtype'] == ops.LP_DTYPE
    splits = list(model.total_split_list)
    with torch.no_grad(), ops.f32_split(model.hip_precision == 'bf16x3'):
        a = R.run_trunk(R.run_stem(frames, pack, norm), pack['trunk'])
        if lp and a.shape[1] * a.shape[2] == 128 and pack['l4'][0]['stride'] == 1:   # any 128-pixel map
            nodes = R.run_layer4(a, pack['l4'], pool=(splits, True))
            hw = 128
        else:
            a = R.run_layer4(a, pack['l4'])
            hw = a.shape[1] * a.shape[2]
            _, nodes, _ = ops.part_pool(a, a, splits, want_lp=False)
        C = nodes.shape[-1]
        nodes = nodes.view(B, V, C)
        nodes = hip_graph_layers(nodes, None, adj.detach().to(torch.float32).contiguous(), pack)
        return R.single_branch_tail(nodes, pack['bnneck'], B, S, P, hw)
