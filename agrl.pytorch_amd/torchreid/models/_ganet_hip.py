"""MI355X execution of the sibling model ``ganet``'s eval forward (reference torchreid/models/ganet.py:378-424) through the
C-ABI of libagrl_hip.so. Same conv kernels, data layout and host path as vmgn (``_resnet_hip``); what is specific:

    part nodes   ganet.py:384-400: every pyramid slice through the position attention module, ``pam(slice) + slice``
                 average pooled. The value conv (2048 -> 2048 on every position, three pyramid levels) is never evaluated per
                 position -- pooling is linear and attention rows sum to one, so per node
                     avgpool(gamma * value . attention^T + 2 slice) = gamma * (Wv (X abar) + bv) + 2 mean(slice)
                 : one stacked query / key 1x1 conv over the map (``agrl_conv2d_bn_act``, bias, no ReLU), ``agrl_pam_pool``
                 (energies, softmax, abar, X abar, mean), ONE (F*P, C) x (C, C) Linear (``agrl_linear_nobias``) and
                 ``agrl_pam_combine``. With the module's gamma == 0 (its value at construction) only the means are needed.
    graph layers ganet.py:253-283: diagonal-masked graphs (``mask_diag``), ``input + gamma * h'`` (``keep`` = 1); with the
                 constructor's gamma = 0 a layer's output IS its input (0 * h' adds nothing) and its kernels are skipped.
    tail         ganet.py:402-411: outputs concatenated along the channels, attention pooling over (num_gb + 1) * 2048
                 channels, one BNNeck (the vmgn tail kernel; its global half is fed zeros and dropped).
"""
from __future__ import annotations

import torch

from torchreid import hip_ops as ops
from torchreid import _hip
import torchreid.models._resnet_hip as R


def _pack_entries(model, pack, dtype, s16):
    """The position attention module, the BNNeck and the graph layers. ('fp16x3': the conv trunk in the split-fp16 arithmetic as in
    vmgn / gsta; the attention module, the graph layers and the tail stay exact fp32)"""
    pam = model.pam_layer
    pack.update({
        # stacked query / key conv as one OHWI weight (2*Cq, 1, 1, C) + bias; value conv as a Linear weight (C, C) + bias
        'qk_w': torch.cat([pam.query_conv.weight, pam.key_conv.weight], 0).detach().float().permute(0, 2, 3, 1).contiguous().to(dtype),
        'qk_b': torch.cat([pam.query_conv.bias, pam.key_conv.bias], 0).detach().float().contiguous(),
        'cq': pam.query_conv.weight.shape[0],
        'v_w': R.own_copy(pam.value_conv.weight.detach().float().view(pam.value_conv.weight.shape[0], -1), dtype),
        'v_b': R.own_copy(pam.value_conv.bias, torch.float32),
        'pam_gamma': float(pam.gamma.detach()),
        'bnneck': R.single_bnneck(model.bottleneck),
        'graph': [],
    })
    for layer in model.graph_layers:
        scale, shift = R.fold_bn1d(layer.bn)
        pack['graph'].append({'w': R.own_copy(layer.linear.weight, dtype), 'scale': scale, 'shift': shift,
                              'slope': float(layer.relu.negative_slope), 'use_pose': bool(layer.use_pose),
                              'learn_graph': bool(layer.learn_graph)})


def pack_weights(model, device, precision):
    return R.pack_weights(model, device, precision, _pack_entries, 'ganet')


def hip_forward_ganet(model, x, adj, stages=None):
    """Eval forward of ``ganet`` on the GPU: (B,S,3,H,W) fp32 (or uint8 frames, see _vmgn_hip.hip_forward), (B,V,V) fp32 ->
    (B, (num_gb + 1) * 2048) fp32."""
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
        a = R.run_layer4(R.run_trunk(R.run_stem(frames, pack, norm), pack['trunk']), pack['l4'])
        C = a.shape[-1]
        # ---- position-attention part nodes
        gamma_p = pack['pam_gamma']
        if gamma_p != 0.0:
            qk = ops.conv_bn_act(a, pack['qk_w'], pack['qk_b'], 1, 0, False)
            xbar, xmean = ops.pam_pool(a, qk, splits)
            operand = xbar.to(pack['dtype']) if lp else xbar
            y = ops.linear_nobias(operand.view(B * V, C), pack['v_w'])
            nodes, nodes_lp = ops.pam_combine(y, pack['v_b'], xmean, gamma_p, want_lp=lp)
        else:
            _, xmean = ops.pam_pool(a, None, splits)
            nodes, nodes_lp = ops.pam_combine(None, None, xmean, 0.0, want_lp=lp)
        del a
        nodes = nodes.view(B, V, C)
        if nodes_lp is not None:
            nodes_lp = nodes_lp.view(B, V, C)
        # ---- graph layers, outputs concatenated with their input
        adj32 = adj.detach().to(torch.float32).contiguous()
        outs = [nodes]
        for g, layer in zip(pack['graph'], model.graph_layers):
            gamma_g = float(layer.gamma)   # a plain attribute in the reference (not a parameter): read at call time
            cur = outs[-1]
            if gamma_g == 0.0:
                outs.append(cur)           # input + 0 * h' (ganet.py:283)
                continue
            operand = nodes_lp if lp else cur
            h = ops.linear_nobias(operand.view(B * V, C), g['w']).view(B, V, C)
            G = ops.graph_matrix(cur, adj32, g['use_pose'], g['learn_graph'], mask_diag=True)
            if stages is not None:
                stages.setdefault('G', []).append(G)
            nxt, nodes_lp = ops.graph_propagate(cur, h, G, g['scale'], g['shift'], gamma_g, g['slope'], want_lp=lp, keep=1.0)
            outs.append(nxt)
        cat = torch.cat(outs, dim=2).contiguous()
        if stages is not None:
            stages.update(nodes=nodes, cat=cat)
        # ---- attention pooling + BNNeck over the concatenated channels
        return R.single_branch_tail(cat, pack['bnneck'], B, S, P, 1)
