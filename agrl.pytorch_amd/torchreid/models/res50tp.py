"""ResNet50 + temporal attention pooling (``res50tp``): the baseline AGRL is measured against -- ResNet50 + four part means +
attention temporal pooling + one BNNeck -> (B, 2048). It is ``gsta`` with no graph layers and four non-pyramid parts.

Drop-in for ``torchreid/models/res50tp.py`` of weleen/AGRL.pytorch: same factory signature (reference res50tp.py:224-236: the flag is
spelt ``pretrain`` here) and keyword swallowing, same module tree / state-dict keys (res50tp.py:111-138: ``bottleneck`` with a frozen
bias, bias-free ``classifier``), call contract ``model(x, *args)`` -- the adjacency is accepted and ignored -- and return conventions
(res50tp.py:186-209).

CUDA tensors in ``eval()`` run ``_sta_hip.hip_forward_res50tp`` -- ``gsta``'s route with the graph layers left out: the part pooling
fused into layer 4's last conv, ``agrl_row_sqnorm`` and ``agrl_attn_pool_bnneck``; no kernel of its own. CPU tensors and train mode use
the stock-torch module tree below.
"""
from __future__ import absolute_import
from __future__ import division

__all__ = ['res50tp']

import os

import torch
from torch import nn
from torch.nn import functional as F

from ._resnet_hip import init_hip_attributes
from .vmgn import Bottleneck, RESNET50_STAGES, make_stage


class ResNet50TP(nn.Module):
    def __init__(self, num_classes, loss, block, layers, last_stride=1, bnneck=True, **kwargs):
        super(ResNet50TP, self).__init__()
        assert block is Bottleneck
        self.num_classes = num_classes
        self.loss = loss
        self.feature_dim = 512 * block.expansion
        self.num_scale = 3
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        ch = 64
        self.layer1, ch = make_stage(ch, 64, layers[0], 1)
        self.layer2, ch = make_stage(ch, 128, layers[1], 2)
        self.layer3, ch = make_stage(ch, 256, layers[2], 2)
        self.layer4, ch = make_stage(ch, 512, layers[3], last_stride)   # this one honours last_stride (res50tp.py:129)

        self.part = 4
        self.avg_pool = nn.AdaptiveAvgPool2d((self.part, 1))
        self.bottleneck = nn.BatchNorm1d(self.feature_dim)
        self.bottleneck.bias.requires_grad_(False)
        self.classifier = nn.Linear(self.feature_dim, num_classes, bias=False)
        self._init_params()

        # MI355X path configuration (not part of the state dict): the plain attributes of GSTASingle
        init_hip_attributes(self)

    def _init_params(self):
        """reference res50tp.py:157-172"""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0, 0.01)

    def featuremaps(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        return self.layer4(self.layer3(self.layer2(self.layer1(x))))

    def pooled_feature(self, x):
        """(B,S,3,H,W) fp32 -> f (B, 2048), t_a (B,S,parts): res50tp.py:187-195."""
        B, S, C, H, W = x.size()
        fm = self.featuremaps(x.view(B * S, C, H, W))
        v_g = self.avg_pool(fm).view(B, S, self.feature_dim, self.part)
        t_a = F.normalize(v_g.norm(p=2, dim=2, keepdim=True), p=1, dim=1)
        f = F.adaptive_avg_pool1d(v_g.mul(t_a).sum(dim=1), 1).view(B, -1)
        return f, t_a.view(B, S, self.part)

    def forward(self, x, *args):
        if x.is_cuda and not self.training:
            from torchreid.models._sta_hip import hip_forward_res50tp
            return hip_forward_res50tp(self, x)
        if x.dtype == torch.uint8:   # the module tree reads fp32 frames: normalise first (hip_ops.clips_to_float)
            from torchreid import hip_ops as _ops
            x = _ops.clips_to_float(x, self.pixel_mean, self.pixel_std)
        f = self.pooled_feature(x)[0]
        bn = self.bottleneck(f)
        if not self.training:
            return bn
        y = self.classifier(bn)
        if self.loss == {'xent'}:
            return y
        elif self.loss == {'xent', 'htri'}:
            return y, f
        raise KeyError('Unsupported loss: {}'.format(self.loss))

    def invalidate_hip_cache(self):
        self._hip_packs.clear()


def res50tp(num_classes=100, loss={'xent', 'htri'}, pretrain=True, bnneck=True, last_stride=1, **kwargs):
    """Factory registered as ``'res50tp'`` (reference res50tp.py:224-236). Never touches the network: ``pretrain`` only takes effect
    through ``AGRL_PRETRAINED_RESNET50`` (a local resnet50-19c8e357.pth)."""
    model = ResNet50TP(num_classes=num_classes, loss=loss, block=Bottleneck, layers=list(RESNET50_STAGES), bnneck=bnneck,
                       last_stride=last_stride, **kwargs)
    path = os.environ.get('AGRL_PRETRAINED_RESNET50', '')
    if pretrain and path and os.path.isfile(path):
        own = model.state_dict()
        picked = {k: v for k, v in torch.load(path, map_location='cpu').items() if k in own and own[k].size() == v.size()}
        own.update(picked)
        model.load_state_dict(own)
    return model
