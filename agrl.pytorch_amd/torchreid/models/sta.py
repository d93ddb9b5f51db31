"""STA (``sta``): Spatial-Temporal Attention baseline (Fu et al., AAAI 2019) -- ResNet50 (last stride 1) + a per-pixel channel-norm
attention map pooled into four horizontal parts + per part the highest-scoring frame concatenated with the attention-weighted
temporal sum + Linear / BatchNorm1d / ReLU head -> (B, 1024).

Drop-in for ``torchreid/models/sta.py`` of weleen/AGRL.pytorch: same factory signature and keyword swallowing (reference
sta.py:268-282, registered as ``'sta'`` by models/__init__.py:20), same module tree / state-dict keys (sta.py:126-159: ``fc1.0``,
``fc1.1``, a ``classifier`` with bias, no ``bottleneck``; the ``dropout`` module exists and is unused), same call contract
``model(x, *args)`` -- the adjacency the driver passes is accepted and ignored -- and return conventions (sta.py:206-253).

CUDA tensors in ``eval()`` run ``_sta_hip.hip_forward_sta``: the shared conv trunk, then ``agrl_sta_frame_stats`` (one pass over the
layer-4 map), ``agrl_sta_fuse`` and ``agrl_linear_bn_relu`` (csrc/sta.hip). CPU tensors and train mode use the stock-torch module
tree below; a native train step for this model is not provided.
"""
from __future__ import absolute_import
from __future__ import division

__all__ = ['sta']

import os

import torch
from torch import nn
from torch.nn import functional as F

from ._resnet_hip import init_hip_attributes
from .vmgn import Bottleneck, RESNET50_STAGES, make_stage


class STA(nn.Module):
    """reference sta.py:116-253. ``score`` names the per-(frame, part) score the temporal attention is built from: ``'map'`` -- the
    L2-normalised per-pixel channel-norm map, part pooled (this model) -- or ``'norm'`` -- the channel norm of the part means
    (``simple_sta``, which derives from this class)."""
    score = 'map'

    def __init__(self, num_classes, loss, block, layers, reduced_dim=512, nonlinear='relu', **kwargs):
        super(STA, self).__init__()
        assert block is Bottleneck
        self.loss = loss
        self.parts = 4
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        ch = 64
        self.layer1, ch = make_stage(ch, 64, layers[0], 1)
        self.layer2, ch = make_stage(ch, 128, layers[1], 2)
        self.layer3, ch = make_stage(ch, 256, layers[2], 2)
        self.layer4, ch = make_stage(ch, 512, layers[3], 1)    # last stride 1 whatever ``last_stride`` says (sta.py:145)

        self.parts_avgpool = nn.AdaptiveAvgPool2d((self.parts, 1))
        self.dropout = nn.Dropout(p=0.5)                         # never called (sta.py:149)
        self.fc1 = nn.Sequential(nn.Linear(2 * ch, reduced_dim, bias=False), nn.BatchNorm1d(reduced_dim), self._head_act(nonlinear))
        self.feature_dim = reduced_dim
        self.classifier = nn.Linear(reduced_dim, num_classes)
        self._init_params()

        # MI355X path configuration (not part of the state dict): the plain attributes of GSTASingle
        init_hip_attributes(self)

    @staticmethod
    def _head_act(nonlinear):
        return nn.ReLU()

    def _init_params(self):
        """reference sta.py:178-193"""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0, 0.01)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def featuremaps(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        return self.layer4(self.layer3(self.layer2(self.layer1(x))))

    def temporal_attention(self, fm, v_g, B, S):
        """(B*S,c,h,w) map, (B,S,c,parts) part means -> t_a (B,S,parts): sta.py:213-220."""
        F_, _, h, w = fm.shape
        g_a = F.normalize(fm.norm(p=2, dim=1, keepdim=True).view(F_, 1, h * w), p=2, dim=2).view(F_, 1, h, w)
        return F.normalize(self.parts_avgpool(g_a).view(B, S, self.parts), p=1, dim=1)

    def fused_feature(self, x):
        """(B,S,3,H,W) fp32 -> f_g (B, 2c), t_a (B,S,parts), idx (B,parts): the tail in front of ``fc1`` (sta.py:209-238)."""
        B, S, C, H, W = x.size()
        fm = self.featuremaps(x.view(B * S, C, H, W))
        c = fm.size(1)
        v_g = self.parts_avgpool(fm).view(B, S, c, self.parts)
        t_a = self.temporal_attention(fm, v_g, B, S)
        idx = t_a.argmax(dim=1)
        f_1 = v_g.gather(dim=1, index=idx.view(B, 1, 1, self.parts).expand(B, 1, c, self.parts)).view(B, c, self.parts)
        f_2 = v_g.mul(t_a.unsqueeze(2)).sum(dim=1)
        f_g = F.adaptive_avg_pool1d(torch.cat([f_1, f_2], dim=1), 1).view(B, -1)
        return f_g, t_a, idx

    def forward(self, x, *args):
        if x.is_cuda and not self.training:
            from torchreid.models._sta_hip import hip_forward_sta
            return hip_forward_sta(self, x)
        if x.dtype == torch.uint8:   # the module tree reads fp32 frames: normalise first (hip_ops.clips_to_float)
            from torchreid import hip_ops as _ops
            x = _ops.clips_to_float(x, self.pixel_mean, self.pixel_std)
        f_t = self.fc1(self.fused_feature(x)[0])
        if not self.training:
            return f_t
        y = self.classifier(f_t)
        if self.loss == {'xent'}:
            return y
        elif self.loss == {'xent', 'htri'}:
            return y, f_t
        raise KeyError('Unsupported loss: {}'.format(self.loss))

    def invalidate_hip_cache(self):
        self._hip_packs.clear()


def build_sta(cls, num_classes, loss, last_stride, pretrained, kwargs):
    model = cls(num_classes=num_classes, loss=loss, block=Bottleneck, layers=list(RESNET50_STAGES), last_stride=last_stride,
                reduced_dim=1024, nonlinear='relu', **kwargs)
    path = os.environ.get('AGRL_PRETRAINED_RESNET50', '')
    if pretrained and path and os.path.isfile(path):
        own = model.state_dict()
        picked = {k: v for k, v in torch.load(path, map_location='cpu').items() if k in own and own[k].size() == v.size()}
        own.update(picked)
        model.load_state_dict(own)
    return model


def sta(num_classes, loss={'xent', 'htri'}, last_stride=1, pretrained=True, **kwargs):
    """Factory registered as ``'sta'`` (reference sta_p4, sta.py:268-282). Never touches the network: ``pretrained`` only takes
    effect through ``AGRL_PRETRAINED_RESNET50`` (a local resnet50-19c8e357.pth)."""
    return build_sta(STA, num_classes, loss, last_stride, pretrained, kwargs)
