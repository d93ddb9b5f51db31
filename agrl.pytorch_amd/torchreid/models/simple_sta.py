"""Simple STA (``simple_sta``): STA without the spatial attention map -- the score of a (frame, part) is the channel norm of its
part mean. ResNet50 (last stride 1) + four part means + per part the highest-scoring frame concatenated with the attention-weighted
temporal sum + Linear / BatchNorm1d / ReLU head -> (B, 1024).

Drop-in for ``torchreid/models/simple_sta.py`` of weleen/AGRL.pytorch: same factory signature and keyword swallowing (reference
simple_sta.py:243-257, registered as ``'simple_sta'`` by models/__init__.py:21), same module tree / state-dict keys as ``sta``
(simple_sta.py:124-155), call contract ``model(x, *args)`` and return conventions (simple_sta.py:202-228).

CUDA tensors in ``eval()`` run ``_sta_hip.hip_forward_sta``: the shared conv trunk with the part pooling fused into layer 4's last
conv where that applies (the 2048-channel map is then never written), ``agrl_sta_fuse`` in its norm mode and
``agrl_linear_bn_relu``. CPU tensors and train mode use the stock-torch module tree of ``sta.STA``.
"""
from __future__ import absolute_import
from __future__ import division

__all__ = ['simple_sta']

from torch import nn
from torch.nn import functional as F

from .sta import STA, build_sta


class SimpleSTA(STA):
    """The reference names this class STA as well (simple_sta.py:114); renamed here only to keep the two apart."""
    score = 'norm'

    def __init__(self, *args, **kwargs):
        super(SimpleSTA, self).__init__(*args, **kwargs)
        self.feature_dim = 2048   # the reference leaves the trunk's width here (simple_sta.py:131), sta.py overwrites it

    @staticmethod
    def _head_act(nonlinear):
        return nn.ReLU() if nonlinear == 'relu' else nn.LeakyReLU(0.1)   # simple_sta.py:150

    def temporal_attention(self, fm, v_g, B, S):
        """simple_sta.py:209"""
        return F.normalize(v_g.norm(p=2, dim=2), p=1, dim=1)


def simple_sta(num_classes, loss={'xent', 'htri'}, last_stride=1, pretrained=True, **kwargs):
    """Factory registered as ``'simple_sta'`` (reference simple_sta_p4, simple_sta.py:243-257). Never touches the network:
    ``pretrained`` only takes effect through ``AGRL_PRETRAINED_RESNET50``."""
    return build_sta(SimpleSTA, num_classes, loss, last_stride, pretrained, kwargs)
