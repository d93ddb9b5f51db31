"""Host side of layer 3's chained kernel, without a GPU: the per-block pointer table, which runs of blocks pack_stage marks, and which
launches run_trunk issues for them on a stub of hip_ops."""
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (os.path.join(ROOT, "agrl.pytorch_amd"),) if p not in sys.path]

from torchreid import hip_ops as ops  # noqa: E402
from torchreid.models import _resnet_hip as R  # noqa: E402

LP = ops.LP_DTYPE


def block(chainable=True, dims=(256, 1024, 256)):
    """a pack_stage-style dict of one Bottleneck with CPU tensors"""
    blk = {"c1": (torch.zeros((256, 1, 1, 1024), dtype=LP), torch.zeros(256)),
           "c2": (torch.zeros((256, 3, 3, 256), dtype=LP), torch.zeros(256)),
           "c3": (torch.zeros((1024, 1, 1, 256), dtype=LP), torch.zeros(1024)), "stride": 1, "ds": None}
    if chainable:
        blk.update(c2p=torch.zeros(16, dtype=torch.uint8), seam=torch.zeros(16, dtype=torch.uint8), seam_dims=dims,
                   seam_b1n=torch.zeros(256))
    return blk


def test_table_rows_point_at_the_blocks_tensors():
    blocks = [block() for _ in range(3)]
    t = ops.bottleneck_chain_table(blocks)
    assert t.dtype == torch.int64 and tuple(t.shape) == (3, 8)
    for row, b in zip(t.tolist(), blocks):
        assert row == [b["c2p"].data_ptr(), b["c2"][1].data_ptr(), b["seam"].data_ptr(), b["c3"][1].data_ptr(),
                       b["seam_b1n"].data_ptr(), 0, 0, 0]


def test_block_ok_and_run_lengths():
    assert ops.bottleneck_chain_block_ok(block())
    assert not ops.bottleneck_chain_block_ok(block(chainable=False))            # a model without packs
    assert not ops.bottleneck_chain_block_ok(block(dims=(256, 1024, 512)))      # the seam into a layer-4 branch
    assert not ops.bottleneck_chain_block_ok(dict(block(), ds=(None, None)))    # a first block
    assert not ops.bottleneck_chain_block_ok(dict(block(), stride=2))
    # layer 3 of ResNet-50: first block, four chainable ones, the last (no seam behind it)
    layer3 = [block(chainable=False)] + [block() for _ in range(4)] + [block(chainable=False)]
    assert [R.chain_run(layer3, i) for i in range(6)] == [0, 4, 3, 2, 1, 0]
    assert R.chain_run([block() for _ in range(7)], 0) == ops.CHAIN_MAX      # a longer run is cut at the kernel's limit
    assert R.chain_run([block(chainable=False) for _ in range(3)], 0) == 0


class StubOps(types.SimpleNamespace):
    """hip_ops as run_trunk sees it: every launch is recorded, tensors are tokens"""

    def __init__(self, chain_on):
        super().__init__(CHAIN_MAX=ops.CHAIN_MAX, bottleneck_chain_block_ok=ops.bottleneck_chain_block_ok, calls=[], chain_on=chain_on)

    def conv_bn_act(self, x, w, b, stride, pad, relu, residual=None):
        self.calls.append("conv%dx%d%s" % (w.shape[1], w.shape[2], "+res" if residual is not None else ""))
        return torch.zeros((2, 16, 8, w.shape[0]), dtype=LP)

    def conv3x3_packed(self, y, packed, bias, cout, relu):
        self.calls.append("conv3x3")
        return y

    def bottleneck_seam(self, y, packed, b3, res, b1n, dims):
        self.calls.append("seam")
        return res, y

    def bottleneck_chain_supported(self, z, a, blocks):
        return self.chain_on and ops.bottleneck_chain_supported(z, a, blocks, forced=True)

    def bottleneck_chain(self, z, a, table, n):
        self.calls.append("chain%d" % n)
        assert tuple(table.shape) == (n, 8)
        return a, z

    def bottleneck_block_supported(self, *a):
        return False

    def bottleneck_tail_supported(self, *a):
        return False


def run(blocks, chain_on, monkeypatch):
    stub = StubOps(chain_on)
    monkeypatch.setattr(R, "ops", stub)
    R.run_trunk(torch.zeros((2, 16, 8, 1024), dtype=LP), blocks)
    return stub.calls


def mark_runs(blocks):
    """what pack_stage does behind the seam packs"""
    i = 0
    while i < len(blocks):
        n = R.chain_run(blocks, i)
        if n:
            blocks[i]["chain"] = (n, ops.bottleneck_chain_table(blocks[i:i + n]))
        i += max(n, 1)
    return blocks


def test_run_trunk_chains_the_middle_blocks(monkeypatch):
    blocks = mark_runs([block() for _ in range(4)] + [block(chainable=False)])
    per_block = ["conv3x3", "seam"]
    last = ["conv3x3", "conv1x1+res"]
    assert run(blocks, True, monkeypatch) == ["conv1x1", "chain4"] + last
    assert run(blocks, False, monkeypatch) == ["conv1x1"] + 4 * per_block + last
    # six chainable blocks: a run of four, then a run of two that starts from the first run's z
    blocks = mark_runs([block() for _ in range(6)] + [block(chainable=False)])
    assert run(blocks, True, monkeypatch) == ["conv1x1", "chain4", "chain2"] + last


def test_model_without_packs_falls_through(monkeypatch):
    blocks = mark_runs([block(chainable=False) for _ in range(3)])
    assert all("chain" not in b for b in blocks)
    assert run(blocks, True, monkeypatch) == ["conv1x1", "conv3x3", "conv1x1+res"] * 3
