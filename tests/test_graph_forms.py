"""hip_ops.graph_forms: which kernel form each stage of a GraphLayer takes at V nodes, and the argument checks of the entry points
behind it -- no GPU needed (an entry point validates its arguments before it launches anything).

Every stage keeps the form it always had up to its own limit (the operands of one tracklet in one workgroup's LDS / registers)
and takes the tiled / streamed form from the next V on; the limits differ per stage, so each is checked on its own."""
import ctypes

import pytest
import torch

OLD = {"gram": "slices", "finalize": "resident", "backward": "resident", "pair": "slices"}
NEW = {"gram": "tiled", "finalize": "rows", "backward": "hbm", "pair": "tiled"}
LIMIT = {"backward": 116, "pair": 144, "finalize": 256, "gram": 304, "propagate": 1024}


def forms(V, C=2048):
    from torchreid import hip_ops as ops
    return ops.graph_forms(V, C)


def test_limits_are_the_ones_the_kernels_have():
    from torchreid import hip_ops as ops
    assert (ops.BACKWARD_RESIDENT_MAX_V, ops.PAIR_PRODUCT_MAX_V, ops.FINALIZE_RESIDENT_MAX_V, ops.GRAM_SLICE_MAX_V, ops.PROPAGATE_TILED_MAX_V) == (
        LIMIT["backward"], LIMIT["pair"], LIMIT["finalize"], LIMIT["gram"], LIMIT["propagate"])
    # the arithmetic behind them (csrc/gcn.hip, csrc/train_tail.hip): what fits 160 KB / 64 KB of LDS
    rowb = 128 * 4 + 16
    assert ((304 + 15) & ~15) * rowb <= 160 * 1024 < ((305 + 15) & ~15) * rowb
    assert 2 * ((144 + 15) & ~15) * rowb <= 160 * 1024 < 2 * ((145 + 15) & ~15) * rowb
    assert (3 * 116 * 116 + 116) * 4 <= 160 * 1024 < (3 * 117 * 117 + 117) * 4   # the entry's message says V <= 115; its check admits 116
    assert 1024 * 16 * 4 <= 64 * 1024 < 1025 * 16 * 4


@pytest.mark.parametrize("V", [64, 115, 116, 128, 144, 256, 304, 1024])
def test_old_form_up_to_each_limit_new_form_from_the_next_v(V):
    at, nxt = forms(V), forms(V + 1)
    for stage in ("backward", "pair", "finalize", "gram"):
        assert at[stage] == (OLD if V <= LIMIT[stage] else NEW)[stage], (V, stage, at)
        assert nxt[stage] == (OLD if V + 1 <= LIMIT[stage] else NEW)[stage], (V + 1, stage, nxt)
    # the message pass: the forms it always had up to V = 1024, the chunked one beyond
    want = {64: "stream", 115: "mfma", 116: "mfma", 128: "mfma", 144: "generic", 256: "tiled", 304: "tiled", 1024: "tiled"}[V]
    want_next = {64: "mfma", 115: "mfma", 116: "mfma", 128: "generic", 144: "generic", 256: "tiled", 304: "tiled", 1024: "chunked"}[V]
    assert at["propagate"] == want and nxt["propagate"] == want_next, (V, at["propagate"], nxt["propagate"])


@pytest.mark.parametrize("stage", sorted(LIMIT))
def test_each_stage_switches_exactly_at_its_own_limit(stage):
    V = LIMIT[stage]
    old, new = ("tiled", "chunked") if stage == "propagate" else (OLD[stage], NEW[stage])
    assert forms(V)[stage] == old and forms(V + 1)[stage] == new
    assert forms(V - 1)[stage] == old and forms(7000)[stage] == new
    # ... and no other stage moves with it
    others = [s for s in LIMIT if s != stage and LIMIT[s] != V]
    assert all(forms(V)[s] == forms(V + 1)[s] for s in others)


def test_propagate_form_mirrors_the_reference_dispatch_of_the_bounds_tests():
    """graph_forms' message-pass names agree with tests/graph_ref.propagate_form wherever that one is defined (V <= 1024)."""
    import graph_ref as GR
    for C in (128, 256, 260, 384):
        for V in (1, 4, 28, 63, 64, 65, 112, 128, 129, 130, 146, 147, 149, 240, 1024):
            ref = GR.propagate_form(V, C)[0]
            assert forms(V, C)["propagate"] == ref.rstrip("248"), (V, C, ref)


def test_entry_points_reject_a_channel_count_that_is_no_multiple_of_128():
    """The Gram and pair-product entries give the message they always gave, at every V, before any launch."""
    from torchreid import _hip
    lib = _hip.lib()
    p = ctypes.c_void_p(4096)   # never dereferenced: the shape check comes first
    for V in (304, 305, 7000):   # the slices form, the first V of the tiled one, a whole tracklet
        assert lib.agrl_graph_gram(p, p, 1, V, 100, 128, None) != 0
        assert lib.agrl_last_error().decode() == "agrl_graph_gram: cslice must be 128 and divide C"
        assert lib.agrl_graph_gram(p, p, 1, V, 256, 64, None) != 0
        assert lib.agrl_last_error().decode() == "agrl_graph_gram: cslice must be 128 and divide C"
    for V in (144, 145, 7000):
        assert lib.agrl_graph_pair_product(p, p, p, p, 1, V, 100, None) != 0
        assert lib.agrl_last_error().decode() == "agrl_graph_pair_product: bad shape (C must be a multiple of 128)"
    # the slices form still asks for its partials; the tiled form has none
    assert lib.agrl_graph_pair_product(p, p, None, p, 1, 144, 128, None) != 0
    assert lib.agrl_last_error().decode() == "agrl_graph_pair_product: null pointer"
    from torchreid import hip_ops as ops
    for V in (144, 145):
        a = torch.zeros((1, V, 100))
        with pytest.raises(AssertionError):
            ops.graph_pair_product(a, a)
