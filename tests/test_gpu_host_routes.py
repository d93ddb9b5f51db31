"""The host path above the C-ABI, held to a recording: every eval forward of the six models (four precisions, two frame sizes, first /
second / uint8 forward) and the native train step of vmgn, gsta and ganet (fp32, bf16x3) must call the entry points that
tests/golden/host_routes.json lists, in that order, and give the recorded bits. The cases and how they run are
tools/record_host_routes.py's -- the recording was made by that script, run twice, on the tree in front of the shared ResNet-50 host
path (models/_resnet_hip.py). A hash stored as null was not bit-reproducible between those two runs and is not compared; the
entry-point lists always are. Recorded with the default (fp16) library: skipped when the bf16 build is the loaded one."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_host_routes", os.path.join(ROOT, "tools", "record_host_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _recorder()
with open(os.path.join(ROOT, "tests", "golden", "host_routes.json")) as _f:
    _STORED = json.load(_f)
GOLD = R.decode(_STORED)


@pytest.fixture(autouse=True)
def _fp16_build_only():
    from torchreid import hip_ops as ops
    if ops.LP_NAME != GOLD["lp_name"]:
        pytest.skip("the routes were recorded with the %s library" % GOLD["lp_name"])


def same_calls(case, got, want):
    diff = R.first_difference(got, want)
    if diff is not None:
        print("%s: %s" % (case, diff))
    assert diff is None, "%s: %s" % (case, diff)


def test_recording_covers_every_case():
    assert sorted(GOLD["eval"]) == sorted(R.eval_cases()) and sorted(GOLD["train"]) == sorted(R.train_cases())
    def pack_time(names):   # agrl_conv1x1_pack, agrl_conv3x3_pack, agrl_bottleneck_seam_pack, agrl_split16_weight_planes
        return [n for n in names if n == "agrl_split16_weight_planes" or ("_pack" in n and "_packed" not in n)]
    for case, rec in GOLD["eval"].items():
        first, second, u8 = rec["calls"]
        assert pack_time(first) or "/%s/" % GOLD["lp_name"] not in case, case   # the 16-bit packs go through the library's packers
        assert not pack_time(second) and not pack_time(u8), case   # answered from the pack cache
        assert len(second) and first[len(first) - len(second):] == second, case


@pytest.mark.parametrize("case", sorted(GOLD["eval"]))
def test_eval_forward_takes_the_recorded_route(case):
    want = GOLD["eval"][case]
    got = R.run_eval_case(case)
    for i, which in enumerate(("first", "second", "uint8")):
        same_calls("%s %s forward" % (case, which), got["calls"][i], want["calls"][i])
    for i, which in enumerate(("first", "second", "uint8")):
        if want["sha256"][i] is not None:
            assert got["sha256"][i] == want["sha256"][i], "%s %s forward: the output's bits differ" % (case, which)


@pytest.mark.parametrize("case", sorted(GOLD["train"]))
def test_train_step_takes_the_recorded_route(case):
    want = GOLD["train"][case]
    got = R.run_train_case(case)
    same_calls(case, got["calls"], want["calls"])
    assert (got["np_next"], got["torch_next"]) == (want["np_next"], want["torch_next"]), "%s: the generators' state after the step" % case
    assert sorted(got["sha256"]) == sorted(want["sha256"])
    for k, h in want["sha256"].items():
        if h is not None:
            assert got["sha256"][k] == h, "%s: the bits of %s differ" % (case, k)
