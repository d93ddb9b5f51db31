"""BASELINE configs[1] names bf16: libagrl_hip_bf16.so (the same sources with bfloat16 as the 16-bit storage / MFMA-operand type)
under the same parity tests as the default fp16 library, inside the default ``-m gpu`` run.

The 16-bit type is fixed when torchreid is imported (AGRL_HIP_LP16), so the bf16 build runs in a FRESH CHILD interpreter -- started
with subprocess, never a re-exec of a process that has touched the GPU -- on: the B = 32, S = 8 stage-by-stage test (the benchmarked
dispatch), every 16-bit kernel case of tests/test_gpu_kernels.py, the elementwise bounds of tests/test_gpu_graph_bounds.py, the model-level 16-bit tests and the whole-pipeline Rank-1 / mAP
test. The tests read their bars from tests/lp16.py (bf16: 8 significand bits -- 1e-2 per stage / 5e-2 on the embedding; fp16 is held
to the north star's 1e-3)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(os.environ.get("AGRL_HIP_LP16", "fp16") == "bf16", reason="this process already runs the bf16 build")
def test_bf16_build_passes_the_16_bit_parity_tests_in_a_fresh_process():
    lib = os.path.join(ROOT, "agrl.pytorch_amd", "lib", "libagrl_hip_bf16.so")
    assert os.path.exists(lib), "libagrl_hip_bf16.so is not built (make -C agrl.pytorch_amd/csrc)"
    env = dict(os.environ, AGRL_HIP_LP16="bf16")
    env.pop("AGRL_HIP_LIB", None)
    env.pop("AGRL_HIP_PRECISION", None)
    sel = ["tests/test_gpu_model.py::test_vmgn_eval_at_benchmarked_size_stage_by_stage",
           "tests/test_gpu_model.py::test_vmgn_eval_16_bit_mode_close_and_ranking_preserved",
           "tests/test_gpu_model.py::test_vmgn_eval_shape_variants",
           "tests/test_gpu_eval.py::test_16_bit_pipeline_keeps_rank1_and_map",
           "tests/test_gpu_kernels.py", "tests/test_gpu_graph_bounds.py"]
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"] + sel, env=env, cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=3000)
    tail = out.stdout.decode()[-3000:]
    print(tail)
    assert out.returncode == 0, tail
    # ... and it really was the other library
    probe = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, 'tests'); import lp16; from torchreid import _hip; "
                            "_hip.lib(); print(_hip.LP_NAME, _hip.LIB_PATH)"], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           timeout=600)
    assert probe.returncode == 0 and "bf16 " in probe.stdout.decode() and "libagrl_hip_bf16.so" in probe.stdout.decode(), probe.stdout.decode() + probe.stderr.decode()[-2000:]
