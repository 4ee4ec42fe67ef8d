"""Runs the C++ driver of the mixture-of-experts entries of the API mirror (llm-inference-engine_amd/cpp_tests/test_moe_api.cpp) on the
GPU: launchMoeRoute on exact logits with ties, launchMoeFfn on both routes against a double loop, and LlamaModel::attachExperts /
detachExperts on a small model (one expert holding the dense matrices stays within fp16 noise of the dense model, random experts move
the rows, detaching restores the bits, a model on the per-kernel loops refuses)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "llm-inference-engine_amd", "cpp_tests")


def test_moe_cpp_driver():
    path = os.path.join(BIN, "test_moe_api")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", BIN, "test_moe_api"])
    r = subprocess.run([path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "all passed" in r.stdout and "FAIL" not in r.stdout
    for what in ("MoeRoute expert ids", "MoeRoute weights", "MoeRoute case has an exact tie", "MoeFfn grouped route", "MoeFfn GEMV route",
                 "LlamaModel one expert with the dense matrices, prefill", "LlamaModel one expert with the dense matrices, decode",
                 "LlamaModel experts, two runs agree, prefill", "LlamaModel experts, two runs agree, decode",
                 "LlamaModel experts move the hidden rows", "LlamaModel experts give finite rows", "LlamaModel detached experts, prefill",
                 "LlamaModel detached experts, decode", "LlamaModel one expert entry per layer is required",
                 "LlamaModel without the fused engine refuses experts"):
        assert what + " passed" in r.stdout, (what, r.stdout[-3000:])
