"""Runs the C++ driver of the QK-norm entries of the API mirror (llm-inference-engine_amd/cpp_tests/test_qknorm_api.cpp) on the GPU:
launchQkNorm against a plain loop, launchDecoderQkNormAttention against launchQkNorm + launchDecoderSinkAttention bit for bit (null
gammas give the sink launcher's bits), and LlamaModel::setQkNorm on a small model (the gammas move prefill and decode rows, cleared
gammas restore the bits, a model on the per-kernel loops refuses)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "llm-inference-engine_amd", "cpp_tests")


def test_qknorm_cpp_driver():
    path = os.path.join(BIN, "test_qknorm_api")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", BIN, "test_qknorm_api"])
    r = subprocess.run([path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "all passed" in r.stdout and "FAIL" not in r.stdout
    for what in ("QkNorm against a plain loop", "DecoderQkNormAttention equals QkNorm + DecoderSinkAttention",
                 "DecoderQkNormAttention null gammas are the sink launcher's bits", "DecoderQkNormAttention the norm matters",
                 "LlamaModel QK-norm moves the rows", "LlamaModel cleared gammas, prefill", "LlamaModel cleared gammas, decode",
                 "LlamaModel without the fused engine refuses QK-norm"):
        assert what + " passed" in r.stdout, (what, r.stdout[-3000:])
