"""LlamaModel::SamplingConfig (api/model.hpp) on the GPU: the C++ driver cpp_tests/test_sampling_config.cpp runs the
dummy-weight model's chat flow with greedy, top-1, seeded and default configs (fp16 and fp32)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "llm-inference-engine_amd", "cpp_tests")


@pytest.mark.gpu
def test_sampling_config_driver():
    path = os.path.join(BIN, "test_sampling_config")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", BIN, "test_sampling_config"])
    r = subprocess.run([path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "all passed" in r.stdout
