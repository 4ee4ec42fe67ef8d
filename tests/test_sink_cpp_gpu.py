"""Runs the C++ driver of the head-sink and RoPE-scaling entries of the API mirror (llm-inference-engine_amd/cpp_tests/test_sink_api.cpp)
on the GPU: launchDecoderSinkAttention against a plain loop with one extra softmax column per head (full attention and windowed; null
sinks and sinks of -inf give the bits of launchDecoderWindowAttention), and LlamaModel::setAttentionSinks / setRopeScaling on a small
model (sinks of -inf, cleared sinks and a restored table give the bits of a model without them; real sinks and a YaRN table move the
rows; a bad struct and a model on the per-kernel loops are refused)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "llm-inference-engine_amd", "cpp_tests")


def test_sink_cpp_driver():
    path = os.path.join(BIN, "test_sink_api")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", BIN, "test_sink_api"])
    r = subprocess.run([path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "all passed" in r.stdout and "FAIL" not in r.stdout
    for what in ("DecoderSinkAttention full attention", "DecoderSinkAttention W=17 S=3", "DecoderSinkAttention the sinks matter",
                 "DecoderSinkAttention the sinks matter (windowed)", "DecoderSinkAttention null sinks are the window launcher's bits",
                 "DecoderSinkAttention sinks of -inf are the window launcher's bits (windowed)", "LlamaModel sinks of -inf, prefill",
                 "LlamaModel sinks of -inf, decode", "LlamaModel head sinks move the rows", "LlamaModel cleared sinks, prefill",
                 "LlamaModel cleared sinks, decode", "LlamaModel a scaled table moves the rows", "LlamaModel table restored, prefill",
                 "LlamaModel table restored, decode", "LlamaModel a factor below 1 is refused",
                 "LlamaModel without the fused engine refuses sinks and scaling"):
        assert what + " passed" in r.stdout, (what, r.stdout[-3000:])
