"""Runs the C++ driver of the sliding-window entries of the API mirror (llm-inference-engine_amd/cpp_tests/test_window_api.cpp) on the
GPU: launchDecoderWindowAttention against a plain loop over NaN-filled dead rows, launchKvWindowAdvance on rows whose outcome is known
by hand, and LlamaModel::setAttentionWindow on a small model (a window over the context and a cleared window give the bits of a
model without one, rows inside the first window keep theirs, later rows move, a model on the per-kernel loops refuses)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "llm-inference-engine_amd", "cpp_tests")


def test_window_cpp_driver():
    path = os.path.join(BIN, "test_window_api")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", BIN, "test_window_api"])
    r = subprocess.run([path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "all passed" in r.stdout and "FAIL" not in r.stdout
    for what in ("DecoderWindowAttention W=17 S=3 over NaN dead rows", "DecoderWindowAttention window 0 is full attention",
                 "DecoderWindowAttention append (windowed)", "KvWindowAdvance table", "KvWindowAdvance status",
                 "LlamaModel window over the context, prefill", "LlamaModel window over the context, decode",
                 "LlamaModel rows inside the first window keep their bits", "LlamaModel rows behind the window move",
                 "LlamaModel local + global layers differ from all-local and all-global", "LlamaModel cleared window, prefill",
                 "LlamaModel cleared window, decode", "LlamaModel one window per layer is required",
                 "LlamaModel without the fused engine refuses a window"):
        assert what + " passed" in r.stdout, (what, r.stdout[-3000:])
