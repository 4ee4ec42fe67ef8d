"""The C++ driver of the mirror for tree speculative decoding (cpp_tests/test_spec_tree_api.cpp): launchSpecTreePrepare,
launchSpecVerifyTree, launchKvTreeCommit, launchNgramDraftTree and LlamaModel::speculativeTreeStep."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_spec_tree_cpp_driver():
    bin_dir = os.path.join(ROOT, "llm-inference-engine_amd", "cpp_tests")
    path = os.path.join(bin_dir, "test_spec_tree_api")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", bin_dir, "test_spec_tree_api"])
    r = subprocess.run([path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "all passed" in r.stdout and "FAIL" not in r.stdout
    for what in ("SpecTreePrepare depth", "SpecTreePrepare anc", "SpecVerifyTree tokens", "SpecVerifyTree path", "SpecVerifyTree counts",
                 "SpecVerifyTree seq_len", "SpecVerifyTree finished", "SpecVerifyTree last_token", "SpecVerifyTree cached_len",
                 "SpecVerifyTree step_rows", "KvTreeCommit K rows", "KvTreeCommit V rows", "NgramDraftTree ids", "NgramDraftTree parents",
                 "NgramDraftTree node counts", "speculativeTreeStep emits the walk over its logits", "speculativeTreeStep path",
                 "speculativeTreeStep cached K rows", "speculativeTreeStep refusal"):
        assert what + " passed" in r.stdout, r.stdout[-3000:]
    assert "moved by the commit passed" in r.stdout
