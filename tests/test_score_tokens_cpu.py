"""llmie_score_tokens on the host side of the C ABI: every refusal answers with its status and a message before anything touches
the GPU, and the workspace stays far below one byte per logit (no compute here)."""
import ctypes as C

import pytest

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4
F32, F16 = 0, 1
ROWS, H, V = 4, 128, 1003


@pytest.fixture(scope="module")
def lib(llmie):
    llmie.build()
    return llmie.lib()


def _call(lib, **over):
    """a well-formed call on addresses that are never dereferenced (every case below is refused on the host), one thing changed"""
    p = C.c_void_p(4096)
    a = dict(hidden=p, gamma=p, eps=1e-5, lm_head=p, bias=None, targets=p, out_logprob=p, out_lse=None, out_argmax=None,
             out_argmax_logprob=None, rows=ROWS, hidden_size=H, vocab=V, workspace=p, workspace_bytes=None, dtype=F16)
    a.update(over)
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = lib.llmie_score_tokens_workspace_bytes(max(a["rows"], 1), a["hidden_size"], a["vocab"])
    return lib.llmie_score_tokens(a["hidden"], a["gamma"], a["eps"], a["lm_head"], a["bias"], a["targets"], a["out_logprob"],
                                  a["out_lse"], a["out_argmax"], a["out_argmax_logprob"], a["rows"], a["hidden_size"], a["vocab"],
                                  a["workspace"], a["workspace_bytes"], a["dtype"], None)


@pytest.mark.parametrize("name", ["hidden", "lm_head", "targets", "out_logprob"])
def test_null_required_pointer_is_invalid_arg(lib, name):
    assert _call(lib, **{name: None}) == INVALID
    assert b"score_tokens" in lib.llmie_last_error()


@pytest.mark.parametrize("over", [dict(rows=0), dict(rows=-3), dict(vocab=0)])
def test_bad_shape_is_invalid_arg(lib, over):
    assert _call(lib, **over) == INVALID
    assert b"score_tokens" in lib.llmie_last_error() and b"shape" in lib.llmie_last_error()


def test_hidden_not_a_multiple_of_64_is_unsupported(lib):
    assert _call(lib, hidden_size=100) == UNSUPPORTED
    assert b"100" in lib.llmie_last_error()


@pytest.mark.parametrize("name", ["hidden", "lm_head"])
def test_misaligned_operand_is_unsupported(lib, name):
    assert _call(lib, **{name: C.c_void_p(4096 + 8)}) == UNSUPPORTED
    assert b"aligned" in lib.llmie_last_error()


def test_fp32_is_unsupported(lib):
    assert _call(lib, dtype=F32) == UNSUPPORTED
    assert b"score_tokens" in lib.llmie_last_error() and b"dtype" in lib.llmie_last_error()


def test_short_or_missing_workspace(lib):
    need = lib.llmie_score_tokens_workspace_bytes(ROWS, H, V)
    assert need >= ROWS * H * 2
    assert _call(lib, workspace_bytes=need - 1) == WORKSPACE
    assert str(need).encode() in lib.llmie_last_error()
    assert _call(lib, workspace=None) == WORKSPACE
    assert b"workspace" in lib.llmie_last_error()


def test_workspace_is_far_below_one_byte_per_logit(lib, llmie):
    rows, hidden, vocab = 2048, 4096, 32000
    need = lib.llmie_score_tokens_workspace_bytes(rows, hidden, vocab)
    assert need == llmie.score_tokens_workspace_bytes(rows, hidden, vocab)
    assert rows * hidden * 2 <= need < rows * vocab
    # O(rows * (H + spans)): beyond the normalised rows, a fixed number of partials per row whatever the vocabulary
    per_row = (need - rows * hidden * 2) / rows
    assert 0 < per_row <= 4096
    big = lib.llmie_score_tokens_workspace_bytes(rows, hidden, 8 * vocab)
    assert (big - rows * hidden * 2) / rows <= 4096
    assert lib.llmie_score_tokens_workspace_bytes(0, hidden, vocab) == 0


def test_python_table_and_header_agree(llmie):
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "llmie.h")).read()
    for name in ("llmie_score_tokens", "llmie_score_tokens_workspace_bytes"):
        assert name in llmie.EXPORTS
        assert re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    assert "#define LLMIE_ABI_VERSION 3" in txt
