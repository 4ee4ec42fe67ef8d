"""MLA verify attention without a GPU: llmie_mla_verify_plan / llmie_mla_verify_workspace_bytes are pure host code -- the plan text, its
grid arithmetic, and every refusal of the planner and of the entry with its message."""
import ctypes as C
import re

import pytest

PLAN = re.compile(r"mla_verify f16 nh(\d+) rows(\d+) (chain|tree) cols (\d+)x(\d+) tile(\d+) chunk(\d+) grid (\d+)x(\d+)x(\d+) merge (none|.+/\d+)$")


@pytest.fixture(scope="module")
def built(llmie):
    llmie.build()
    return llmie


@pytest.mark.parametrize("heads", [16, 128])
@pytest.mark.parametrize("rows", [1, 2, 5, 64])
def test_grid_follows_the_rows_and_the_context(built, heads, rows):
    for max_seq, max_ctx, tree in ((640, 0, True), (640, 258, False), (256, 0, False), (384, 1, True)):
        text, rc = built.mla_verify_plan(3, rows, heads, max_seq, max_ctx=max_ctx, tree=tree)
        m = PLAN.match(text or "")
        assert rc == 0 and m, text
        hb, rb, tile, chunk = int(m[4]), int(m[5]), int(m[6]), int(m[7])
        assert (int(m[1]), int(m[2]), m[3]) == (heads, rows, "tree" if tree else "chain")
        assert hb == 16 and rb >= 2 and 128 % tile == 0 and chunk % tile == 0
        splits = -(-(max_ctx or max_seq) // chunk)
        assert (int(m[8]), int(m[9]), int(m[10])) == (splits, heads // hb, 3 * -(-rows // rb))
        assert m[11] == ("none" if splits == 1 else "%dx%d/128" % (heads, 3 * rows))
        need = built.lib().llmie_mla_verify_workspace_bytes(3, rows, heads, max_ctx or max_seq)
        assert need == (0 if splits == 1 else 3 * rows * heads * splits * (512 + 2) * 4)
        paged = built.mla_verify_plan(3, rows, heads, max_seq, max_ctx=max_ctx, tree=tree, paged=True, max_pages=5, num_pages=9)
        assert paged == (text, 0)   # the page table changes no launch


@pytest.mark.parametrize("kwargs,status,word", [
    (dict(rows=0), -1, "rows=0"), (dict(rows=65), -2, "rows=65"), (dict(head_num=8), -2, "head_num=8"),
    (dict(paged=True, max_pages=3, num_pages=8, max_seq_len=512), -1, "max_pages=3"),
    (dict(max_seq_len=512, workspace_bytes=2 * 4 * 16 * 2 * 514 * 4 - 1), -4, "workspace"),
    (dict(max_seq_len=512, workspace_bytes=None), -4, "workspace"),
    (dict(max_seq_len=512, max_ctx=513), -1, "max_ctx"),
])
def test_refusals_carry_a_message(built, kwargs, status, word):
    call = dict(batch=2, rows=4, head_num=16, max_seq_len=256)
    call.update(kwargs)
    assert built.mla_verify_plan(**call) == (None, status)
    assert word in built.lib().llmie_last_error().decode()
    # the entry itself: the same planner behind the pointer checks (never-dereferenced pointers: every call here is refused)
    one, ws = C.c_void_p(16), call.get("workspace_bytes", 0)
    rc = built.lib().llmie_mla_verify(one, one, one, 0, call["batch"], call["rows"], call["head_num"], call["max_seq_len"], call.get("max_ctx", 0),
                                      one, None, None, 0.1, one if ws else None, ws or 0, one if call.get("paged") else None,
                                      call.get("max_pages", 0), call.get("num_pages", 0), None)
    assert rc == status and word in built.lib().llmie_last_error().decode()
    assert built.lib().llmie_mla_verify(one, None, one, 0, 1, 2, 16, 128, 0, one, None, None, 0.1, None, 0, None, 0, 0, None) == -1
    assert "NULL operand" in built.lib().llmie_last_error().decode()
