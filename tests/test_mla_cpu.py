"""MLA decode attention without a GPU: llmie_mla_decode_plan / llmie_mla_decode_workspace_bytes are pure host code -- the plan text,
the grid arithmetic at the contexts tests/test_mla_gpu.py uses, and every refusal with its message."""
import re

import pytest

PLAN = re.compile(r"mla f16 nh(\d+) hb(\d+) tile(\d+) chunk(\d+) grid (\d+)x(\d+)x(\d+) merge (none|(\d+)x(\d+)/(\d+))$")


@pytest.fixture(scope="module")
def built(llmie):
    llmie.build()
    for n in ("llmie_mla_decode_workspace_bytes", "llmie_mla_kv_append", "llmie_mla_q_absorb", "llmie_mla_decode", "llmie_mla_out_project",
              "llmie_mla_decode_plan"):
        assert n in llmie.EXPORTS and hasattr(llmie.lib(), n), n
    return llmie


def parse(text):
    m = PLAN.match(text)
    assert m, text
    return dict(nh=int(m[1]), hb=int(m[2]), tile=int(m[3]), chunk=int(m[4]), grid=(int(m[5]), int(m[6]), int(m[7])), merge=m[8])


@pytest.mark.parametrize("heads", [16, 32, 128])
def test_grid_follows_the_context(built, heads):
    t, rc = built.mla_decode_plan(3, heads, 640)
    p = parse(t)
    T, C = p["tile"], p["chunk"]
    assert rc == 0 and p["hb"] >= 16 and heads % p["hb"] == 0 and 128 % T == 0 and C % T == 0
    # device-resident lengths: the grid covers max_seq_len
    assert p["grid"] == (-(-640 // C), heads // p["hb"], 3) and p["merge"] == "%dx3/128" % heads
    for ctx in (1, T - 1, T, T + 1, 128, 129, C, C + 1, 2 * C + T + 3):
        max_seq = -(-ctx // 128) * 128
        p = parse(built.mla_decode_plan(1, heads, max_seq, max_ctx=ctx)[0])
        assert p["grid"] == (-(-ctx // C), heads // p["hb"], 1), ctx
        assert (p["merge"] == "none") == (p["grid"][0] == 1), ctx
        need = built.lib().llmie_mla_decode_workspace_bytes(1, heads, ctx)
        assert need == (0 if ctx <= C else heads * -(-ctx // C) * (512 + 2) * 4)
        paged = parse(built.mla_decode_plan(1, heads, max_seq, max_ctx=ctx, paged=True, max_pages=max_seq // 128, num_pages=9)[0])
        assert paged == p   # the page table changes no launch


@pytest.mark.parametrize("kwargs,status,word", [
    (dict(head_num=8), -2, "head_num=8"), (dict(head_num=24), -2, "head_num=24"), (dict(head_num=144), -2, "head_num=144"),
    (dict(max_seq_len=0), -1, "max_seq_len"),
    (dict(paged=True, max_pages=3, num_pages=8, max_seq_len=512), -1, "max_pages=3"),
    (dict(max_seq_len=512, workspace_bytes=2 * 16 * 2 * 514 * 4 - 1), -4, "workspace"),
    (dict(max_seq_len=512, workspace_bytes=None), -4, "workspace"),
    (dict(max_seq_len=512, max_ctx=513), -1, "max_ctx"),
])
def test_refusals_carry_a_message(built, kwargs, status, word):
    call = dict(batch=2, head_num=16, max_seq_len=256)
    call.update(kwargs)
    text, rc = built.mla_decode_plan(**call)
    assert text is None and rc == status
    assert word in built.lib().llmie_last_error().decode()
