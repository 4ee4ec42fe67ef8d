"""MLA prefill without a GPU: the plan line and its grid arithmetic, and every refusal of the planner and the entries with its message."""
import ctypes as C
import re

import pytest

PLAN = re.compile(r"mla_prefill f16 nh(\d+) q(\d+) kt(\d+) flash (\d+)x(\d+)x(\d+) up tt(\d+) hb(\d+) (\d+)x(\d+)x(\d+) append (\d+)$")


@pytest.fixture(scope="module")
def built(llmie):
    llmie.build()
    return llmie


def test_plan_line_and_its_grids(built):
    text, rc = built.mla_prefill_plan(2, 32, 200, 384, 512, total_tokens=333)
    m = PLAN.match(text)
    assert rc == 0 and m, text
    nh, Q, KT, fx, fy, fz, tt, hb, ux, uy, uz, ap = map(int, m.groups())
    assert nh == 32 and Q % 16 == 0 and 128 % KT == 0 and 128 % tt == 0 and 32 % hb == 0
    assert (fx, fy, fz) == (-(-200 // Q), 32, 2) and (ux, uy, uz) == (-(-384 // tt), 32 // hb, 2) and ap == 333
    assert built.mla_prefill_plan(2, 32, 200, 384, 512, total_tokens=333, paged=True, max_pages=4, num_pages=9) == (text, 0)


@pytest.mark.parametrize("kwargs,status,word", [
    (dict(head_num=8), -2, "head_num=8"), (dict(head_num=144), -2, "head_num=144"),
    (dict(kv_span=513), -1, "kv_span=513"), (dict(max_q_len=0), -1, "max_q_len=0"),
    (dict(paged=True, max_pages=3, num_pages=8), -1, "max_pages=3"),
])
def test_planner_refusals_carry_a_message(built, kwargs, status, word):
    call = dict(batch=2, head_num=16, max_q_len=64, kv_span=256, max_seq_len=512, total_tokens=100)
    call.update(kwargs)
    text, rc = built.mla_prefill_plan(**call)
    assert text is None and rc == status
    assert word in built.lib().llmie_last_error().decode()


@pytest.mark.parametrize("entry", ["mla_kv_append_rows", "mla_kv_up", "mla_prefill"])
def test_entries_refuse_null_operands_and_bad_shapes(built, entry):
    lib, one = built.lib(), C.c_void_p(16)   # (never dereferenced: the host checks fail first)
    calls = {
        "mla_kv_append_rows": lambda p, heads, span: lib.llmie_mla_kv_append_rows(p, one, 1e-6, one, one, 0, 2, 100, 64, span, 512, one, one, None, 0, 0, None),
        "mla_kv_up": lambda p, heads, span: lib.llmie_mla_kv_up(p, one, one, 0, 2, heads, 64, span, 512, one, one, None, 0, 0, None),
        "mla_prefill": lambda p, heads, span: lib.llmie_mla_prefill(p, one, one, one, one, 0, 2, heads, 100, 64, span, 512, one, one, 0.1, None, 0, 0, None),
    }
    assert calls[entry](None, 16, 256) == -1 and ("%s: NULL operand" % entry) in lib.llmie_last_error().decode()
    assert calls[entry](one, 16, 513) == -1 and ("%s: kv_span=513" % entry) in lib.llmie_last_error().decode()
