"""The MLA e4m3 latent cache without a GPU: llmie_mla_decode_e4m3_plan is pure host code -- the plan text and every refusal --, and
llmie_mla_decode_e4m3 refuses a c_scale that is not positive and finite before any launch."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def built(llmie):
    llmie.build()
    for n in ("llmie_mla_kv_append_e4m3", "llmie_mla_kv_append_rows_e4m3", "llmie_mla_decode_e4m3", "llmie_mla_decode_e4m3_plan",
              "llmie_mla_cache_dequant_e4m3"):
        assert n in llmie.EXPORTS and hasattr(llmie.lib(), n), n
    return llmie


def test_plan_text(built):
    assert built.mla_decode_e4m3_plan(2, 16, 256) == ("mla e4m3 nh16 hb16 tile32 chunk256 row640 grid 1x1x2 merge none", 0)
    assert built.mla_decode_e4m3_plan(2, 128, 2048) == ("mla e4m3 nh128 hb16 tile32 chunk256 row640 grid 8x8x2 merge 128x2/128", 0)


@pytest.mark.parametrize("kwargs,status,word", [
    (dict(head_num=8), -2, "head_num=8"), (dict(head_num=144), -2, "head_num=144"),
    (dict(max_seq_len=512, max_ctx=513), -1, "max_ctx"),
    (dict(paged=True, max_pages=3, num_pages=8, max_seq_len=512), -1, "max_pages=3"),
    (dict(max_seq_len=512, workspace_bytes=2 * 16 * 2 * 514 * 4 - 1), -4, "workspace"),
])
def test_refusals_carry_a_message(built, kwargs, status, word):
    call = dict(batch=2, head_num=16, max_seq_len=256)
    call.update(kwargs)
    text, rc = built.mla_decode_e4m3_plan(**call)
    assert text is None and rc == status
    err = built.lib().llmie_last_error().decode()
    assert word in err and "mla_decode_e4m3" in err


@pytest.mark.parametrize("c_scale", [0.0, -0.5, float("inf"), float("nan")])
def test_bad_c_scale_is_refused_before_any_launch(built, c_scale):
    one = C.c_void_p(16)   # never dereferenced: the check fails first
    rc = built.lib().llmie_mla_decode_e4m3(one, one, one, 0, 1, 16, 128, 0, one, 0.1, None, 0, None, 0, 0, c_scale, None)
    assert rc == -1 and "c_scale" in built.lib().llmie_last_error().decode()
