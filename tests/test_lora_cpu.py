"""Host side of the multi-LoRA entries (no GPU): exports and signatures, every refusal with its code and message, the size queries
against the formulas of include/llmie.h, and the planners' answers under LLMIE_PLAN_LORA.  Nothing here launches: every call is
refused on the host, or is a pure host query."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

import test_decoder_plan_cpu as dp
import test_prefill_layer_plan_cpu as pl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "llm-inference-engine_amd")
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
FAKE = 4096   # an aligned non-NULL "device pointer": every call below is refused before anything is dereferenced
PLAN_LORA = 1024


@pytest.fixture(scope="module")
def lib(llmie):
    llmie.build()
    return llmie.lib()


def test_exports_signatures_and_constants(lib, llmie):
    vp, i, sz = C.c_void_p, C.c_int, C.c_size_t
    want = {
        "llmie_lora_table_bytes": [i, i],
        "llmie_lora_slot_load": [vp, i, i, i, vp, vp],
        "llmie_lora_workspace_bytes": [i, i, i],
        "llmie_lora_plan": [vp, vp, i, i, vp, i, vp, sz, vp],
        "llmie_lora_apply": [vp, vp, i, i, i, i, vp, vp, i, i, i, i, vp, sz, i, vp],
        "llmie_decoder_lora_workspace_bytes": [vp, i, i],
        "llmie_decoder_lora_attach": [vp, vp, i, vp, vp, sz],
        "llmie_decoder_lora_detach": [vp],
    }
    for name, args in want.items():
        assert name in llmie.EXPORTS
        assert getattr(lib, name).argtypes == args, name
    for name in ("llmie_lora_table_bytes", "llmie_lora_workspace_bytes", "llmie_decoder_lora_workspace_bytes"):
        assert getattr(lib, name).restype is sz
    hdr = open(os.path.join(ROOT, "include", "llmie.h")).read()
    assert "#define LLMIE_PLAN_LORA 1024u" in hdr and llmie.PLAN_LORA == PLAN_LORA
    assert "#define LLMIE_LORA_MAX_SLOTS %d" % llmie.LORA_MAX_SLOTS in hdr and "#define LLMIE_LORA_MAX_KSPLIT %d" % llmie.LORA_MAX_KSPLIT in hdr
    assert "#define LLMIE_ABI_VERSION 3" in hdr
    for mo, name in enumerate(llmie.LORA_MODULES):
        assert "#define LLMIE_LORA_%s %d" % (name.upper(), mo) in hdr
    for fn in ("lora_table", "lora_slot_load", "lora_plan", "lora_apply", "lora_workspace_bytes"):
        assert callable(getattr(llmie, fn))
    assert callable(llmie.Decoder.lora_attach) and callable(llmie.Decoder.lora_detach)


def _align(v):
    return (v + 255) // 256 * 256


def test_size_queries_follow_their_formulas(lib, llmie):
    for slots, layers in ((1, 1), (4, 2), (64, 32), (1024, 80)):
        assert lib.llmie_lora_table_bytes(slots, layers) == slots * (16 + 64 * layers)
    for bad in ((0, 2), (2, 0), (-1, 2), (1025, 2)):
        assert lib.llmie_lora_table_bytes(*bad) == 0
    for rows, slots, rt in ((1, 1, 64), (5, 4, 192), (130, 6, 128), (2048, 64, 192), (33, 1024, 64)):
        tiles = rows // 16 + min(slots, rows)
        want = 256 + _align(4 * rows) + _align(4 * tiles) + _align(64 * tiles) + _align(8 * tiles * 16 * rt * 4)
        assert lib.llmie_lora_workspace_bytes(rows, slots, rt) == want, (rows, slots, rt)
    for bad in ((0, 4, 64), (5, 0, 64), (5, 4, 0), (5, 4, 193), (5, 1025, 64)):
        assert lib.llmie_lora_workspace_bytes(*bad) == 0
    cfg = dp._config(llmie, dp.W_F16, 128, (32, 32, 128, 11008), 8, 0)
    assert lib.llmie_decoder_lora_workspace_bytes(C.byref(cfg), 2048, 16) == lib.llmie_lora_workspace_bytes(2048, 16, 192)
    assert lib.llmie_decoder_lora_workspace_bytes(C.byref(cfg), 3, 16) == lib.llmie_lora_workspace_bytes(8, 16, 192)   # max_batch rows at least
    assert lib.llmie_decoder_lora_workspace_bytes(C.byref(cfg), 0, 16) == 0
    # the engine's own size queries keep their values: they do not know about adapters (recorded in tests/golden/decoder_paths.txt)


def _err(lib):
    return lib.llmie_last_error().decode()


def _apply(lib, **kw):
    a = dict(x=FAKE, y=FAKE, rows=5, K=64, N=32, blocks=2, widths=(16, 16), table=FAKE, slots=4, layers=2, layer=1, module=0, ws=FAKE * 16,
             ws_bytes=1 << 30, dtype=1)
    a.update(kw)
    w = (C.c_int * max(len(a["widths"]), 1))(*a["widths"]) if a["widths"] is not None else None
    return lib.llmie_lora_apply(a["x"], a["y"], a["rows"], a["K"], a["N"], a["blocks"], w, a["table"], a["slots"], a["layers"], a["layer"],
                                a["module"], a["ws"], a["ws_bytes"], a["dtype"], None)


APPLY_REFUSALS = [
    (dict(x=None), INVALID, "NULL pointer"), (dict(y=None), INVALID, "NULL pointer"), (dict(table=None), INVALID, "NULL pointer"),
    (dict(rows=0), INVALID, "non-positive size"), (dict(slots=0), INVALID, "non-positive size"),
    (dict(layer=2), INVALID, "layer 2"), (dict(module=4), INVALID, "module 4"), (dict(module=-1), INVALID, "module -1"),
    (dict(blocks=0, widths=()), INVALID, "0 column blocks outside [1, 3]"),
    (dict(blocks=4, widths=(16, 16, 16, 16), N=64), INVALID, "4 column blocks outside [1, 3]"),
    (dict(widths=None), INVALID, "column blocks"),
    (dict(widths=(16, 32)), INVALID, "sum to 48, not N=32"),
    (dict(widths=(32, 0)), INVALID, "column block 1 has width 0"),
    (dict(K=48), UNSUPPORTED, "K=48 is not a multiple of 32"),
    (dict(widths=(24, 8)), UNSUPPORTED, "width 24, not a multiple of 16"),
    (dict(dtype=0), UNSUPPORTED, "fp16 activations only"),
    (dict(x=FAKE + 8), UNSUPPORTED, "not 16-byte aligned"), (dict(y=FAKE + 2), UNSUPPORTED, "not 16-byte aligned"),
    (dict(slots=1025), UNSUPPORTED, "LLMIE_LORA_MAX_SLOTS"),
    (dict(ws=None), WORKSPACE, "workspace"), (dict(ws=FAKE * 16 + 16), WORKSPACE, "256-byte aligned"),
]


@pytest.mark.parametrize("kw,rc,msg", APPLY_REFUSALS)
def test_apply_refusals(lib, kw, rc, msg):
    assert _apply(lib, **kw) == rc, kw
    assert _err(lib).startswith("lora_apply:") and msg in _err(lib), _err(lib)


def test_apply_and_plan_workspace_short_by_one_byte(lib):
    need = lib.llmie_lora_workspace_bytes(5, 4, 128)
    assert _apply(lib, ws_bytes=need - 1) == WORKSPACE and str(need) in _err(lib)
    # the plan needs the fixed part only
    fixed = 256 + 256 + 256 + _align(64 * (5 // 16 + 4))
    assert lib.llmie_lora_plan(FAKE, None, 5, 5, FAKE, 4, FAKE * 16, fixed - 1, None) == WORKSPACE
    assert _err(lib).startswith("lora_plan:") and str(fixed) in _err(lib)
    assert lib.llmie_lora_plan(None, None, 5, 5, FAKE, 4, FAKE * 16, 1 << 20, None) == INVALID and "NULL pointer" in _err(lib)
    assert lib.llmie_lora_plan(FAKE, None, 5, 0, FAKE, 4, FAKE * 16, 1 << 20, None) == INVALID and "non-positive" in _err(lib)
    assert lib.llmie_lora_plan(FAKE, FAKE, 0, 5, FAKE, 4, FAKE * 16, 1 << 20, None) == INVALID and "non-positive" in _err(lib)
    assert lib.llmie_lora_plan(FAKE, None, 5, 5, FAKE, 2000, FAKE * 16, 1 << 20, None) == UNSUPPORTED and "LLMIE_LORA_MAX_SLOTS" in _err(lib)


def _adapter(llmie, rank=16, layers=2, a=FAKE, b=FAKE, scale=1.0):
    arr = (llmie.LoraLayer * layers)()
    for l in range(layers):
        for mo in range(4):
            arr[l].a[mo], arr[l].b[mo] = a, b
    return llmie.LoraAdapter(rank, scale, layers, arr), arr


def test_slot_load_refusals(lib, llmie):
    load = lib.llmie_lora_slot_load
    good, keep = _adapter(llmie)
    assert load(None, 4, 2, 0, C.byref(good), None) == INVALID and "NULL pointer" in _err(lib)
    assert load(FAKE, 0, 2, 0, C.byref(good), None) == INVALID and "non-positive" in _err(lib)
    assert load(FAKE, 4, 2, 4, C.byref(good), None) == INVALID and "slot 4 outside [0, 4)" in _err(lib)
    assert load(FAKE, 4, 2, -1, None, None) == INVALID and "slot -1" in _err(lib)
    assert load(FAKE, 2000, 2, 0, C.byref(good), None) == UNSUPPORTED and "LLMIE_LORA_MAX_SLOTS" in _err(lib)
    for rank in (0, 4, 12, 24, 128, -8):
        bad, k2 = _adapter(llmie, rank=rank)
        assert load(FAKE, 4, 2, 0, C.byref(bad), None) == INVALID and "rank %d outside {8, 16, 32, 64}" % rank in _err(lib)
    bad, k2 = _adapter(llmie, layers=3)
    assert load(FAKE, 4, 2, 0, C.byref(bad), None) == INVALID and "describes 3 layers, the table has 2" in _err(lib)
    bad, k2 = _adapter(llmie, b=None)
    assert load(FAKE, 4, 2, 0, C.byref(bad), None) == INVALID and "an A without its B" in _err(lib)
    bad, k2 = _adapter(llmie, a=FAKE + 8)
    assert load(FAKE, 4, 2, 0, C.byref(bad), None) == UNSUPPORTED and "not 16-byte aligned" in _err(lib)
    assert all(_err(lib).startswith("lora_slot_load:") for _ in (0,))


PLAN_FORMATS = [("f16", dp.W_F16, 128), ("int8", dp.W_INT8, 128), ("int4", dp.W_INT4, 128)]


def test_planners_answer_lora_under_the_flag(lib, llmie):
    plan = pl.ctypes_plan(lib, lib.llmie_decoder_prefill_layer_plan)
    for (name, fmt, group), geom, mb in itertools.product(PLAN_FORMATS, [(32, 32, 128, 11008), (16, 4, 128, 1024), (8, 8, 64, 768)], (1, 8, 32, 128)):
        cfg = dp._config(llmie, fmt, group, geom, mb, 0)
        for rows in sorted(r for r in {1, 2, 5, mb} if r <= mb):
            for extra in (0, dp.PAGED, dp.RAGGED, dp.PAGED | dp.RAGGED):
                assert dp._plan(lib, cfg, 0, rows, PLAN_LORA | extra, 0) == "lora", (name, geom, mb, rows, extra)
        if geom[2] != 128:   # prefill takes head_size 128 only, with or without adapters
            assert dp._plan(lib, cfg, 1, 64, PLAN_LORA, 0).startswith("refused:decoder_prefill: fp16 activations")
            continue
        for T in (1, 64, 129, 192, 2048):
            for extra in (0, dp.PAGED, dp.O_BIAS, dp.WEIGHTS_MISALIGNED):
                assert dp._plan(lib, cfg, 1, T, PLAN_LORA | extra, 0) == "lora", (name, geom, T, extra)
            text, status, err = plan(cfg, T, 1, T, PLAN_LORA, 0)
            assert text is not None, err
            words = dict(w.split("=") for w in text.split(" launches")[0].split(" ") if "=" in w)
            assert text.split(" ")[0] == "lora" and words["token_table"] == "0"
            assert (words["attn_norm"], words["qkv"], words["pre"], words["rope_done"], words["rope_append"]) == ("inplace", "plain", "none", "0", "1")
            assert (words["ffn_norm"], words["gate_up"]) == ("inplace", "two_launch")
            # shrink + expand behind each projection; gate/up: projection + update + llmie_silu_and_mul
            assert text.endswith("launches attn_norm=1 qkv_gemm=3 mha=1 o_gemm=3 ffn_norm=1 gate_up_swiglu=4 down_gemm=3"), text


def test_planners_refuse_fp8_and_packed_only_under_the_flag(lib, llmie):
    plan = pl.ctypes_plan(lib, lib.llmie_decoder_prefill_layer_plan)
    geom = (32, 32, 128, 11008)
    for fmt, flags, word in ((dp.W_FP8, 0, "fp8-weight engine"), (dp.W_F16, 2, "LLMIE_DEC_PACKED_ONLY"), (dp.W_INT8, 2, "LLMIE_DEC_PACKED_ONLY")):
        cfg = dp._config(llmie, fmt, 128, geom, 8, flags)
        for prefill, rows in ((0, 1), (0, 8), (1, 64), (1, 2048)):
            a = dp._plan(lib, cfg, prefill, rows, PLAN_LORA, 0)
            assert a.startswith("refused:") and "adapters need an fp16 engine" in a and word in a, a
            assert not dp._plan(lib, cfg, prefill, rows, 0, 0).startswith("refused:")
        text, status, err = plan(cfg, 64, 1, 64, PLAN_LORA, 0)
        assert text is None and status == UNSUPPORTED and "adapters need an fp16 engine" in err
    cfg = dp._config(llmie, dp.W_F32, 128, geom, 8, 0)
    assert "adapters need an fp16 engine" in dp._plan(lib, cfg, 0, 1, PLAN_LORA, 0)


def test_without_the_flag_the_recordings_are_reproduced(lib, llmie):
    """the committed recordings, re-read: the new call flag changes nothing about the answers without it"""
    got, exp = dp.recording(llmie, lib), dp._fixture()
    assert got == exp
    got, exp = pl.recording(llmie, pl.ctypes_plan(lib, lib.llmie_decoder_prefill_layer_plan)), pl._fixture()
    assert got == exp


def test_attach_refusals_on_the_host(lib):
    assert lib.llmie_decoder_lora_attach(None, FAKE, 4, FAKE, FAKE * 16, 1 << 20) == INVALID
    assert _err(lib).startswith("decoder_lora_attach:") and "NULL pointer" in _err(lib)
    assert lib.llmie_decoder_lora_detach(None) == INVALID and "NULL decoder" in _err(lib)


def test_no_new_environment_switch():
    assert "getenv" not in open(os.path.join(PKG, "csrc", "lora.hip")).read()
    assert open(os.path.join(PKG, "csrc", "engine.hip")).read().count("getenv(") == 6   # the six switches of EngineSwitches, as before


def test_cpp_driver_compiles():
    src = os.path.join(PKG, "cpp_tests", "test_lora_api.cpp")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-I", PKG, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "test_lora_api" in open(os.path.join(PKG, "cpp_tests", "Makefile")).read()
