"""The launch sequence of every decode step and prefill pass, asserted without a GPU through llmie_decoder_plan_name (pure host code).

tests/golden/decoder_paths.txt was recorded from llmie_decoder_forward and llmie_decoder_prefill as they stood before the planners
existed: a scratch build of that commit with a dry-run probe at every branch site of the two ladders (each `if` body that starts a
launch sequence and each refusal returned the site's name -- or left its error text -- instead of launching; the switches came from a
mask instead of the environment), run on a host-only llmie_decoder filled from the config (pk_wf, packed_only, one layer of made-up
addresses whose alignment follows the call flags), together with the two size queries that follow the same decision.  The probe was
not committed.  plan_decode / plan_prefill, and everything that asks them, must reproduce the recording exactly.

Layout of the fixture, everything in order of first use: `refusal rN : <error text>`; `pattern pN : <answers of one call description
over the rows axis, run-length coded value*count>` -- decode: every batch <= max_batch, for each max_batch in turn; prefill: the token
counts -- an answer being a path name, a refusal rN (an engine llmie_decoder_create refuses: create's text) or `invalid` for a config
the library rejects; then per engine one line with the pattern of every call description (run-length coded as well) and the two size
queries over max_batch.
"""
import ctypes as C
import itertools
import os

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decoder_paths.txt")

W_F16, W_INT8, W_INT4, W_FP8, W_F32 = 0, 1, 2, 3, 4
FORMATS = [("f16", W_F16, 128), ("int8", W_INT8, 128), ("int4g128", W_INT4, 128), ("int4g64", W_INT4, 64), ("fp8", W_FP8, 128),
           ("f32", W_F32, 128)]
GEOMETRIES = [(32, 32, 128, 11008), (16, 4, 128, 1024), (8, 8, 64, 768), (12, 12, 32, 1000), (6, 2, 48, 768)]
MAX_BATCHES = [1, 2, 5, 8, 16, 32, 64, 128, 160]
BATCHES = [1, 2, 3, 4, 5, 6, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 160]
ENGINE_FLAGS = [("default", 0), ("no_packed_copy", 1), ("packed_only", 2)]
TOKENS = [1, 8, 64, 65, 128, 129, 191, 192, 193, 512, 2048]
PREFILL_MAX_BATCH = 8
# call flags / switch mask of llmie_decoder_plan_name (include/llmie.h)
PAGED, RAGGED, HIDDEN_MISALIGNED, WEIGHTS_MISALIGNED, GAMMAS_MISALIGNED, O_BIAS, SCALES_MISALIGNED = 1, 2, 4, 8, 16, 32, 64
SW_NO_FUSED_DECODE, SW_NO_FUSED_BATCH, SW_NO_PACKED_BATCH, SW_CHAIN, SW_NO_FUSED_SHORT_PREFILL, SW_NO_QKV_ROPE_FUSION = 1, 2, 4, 8, 16, 32
DECODE_SWITCHES = [0, SW_NO_FUSED_DECODE, SW_NO_FUSED_BATCH, SW_NO_PACKED_BATCH, SW_CHAIN]
# cache (native / e4m3) x layout (dense / paged) x call kind (plain / ragged) x hidden state (aligned / +8 bytes) x switch
DECODE_CALLS = [(kv, paged | ragged | mis, sw) for kv in (0, 1) for paged in (0, PAGED) for ragged in (0, RAGGED)
                for mis in (0, HIDDEN_MISALIGNED) for sw in DECODE_SWITCHES]
PREFILL_CALLS = [(f, 0) for f in (0, PAGED, RAGGED, HIDDEN_MISALIGNED, WEIGHTS_MISALIGNED, GAMMAS_MISALIGNED, O_BIAS, SCALES_MISALIGNED)] + \
                [(0, SW_NO_FUSED_SHORT_PREFILL), (0, SW_NO_QKV_ROPE_FUSION)]


def _config(llmie, fmt, group, geom, max_batch, flags, kv_fmt=0):
    nh, kvh, hs, inter = geom
    return llmie.DecoderConfig(head_num=nh, kv_head_num=kvh, head_size=hs, inter_size=inter, num_layers=2, vocab_size=32000,
                               max_seq_len=2048, max_batch=max_batch, rotary_dim=hs, rotary_base=10000.0, rms_eps=1e-5,
                               dtype=0 if fmt == W_F32 else 1, wfmt=fmt, int4_group=group, kv_fmt=kv_fmt, k_scale=0.0, v_scale=0.0,
                               flags=flags)


def _plan(lib, cfg, prefill, rows, call_flags, switch_mask):
    r = lib.llmie_decoder_plan_name(C.byref(cfg), prefill, rows, call_flags, switch_mask)
    if r is not None:
        return r.decode()
    text = lib.llmie_last_error().decode()
    return "invalid" if text.startswith("decoder_plan_name: invalid config") else "refused:" + text


def _rle(values):
    out = []
    for v in values:
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return " ".join("%s*%d" % (v, n) for v, n in out)


def recording(llmie, lib):
    """the fixture's lines, in its order"""
    refusals, patterns, lines = {}, {}, []

    def answer(*call):
        a = _plan(lib, *call)
        return refusals.setdefault(a[8:], "r%d" % len(refusals)) if a.startswith("refused:") else a

    def pid(values):
        return patterns.setdefault(_rle(values), "p%d" % len(patterns))

    for (fname, fmt, group), geom, (flname, flags) in itertools.product(FORMATS, GEOMETRIES, ENGINE_FLAGS):
        engine = "%s %d/%d/%d/%d %s" % ((fname,) + geom + (flname,))
        cfgs = {(mb, kv): _config(llmie, fmt, group, geom, mb, flags, kv) for mb in MAX_BATCHES for kv in (0, 1)}
        ids = [pid(answer(cfgs[mb, kv], 0, b, cf, sw) for mb in MAX_BATCHES for b in BATCHES if b <= mb) for kv, cf, sw in DECODE_CALLS]
        lines.append("decode %s : %s" % (engine, _rle(ids)))
        for query in ("llmie_decoder_workspace_bytes", "llmie_decoder_resident_weight_bytes"):
            lines.append("%s %s : %s" % (query[14:], engine, " ".join(str(getattr(lib, query)(C.byref(cfgs[mb, 0]))) for mb in MAX_BATCHES)))
        cfg = _config(llmie, fmt, group, geom, PREFILL_MAX_BATCH, flags)
        ids = [pid(answer(cfg, 1, T, cf, sw) for T in TOKENS) for cf, sw in PREFILL_CALLS]
        lines.append("prefill %s : %s" % (engine, _rle(ids)))
    return ["refusal %s : %s" % (r, t) for t, r in refusals.items()] + ["pattern %s : %s" % (p, v) for v, p in patterns.items()] + lines


def _fixture():
    return [line.rstrip("\n") for line in open(FIXTURE) if line.strip() and not line.startswith("#")]


@pytest.fixture(scope="module")
def built(llmie):
    llmie.build()
    return llmie


def test_plans_and_sizes_reproduce_the_recording(built):
    got, exp = recording(built, built.lib()), _fixture()
    keys = lambda lines: [l.split(" : ")[0] for l in lines if not l.startswith(("pattern", "refusal"))]
    assert keys(got) == keys(exp), "the grid of the fixture is not the grid of this test"
    wrong = ["recorded %s\n    planned  %s" % (e, g) for e, g in itertools.zip_longest(exp, got) if e != g]
    assert not wrong, "%d of %d lines differ:\n%s" % (len(wrong), len(exp), "\n".join(wrong[:20]))


def test_every_refusal_comes_with_an_error_text(built):
    lib, refused = built.lib(), 0
    for (fname, fmt, group), geom, (flname, flags) in itertools.product(FORMATS, GEOMETRIES, ENGINE_FLAGS):
        for mb in (2, 32, 160):
            for kv, cf, sw in DECODE_CALLS:
                cfg = _config(built, fmt, group, geom, mb, flags, kv)
                for b in (1, mb):
                    if lib.llmie_decoder_plan_name(C.byref(cfg), 0, b, cf, sw) is None:
                        refused += 1
                        assert len(lib.llmie_last_error()) > 20, (fname, geom, flname, mb, kv, cf, sw, b)
        cfg = _config(built, fmt, group, geom, PREFILL_MAX_BATCH, flags)
        for cf, sw in PREFILL_CALLS:
            if lib.llmie_decoder_plan_name(C.byref(cfg), 1, 64, cf, sw) is None:
                refused += 1
                assert len(lib.llmie_last_error()) > 20, (fname, geom, flname, cf, sw)
    assert refused > 100
    # rows outside the engine's range are refused as the entry points refuse them
    cfg = _config(built, W_F16, 128, GEOMETRIES[0], 8, 0)
    assert lib.llmie_decoder_plan_name(C.byref(cfg), 0, 9, 0, 0) is None and b"outside [1,8]" in lib.llmie_last_error()
    assert lib.llmie_decoder_plan_name(C.byref(cfg), 0, 8, 0, 0) == b"packed"
    assert lib.llmie_decoder_plan_name(C.byref(cfg), 1, 64, 0, 0) == b"short_splitk"
