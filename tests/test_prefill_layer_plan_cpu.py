"""What one layer of a prefill pass launches, asserted without a GPU through llmie_decoder_prefill_layer_plan (pure host code).

tests/golden/prefill_layer_plans.txt was recorded from llmie_decoder_prefill as it stood before plan_prefill_layer and plan_prefill_attn
existed: a scratch build of that commit's engine.hip and prefill.hip with a dry-run probe at every branch site of the ladders in
PrefillPass (qkv_proj, gate_up, the four sequences) and in prefill_attention_f16 -- each site noted its name (the flash launch: its
template arguments and grid) instead of launching, every launcher behind them was a no-op, TIMED counted the launches of one pass
through the layer loop, and the switches came from a mask instead of the environment -- run through the real llmie_decoder_prefill on a
host-only, one-layer llmie_decoder filled from the config, with made-up addresses whose residues follow the call flags (a misaligned
matrix or hidden state 8 bytes off, int4 scales 2 bytes off, the QKV bias 4 bytes off, the gate/up scales 8 bytes off).  The probe was
not committed.  plan_prefill + plan_prefill_layer + plan_prefill_attn, through the query, must reproduce the recording exactly.

Layout of the fixture, everything in order of first use: `refusal rN : <error text>`; `layer yN : <the plan text without its attention
part>`; `pattern pN : <answers of one call description over its token counts, run-length coded value*count>`, an answer being a layer
yN or a refusal rN; `attn <heads> <cache> <shape> : <attention part over the shape's token counts>` -- the attention launch reads the
head count, the cache format, the batch shape and rope_done only, which recording() asserts, so it is listed once per such key with
rope_append = 1 - rope_done left out; then per engine one line with the pattern of every call description, run-length coded as well.
"""
import ctypes as C
import itertools
import os

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prefill_layer_plans.txt")

W_F16, W_INT8, W_INT4, W_FP8 = 0, 1, 2, 3
FORMATS = [("f16", W_F16, 128), ("int8", W_INT8, 128), ("int4g128", W_INT4, 128), ("int4g64", W_INT4, 64), ("fp8", W_FP8, 128)]
GEOMETRIES = [(32, 32, 128, 11008), (32, 8, 128, 11008), (16, 16, 128, 3072), (16, 4, 128, 1024), (8, 8, 128, 1376), (3, 1, 128, 1000),
              (9, 3, 128, 1000)]
ENGINE_FLAGS = [("default", 0), ("packed_only", 2)]
TOKENS = [1, 8, 64, 65, 128, 129, 191, 192, 193, 300, 512, 513, 1024, 2048, 4096]
# batch shapes that reach the three forms of the flash kernel: name, token counts, (batch, max_q_len) of a token count
SHAPES = [("one", TOKENS, lambda T: (1, T)),
          ("eight_le512", [T for T in TOKENS if T >= 8], lambda T: (8, (T + 7) // 8)),
          ("two_gt512", [T for T in TOKENS if T >= 1024], lambda T: (2, T * 5 // 8))]
# call flags / switch mask of llmie_decoder_prefill_layer_plan (include/llmie.h)
PAGED, RAGGED, HIDDEN_MISALIGNED, WEIGHTS_MISALIGNED, GAMMAS_MISALIGNED, O_BIAS, SCALES_MISALIGNED = 1, 2, 4, 8, 16, 32, 64
QKV_BIAS_MISALIGNED, GATE_UP_SCALES_MISALIGNED, NO_FFN_GAMMA = 128, 256, 512
SW_NO_FUSED_SHORT_PREFILL, SW_NO_QKV_ROPE_FUSION = 16, 32
CALL_FLAGS = [PAGED, RAGGED, HIDDEN_MISALIGNED, WEIGHTS_MISALIGNED, GAMMAS_MISALIGNED, O_BIAS, SCALES_MISALIGNED, QKV_BIAS_MISALIGNED,
              GATE_UP_SCALES_MISALIGNED, NO_FFN_GAMMA]
# (shape, e4m3 cache, call flags, switch mask): every shape on both caches; each flag and each switch alone on one sequence
CALLS = [(s, kv, 0, 0) for s in range(len(SHAPES)) for kv in (0, 1)] + [(0, 0, f, 0) for f in CALL_FLAGS] + \
        [(0, 0, 0, SW_NO_FUSED_SHORT_PREFILL), (0, 0, 0, SW_NO_QKV_ROPE_FUSION)]
MAX_BATCH, MAX_SEQ = 8, 4096


def _config(llmie, fmt, group, geom, flags, kv_fmt=0):
    nh, kvh, hs, inter = geom
    return llmie.DecoderConfig(head_num=nh, kv_head_num=kvh, head_size=hs, inter_size=inter, num_layers=2, vocab_size=32000,
                               max_seq_len=MAX_SEQ, max_batch=MAX_BATCH, rotary_dim=hs, rotary_base=10000.0, rms_eps=1e-5, dtype=1,
                               wfmt=fmt, int4_group=group, kv_fmt=kv_fmt, k_scale=0.0, v_scale=0.0, flags=flags)


def ctypes_plan(lib, fn):
    """plan(cfg, tokens, batch, max_q_len, call_flags, switch_mask) -> (text or None, status, error text) over a C function with
    llmie_decoder_prefill_layer_plan's signature"""
    fn.restype = C.c_char_p
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_void_p]

    def plan(cfg, *args):
        status = C.c_int(0)
        t = fn(C.addressof(cfg), *args, C.addressof(status))
        return (t.decode(), 0, "") if t is not None else (None, status.value, lib.llmie_last_error().decode())
    return plan


def split_plan(text):
    """(layer part, attention part, rope_done) of a plan text"""
    words = text.split(" ")
    attn = [w for w in words if w.split("=")[0] in ("attn", "kv", "grid", "rope_append")]
    f = dict(w.split("=") for w in words if "=" in w)
    assert len(attn) == 4 and int(f["rope_append"]) == 1 - int(f["rope_done"]), text
    return " ".join(w for w in words if w not in attn), " ".join(attn[:3]), int(f["rope_done"])


def _rle(values):
    out = []
    for v in values:
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return " ".join("%s*%d" % (v, n) for v, n in out)


def grid(llmie):
    """(engine name, [(call, [(config, tokens, batch, max_q_len, call flags, switch mask)])]) of every engine"""
    for (fname, fmt, group), geom, (flname, flags) in itertools.product(FORMATS, GEOMETRIES, ENGINE_FLAGS):
        cfgs = [_config(llmie, fmt, group, geom, flags, kv) for kv in (0, 1)]
        yield "%s %d/%d/%d/%d %s" % ((fname,) + geom + (flname,)), geom[0], \
            [((s, kv), [(cfgs[kv], T) + SHAPES[s][2](T) + (cf, sw) for T in SHAPES[s][1]]) for s, kv, cf, sw in CALLS]


def recording(llmie, plan):
    """the fixture's lines, in its order"""
    refusals, layers, patterns, attn, lines = {}, {}, {}, {}, []
    for engine, heads, calls in grid(llmie):
        ids = []
        for (s, kv), points in calls:
            answers = []
            for i, point in enumerate(points):
                text, status, err = plan(*point)
                if text is None:
                    assert status != 0
                    answers.append(refusals.setdefault(err, "r%d" % len(refusals)))
                    continue
                layer, a, rope_done = split_plan(text)
                answers.append(layers.setdefault(layer, "y%d" % len(layers)))
                # the attention launch reads nothing else of the call
                assert attn.setdefault((heads, kv, s, i, rope_done), a) == a, (engine, point[1:], a)
            ids.append(patterns.setdefault(_rle(answers), "p%d" % len(patterns)))
        lines.append("engine %s : %s" % (engine, _rle(ids)))
    table = []
    for heads, kv, s in sorted({k[:3] for k in attn}):
        # per token count: the launch behind an unfused QKV projection; it is the same behind a fused one (asserted)
        row = []
        for i in range(len(SHAPES[s][1])):
            forms = {attn[k] for k in attn if k[:4] == (heads, kv, s, i)}
            assert len(forms) == 1, (heads, kv, s, i, forms)
            row.append(forms.pop().replace(" ", ","))
        table.append("attn %d %s %s : %s" % (heads, "e4m3" if kv else "native", SHAPES[s][0], _rle(row)))
    return ["refusal %s : %s" % (r, t) for t, r in refusals.items()] + ["layer %s : %s" % (y, t) for t, y in layers.items()] + \
           ["pattern %s : %s" % (p, v) for v, p in patterns.items()] + table + lines


def _fixture():
    return [line.rstrip("\n") for line in open(FIXTURE) if line.strip() and not line.startswith("#")]


@pytest.fixture(scope="module")
def built(llmie):
    llmie.build()
    return llmie


def test_layer_plans_reproduce_the_recording(built):
    lib = built.lib()
    got, exp = recording(built, ctypes_plan(lib, lib.llmie_decoder_prefill_layer_plan)), _fixture()
    keys = lambda lines: [l.split(" : ")[0] for l in lines if l.startswith(("attn", "engine"))]
    assert keys(got) == keys(exp), "the grid of the fixture is not the grid of this test"
    wrong = ["recorded %s\n    planned  %s" % (e, g) for e, g in itertools.zip_longest(exp, got) if e != g]
    assert not wrong, "%d of %d lines differ:\n%s" % (len(wrong), len(exp), "\n".join(wrong[:20]))


def test_path_is_the_pass_planners_and_refusals_carry_a_text(built):
    lib = built.lib()
    plan = ctypes_plan(lib, lib.llmie_decoder_prefill_layer_plan)
    planned = refused = 0
    for engine, heads, calls in grid(built):
        for _, points in calls:
            for cfg, T, batch, mq, cf, sw in points:
                text, status, err = plan(cfg, T, batch, mq, cf, sw)
                name = lib.llmie_decoder_plan_name(C.byref(cfg), 1, T, cf & 127, sw)
                if text is None:
                    refused += 1
                    assert status < 0 and len(err) > 20 and name is None, (engine, T, batch, mq, cf, sw, err)
                else:
                    planned += 1
                    assert name is not None and text.split(" ")[0] == name.decode(), (engine, T, batch, mq, cf, sw, text)
    assert planned > 10000 and refused > 1000
    # a shape the entry point refuses is refused with its words
    cfg = _config(built, W_F16, 128, GEOMETRIES[0], 0)
    assert plan(cfg, 64, 1, 32, 0, 0)[0] is None and "num_tokens > batch*max_q_len" in plan(cfg, 64, 1, 32, 0, 0)[2]
    assert plan(cfg, 64, 1, 64, 0, 0)[0].startswith("short_splitk token_table=0 attn_norm=none qkv=splitk_rope ")
