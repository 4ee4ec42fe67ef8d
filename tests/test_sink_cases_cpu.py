"""The tests of the head-sink tests (tests/sink_attn_cases.py) and the host side of the head-sink / RoPE-scaling entries: no GPU.

  - every seeded defect of sink_attn_cases.DEFECTS lies at least 10 bounds from the reference on every case it applies to, decode and
    prefill: a kernel with that defect cannot pass the GPU tests;
  - llmie_rope_table_fill against a float64 numpy restatement of the formulas of include/llmie.h (gpt-oss YaRN with and without
    truncation, Llama-3.1, linear, a partial rotary_dim, lo == hi), kind NONE bit for bit against attn_cases.rope_table (evaluated
    with numpy's SIMD kernels off) and against the engine's fp32 formula evaluated with the C library, every scaled table far from the
    unscaled one below position 64;
  - every host refusal of the new entries, and the plan texts with and without the new bits.
"""
import ctypes as C
import ctypes.util
import os
import subprocess
import sys

import numpy as np
import pytest

import attn_cases as ac
import sink_attn_cases as sc
import window_attn_cases as wc

BOUNDS = ac.BOUNDS["rope"][ac.F16]


# ------------------------------------------------------------------------------------------------------------ the decode cases
def _decode_cases():
    for cid, geo, W, S in sc.decode_cases():
        chunk = ac.chunk_len(ac.F16, geo[1], e4m3=geo[4] is not None)
        for i, steps in enumerate(sc.step_sets(chunk)):
            yield "%s-set%d" % (cid, i), sc.build(geo, W, S, steps, chunk, sc.max_seq_of(chunk), shift=2 - i)


@pytest.fixture(scope="module")
def decode_cases():
    return list(_decode_cases())


def test_the_step_sets_give_the_split_counts(decode_cases):
    """1 (the direct store), 2, 16 and 17 (a second merge round) splits per sequence without a window; bounded by it with one"""
    seen = set()
    for cid, c in decode_cases:
        n = [len(wc.live_chunks(s, c.W, c.S, c.chunk)) for s in c.steps]
        if c.W == 0:
            seen |= set(n)
        else:
            assert max(n) <= wc.live_bound(c.max_seq, c.W, c.S, c.chunk), cid
    assert seen == {1, 2, 16, 17}, seen


def test_every_class_is_met_and_a_group_mixes_them(decode_cases):
    met = set()
    for cid, c in decode_cases:
        met |= {c.sink_cls[h] for b in range(c.bs) for h in range(c.nh) if c.pos[b][h] is not None}
        for g in range(c.kvh):
            cls = c.sink_cls[g * c.rep:(g + 1) * c.rep]
            assert all(a != b for a, b in zip(cls, cls[1:])), (cid, cls)
            assert c.rep > len(sc.CLASSES) or len(set(cls)) == c.rep, (cid, cls)
        assert "half" in c.sink_cls, cid
    assert met == set(sc.CLASSES), met


def test_minus_infinity_is_the_plain_reference(decode_cases):
    for cid, c in decode_cases[:6]:
        assert np.array_equal(sc.attend(c, np.full(c.nh, -np.inf)), c.ref_plain), cid


@pytest.mark.parametrize("defect", sc.DEFECTS)
def test_decode_defects_are_far_from_the_reference(decode_cases, defect):
    applied = 0
    for cid, c in decode_cases:
        if not sc.applies(c, defect):
            continue
        applied += 1
        d = sc.distance(c, sc.attend(c, c.sink, defect), BOUNDS)
        assert d >= 10.0, "%s: defect %s lies only %.3g bounds from the reference" % (cid, defect, d)
    assert applied >= 6, (defect, applied)


# ----------------------------------------------------------------------------------------------------------- the prefill cases
@pytest.fixture(scope="module")
def prefill_cases():
    out = []
    for kv in ("f16", "np2"):
        for i, (W, S) in enumerate(((0, 0), (5, 0), (100, 4))):
            out.append(sc.make_prefill_case("sink-%s-W%d-S%d" % (kv, W, S), 8, 2, wc.PREFILL_LENS, wc.PREFILL_HIST, kv, "q64w4t1", W, S, shift=i))
    return out


@pytest.mark.parametrize("defect", ["missing", "per_lane", "group_div", "group_mod"])
def test_prefill_defects_are_far_from_the_reference(prefill_cases, defect):
    import prefill_attn_cases as pc
    for c in prefill_cases:
        wrong = sc.prefill_reference(c, c.deq(c.k_cpu, 0), c.deq(c.v_cpu, 1), c.sink, defect)
        rtol, atol = pc.BOUND
        worst = max(float((np.abs(wrong[s] - c.ref[s]) / (atol + rtol * np.abs(c.ref[s]) + c.extra_atol(s))).max()) for s in range(c.bs))
        assert worst >= 10.0, "W=%d S=%d kv=%s: defect %s lies only %.3g bounds from the reference" % (c.W, c.S, c.kv, defect, worst)


def test_prefill_minus_infinity_is_the_plain_reference(prefill_cases):
    for c in prefill_cases:
        plain = sc.prefill_reference(c, c.deq(c.k_cpu, 0), c.deq(c.v_cpu, 1), np.full(c.nh, -np.inf))
        assert all(np.array_equal(a, b) for a, b in zip(plain, c.ref_plain))


# ------------------------------------------------------------------------------------------------------------------ rope_table
def rope_restatement(max_pos, hs, rot, base, s):
    """float64 numpy restatement of the scaled kinds of include/llmie.h -> ([max_pos, hs/2, 2] float64, attention factor)"""
    j = np.arange(rot // 2, dtype=np.float64)
    f = np.float64(np.float32(base)) ** (-2.0 * j / rot)
    factor, orig, attn = np.float64(np.float32(s["factor"])), float(s.get("original_max_pos", 0)), 1.0
    if s["kind"] == "linear":
        g = f / factor
    elif s["kind"] == "llama3":
        lf, hf = np.float64(np.float32(s["low_freq_factor"])), np.float64(np.float32(s["high_freq_factor"]))
        w = 2 * np.pi / f
        t = (orig / w - lf) / (hf - lf)
        g = np.where(w > orig / lf, f / factor, np.where(w < orig / hf, f, (1 - t) * f / factor + t * f))
    else:
        bf, bs = float(np.float32(s.get("beta_fast", 0))) or 32.0, float(np.float32(s.get("beta_slow", 0))) or 1.0
        corr = lambda n: rot * np.log(orig / (2 * np.pi * n)) / (2 * np.log(np.float64(np.float32(base))))
        lo, hi = corr(bf), corr(bs)
        if s.get("truncate"):
            lo, hi = np.floor(lo), np.ceil(hi)
        lo, hi = max(lo, 0.0), min(hi, rot - 1.0)
        if lo == hi:
            hi += 0.001
        ramp = np.clip((j - lo) / (hi - lo), 0.0, 1.0)
        g = f / factor * ramp + f * (1 - ramp)
        a = float(np.float32(s.get("attn_factor", 0)))
        attn = a if a > 0 else 0.1 * np.log(factor) + 1.0
    ang = np.arange(max_pos, dtype=np.float64)[:, None] * g[None, :]
    tab = np.zeros((max_pos, hs // 2, 2))
    tab[:, :, 0] = 1.0
    tab[:, :rot // 2, 0], tab[:, :rot // 2, 1] = np.cos(ang) * attn, np.sin(ang) * attn
    return tab, attn, (lo, hi) if s["kind"] == "yarn" else None


GPT_OSS = dict(kind="yarn", factor=32.0, original_max_pos=4096, beta_fast=32.0, beta_slow=1.0, truncate=0)
ROPE_CONFIGS = [
    ("gpt-oss", 2048, 64, 64, 150000.0, GPT_OSS),
    ("gpt-oss-truncate", 2048, 64, 64, 150000.0, dict(GPT_OSS, truncate=1)),
    ("gpt-oss-defaults", 512, 64, 64, 150000.0, dict(kind="yarn", factor=32.0, original_max_pos=4096)),
    ("yarn-attn-factor", 512, 64, 64, 150000.0, dict(GPT_OSS, attn_factor=1.25)),
    ("llama-3.1", 2048, 128, 128, 500000.0, dict(kind="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_pos=8192)),
    ("linear-4", 1024, 128, 128, 10000.0, dict(kind="linear", factor=4.0)),
    ("partial-rotary", 512, 128, 64, 10000.0, dict(kind="yarn", factor=8.0, original_max_pos=2048)),
    # beta_fast = beta_slow: lo = hi = c(8) = 15.3, hi += 0.001 -- the ramp is a step between pairs 15 and 16
    ("lo-equals-hi", 512, 64, 64, 10000.0, dict(kind="yarn", factor=4.0, original_max_pos=4096, beta_fast=8.0, beta_slow=8.0)),
]


@pytest.mark.parametrize("name,max_pos,hs,rot,base,scaling", ROPE_CONFIGS, ids=[r[0] for r in ROPE_CONFIGS])
def test_rope_table_follows_the_formulas(llmie, name, max_pos, hs, rot, base, scaling):
    got = llmie.rope_table(max_pos, hs, rot, base, scaling)
    exp, attn, lohi = rope_restatement(max_pos, hs, rot, base, scaling)
    assert got.shape == (max_pos, hs // 2, 2) and got.dtype == np.float32
    # one fp32 rounding of a value no larger than the attention factor, plus a last-bit libm difference before the rounding
    err = np.abs(got.astype(np.float64) - exp).max()
    assert err <= 2.0 ** -23 * attn, (name, err)
    assert np.array_equal(got[:, rot // 2:, 0], np.ones((max_pos, (hs - rot) // 2), np.float32)) and not got[:, rot // 2:, 1].any()
    plain = llmie.rope_table(max_pos, hs, rot, base)
    assert np.abs(got[:64].astype(np.float64) - plain[:64]).max() > 1e-2, name + ": the scaling shows nowhere below position 64"
    if name == "lo-equals-hi":
        assert 15 < lohi[0] < 16 and lohi[1] == lohi[0] + 0.001
    if name == "gpt-oss":
        assert abs(attn - (0.1 * np.log(32.0) + 1.0)) < 1e-12 and 0 < lohi[0] < lohi[1] < 63


NONE_SHAPES = ((300, 128, 128, 10000.0), (160, 64, 32, 10000.0), (64, 64, 64, 150000.0), (40, 4, 4, 10000.0))


def test_rope_table_without_scaling_is_the_engines_formula(llmie):
    """kind NONE / no struct: the engine's create-time formula -- cosf / sinf of pos / powf(base, 2j / rot) -- bit for bit (evaluated
    here with the C library's own float functions, which is what llmie_decoder_create has always called)"""
    libm = C.CDLL(ctypes.util.find_library("m"))
    for fn, n in (("powf", 2), ("cosf", 1), ("sinf", 1)):
        getattr(libm, fn).restype, getattr(libm, fn).argtypes = C.c_float, [C.c_float] * n
    for max_pos, hs, rot, base in NONE_SHAPES:
        got = llmie.rope_table(max_pos, hs, rot, base)
        assert np.array_equal(got, llmie.rope_table(max_pos, hs, rot, base, dict(kind="none", factor=7.0)))
        exp = np.zeros_like(got)
        exp[:, :, 0] = 1.0
        for pos in range(max_pos):
            for j in range(rot // 2):
                ang = np.float32(pos) / np.float32(libm.powf(base, np.float32(2 * j) / np.float32(rot)))
                exp[pos, j] = libm.cosf(ang), libm.sinf(ang)
        assert np.array_equal(got, exp), (max_pos, hs, rot, base)


def _attn_cases_rope_tables_scalar():
    """attn_cases.rope_table at NONE_SHAPES, evaluated by a child interpreter whose numpy has its CPU-dispatched SIMD kernels switched
    off (NPY_DISABLE_CPU_FEATURES = every dispatched feature this CPU has), so that its float32 power / cos / sin are the C library's"""
    try:
        from numpy._core._multiarray_umath import __cpu_dispatch__, __cpu_features__
    except ImportError:
        from numpy.core._multiarray_umath import __cpu_dispatch__, __cpu_features__
    env = dict(os.environ)
    off = [f for f in __cpu_dispatch__ if __cpu_features__.get(f)]
    if off:
        env["NPY_DISABLE_CPU_FEATURES"] = " ".join(off)
    code = ("import sys; sys.path.insert(0, %r); import attn_cases as ac\n"
            "for a in %r: sys.stdout.buffer.write(ac.rope_table(*a).tobytes())" % (os.path.dirname(os.path.abspath(__file__)), NONE_SHAPES))
    raw = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, check=True).stdout
    out, at = [], 0
    for max_pos, hs, rot, base in NONE_SHAPES:
        n = max_pos * (hs // 2) * 2
        out.append(np.frombuffer(raw, np.float32, n, at * 4).reshape(max_pos, hs // 2, 2))
        at += n
    assert at * 4 == len(raw)
    return out


def test_rope_table_without_scaling_is_attn_cases_rope_table(llmie):
    """Kind NONE equals attn_cases.rope_table bit for bit -- with numpy's float32 power / cos / sin being the C library's, which is
    what the engine's create-time formula calls.  Where numpy dispatches those three to its own SIMD kernels (AVX2 / AVX-512 builds) its
    results differ from the C library's in the last bit, and the table with them: measured in one process on the build machine
    (elements that differ / all, largest difference) (300, 128, 128, 1e4) 7692 / 38400, 1.5e-5; (160, 64, 32, 1e4) 618 / 10240, 2.4e-7;
    (64, 64, 64, 1.5e5) 638 / 4096, 1.9e-6; (40, 4, 4, 1e4) 13 / 160, 6.0e-8 -- a last-bit difference in the divisor, multiplied by the
    position; with the SIMD kernels off, 0 everywhere.  So the reference is evaluated in a child interpreter with them off (the same
    function, the same shapes, no tolerance); what this process's numpy gives is printed beside it."""
    for (max_pos, hs, rot, base), exp in zip(NONE_SHAPES, _attn_cases_rope_tables_scalar()):
        got, here = llmie.rope_table(max_pos, hs, rot, base), ac.rope_table(max_pos, hs, rot, base)
        print("%s: against this process's numpy %d of %d elements differ, largest difference %.3g" % (
            (max_pos, hs, rot, base), (got != here).sum(), got.size, np.abs(got.astype(np.float64) - here).max()))
        assert np.array_equal(got, exp), ((max_pos, hs, rot, base), int((got != exp).sum()))


def test_rope_table_refusals(llmie):
    ok = dict(kind="yarn", factor=32.0, original_max_pos=4096)
    bad = [
        (64, 64, 64, dict(ok, factor=0.5), "factor"),
        (64, 64, 64, dict(kind="linear", factor=0.99), "factor"),
        (64, 64, 64, dict(kind="linear", factor=float("nan")), "factor"),
        (64, 64, 64, dict(ok, original_max_pos=0), "original_max_pos"),
        (64, 64, 64, dict(kind="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_pos=-1), "original_max_pos"),
        (64, 64, 64, dict(kind="llama3", factor=8.0, low_freq_factor=4.0, high_freq_factor=4.0, original_max_pos=8192), "low_freq_factor"),
        (64, 64, 64, dict(kind="llama3", factor=8.0, low_freq_factor=4.0, high_freq_factor=1.0, original_max_pos=8192), "low_freq_factor"),
        (64, 64, 63, ok, "rotary_dim"), (64, 64, 0, ok, "rotary_dim"), (64, 64, 66, ok, "rotary_dim"), (64, 64, -2, None, "rotary_dim"),
        (64, 64, 63, None, "rotary_dim"), (0, 64, 64, None, "shape"), (64, 64, 64, dict(ok, beta_fast=-1.0), "beta"),
        (64, 64, 64, dict(kind=9, factor=2.0), "kind"),
    ]
    for max_pos, hs, rot, s, word in bad:
        with pytest.raises(llmie.LlmieError, match=word):
            llmie.rope_table(max_pos, hs, rot, 10000.0, s)
    sc_ = llmie.rope_scaling(ok)
    assert llmie.lib().llmie_rope_table_fill(None, 64, 64, 64, 10000.0, C.addressof(sc_)) == -1
    llmie.rope_table(64, 64, 64, 10000.0, dict(kind="linear", factor=1.0))   # factor 1 is allowed
    with pytest.raises(llmie.LlmieError, match="unknown field"):
        llmie.rope_scaling(dict(kind="yarn", factr=2.0))


# ------------------------------------------------------------------------------------------------ plans and host-side refusals
def test_decode_plan_texts_with_and_without_the_bit(llmie):
    forms = ("rope", "ragged", "step_dev")
    for kw in (dict(window=0), dict(window=100, sinks=4)):
        for e4m3, hs, nh, kvh in ((False, 128, 8, 1), (False, 64, 2, 2), (True, 128, 8, 2), (True, 64, 4, 4)):
            base, st0 = llmie.decoder_mha_window_plan(llmie.F16, 3, nh, kvh, hs, 4096, kw["window"], kw.get("sinks", 0), kv_e4m3=e4m3, forms=forms)
            same, st1 = llmie.decoder_mha_sink_plan(llmie.F16, 3, nh, kvh, hs, 4096, kv_e4m3=e4m3, forms=forms, **kw)
            sink, st2 = llmie.decoder_mha_sink_plan(llmie.F16, 3, nh, kvh, hs, 4096, kv_e4m3=e4m3, forms=forms + ("head_sink",), **kw)
            assert st0 == st1 == st2 == 0 and base is not None and same == base and sink == base + " head_sink", (base, same, sink)
            # the older queries ignore the bit
            assert llmie.decoder_mha_window_plan(llmie.F16, 3, nh, kvh, hs, 4096, kw["window"], kw.get("sinks", 0), kv_e4m3=e4m3,
                                                 forms=forms + ("head_sink",))[0] == base
    assert llmie.decoder_mha_plan(llmie.F16, 3, 8, 2, 128, 4096, forms=forms + ("head_sink",)) == llmie.decoder_mha_plan(llmie.F16, 3, 8, 2, 128, 4096, forms=forms)
    # tickets, a host step of one chunk (the direct store)
    text, _ = llmie.decoder_mha_sink_plan(llmie.F16, 1, 8, 2, 128, 4096, step=100, forms=("rope", "tickets", "head_sink"))
    assert text.endswith("merge none head_sink"), text


def test_decode_plan_refuses_a_head_sink_without_a_kernel(llmie):
    forms = ("rope", "ragged", "step_dev", "head_sink")
    for dtype, e4m3, hs, nh, kvh, residues in ((llmie.F32, False, 128, 8, 2, None), (llmie.F16, False, 32, 8, 2, None), (llmie.F16, False, 256, 8, 2, None),
                                               (llmie.F16, False, 128, 16, 1, None), (llmie.F16, False, 128, 6, 2, None), (llmie.F16, True, 128, 8, 1, None),
                                               (llmie.F16, False, 128, 8, 2, {"qkv": 8}), (llmie.F16, False, 128, 8, 2, {"k": 2})):
        text, status = llmie.decoder_mha_sink_plan(dtype, 3, nh, kvh, hs, 4096, kv_e4m3=e4m3, forms=forms, residues=residues)
        assert text is None and status == -2, (dtype, e4m3, hs, nh, kvh, residues, text, status)
        if not e4m3:
            assert "head sink" in llmie.lib().llmie_last_error().decode()
            # ... and the same call without the bit is planned, where the geometry has any kernel
            if residues is None and nh % kvh == 0 and nh // kvh in (1, 2, 4, 8):
                assert llmie.decoder_mha_sink_plan(dtype, 3, nh, kvh, hs, 4096, forms=forms[:-1])[1] == 0


def test_decoder_mha_sink_host_refusals(llmie):
    """argument checks and planner refusals come before any device access: the pointers here are never followed"""
    p, ws = 1 << 20, 1 << 30
    f = llmie.lib().llmie_decoder_mha_sink

    def call(qkv=p, k=p, v=p, out=p, ctx=p, head_num=8, kvh=2, hs=128, window=0, sinks=0, sink=p, dtype=llmie.F16, e4m3=0, tickets=None):
        return f(qkv, None, k, v, out, 0, 3, head_num, kvh, hs, 4096, ctx, p, ws, p, hs, None, 0, 0, window, sinks, tickets, e4m3, 1.0, 1.0, sink, dtype, None)

    err = lambda: llmie.lib().llmie_last_error().decode()
    assert call(qkv=None) == -1 and call(ctx=None) == -1 and call(out=None) == -1
    assert call(window=-1) == -1 and "negative" in err()
    assert call(sinks=-1) == -1
    assert call(sink=p + 2) == -1 and "aligned" in err()
    assert call(head_num=7) == -1
    assert call(dtype=llmie.F32) == -2 and "head sink" in err()
    assert call(hs=32) == -2 and "head sink" in err()
    assert call(hs=256) == -2
    assert call(head_num=32, kvh=2) == -2          # ratio 16
    assert call(qkv=p + 8) == -2 and "head sink" in err()    # the generic kernel's operands
    assert call(e4m3=1, head_num=16, kvh=2) == -2   # e4m3 cache: ratio 8
    assert call(e4m3=1, tickets=p) == -2            # e4m3 cache: separate merge only


def test_engine_plans_under_the_head_sink_bit(llmie):
    cfg = dict(head_num=8, kv_head_num=2, head_size=128, inter_size=512, num_layers=2, vocab_size=100, max_seq_len=1024, max_batch=4,
               rotary_dim=128, rotary_base=10000.0, rms_eps=1e-5, dtype=llmie.F16, wfmt=llmie.W_F16, int4_group=128)
    for prefill, rows in ((False, 1), (False, 4), (True, 300)):
        assert llmie.decoder_plan_name(cfg, prefill, rows, call_flags=llmie.PLAN_HEAD_SINK) == llmie.decoder_plan_name(cfg, prefill, rows) is not None
    base, st = llmie.decoder_prefill_layer_plan(cfg, 300, 2, 200)
    sink, st1 = llmie.decoder_prefill_layer_plan(cfg, 300, 2, 200, call_flags=llmie.PLAN_HEAD_SINK)
    both, st2 = llmie.decoder_prefill_layer_plan(cfg, 300, 2, 200, call_flags=llmie.PLAN_HEAD_SINK | llmie.PLAN_WINDOW)
    assert st == st1 == st2 == 0 and sink == base + " attn_head_sink=1" and both == base + " attn_window=1 attn_head_sink=1", (base, sink, both)
    for bad in (dict(cfg, head_size=32, rotary_dim=32), dict(cfg, dtype=llmie.F32, wfmt=llmie.W_F32), dict(cfg, head_num=32)):
        assert llmie.decoder_plan_name(bad, False, 1, call_flags=llmie.PLAN_HEAD_SINK) is None
        assert "head sinks need" in llmie.lib().llmie_last_error().decode()
        assert llmie.decoder_plan_name(bad, False, 1) is not None
    text, status = llmie.decoder_prefill_layer_plan(dict(cfg, head_num=32), 300, 2, 200, call_flags=llmie.PLAN_HEAD_SINK)
    assert text is None and status == -2
