"""Every refusal of the projection entries that ends in the host checks -- llmie_linear, llmie_linear_swiglu, llmie_linear_w8a16,
llmie_linear_w4a16, llmie_linear_mxfp4, llmie_linear_fp8, llmie_linear_fp8_swiglu, llmie_linear_packed, and llmie_linear_route for
the planner's refusals no compute entry reaches (a fused SwiGLU on quantised weights, the MXFP4 epilogue) -- by return code and by
the WHOLE llmie_last_error() text (no GPU).  Each call breaks one rule of its entry, a rule of the route planner behind it (a fused
SwiGLU without a form, slabs too small, the int4 split-K scale alignment, the MXFP4 and fp8 shape refusals, the workspace alignment
rules), or two rules at once, so that the recorded text also says which check comes first.  The texts in
golden/linear_refusals.json are what the library printed when they were recorded (`python tests/test_linear_refusals_cpu.py
--record`): a change to the host side of the projection family that rewords or reorders a refusal fails here.  Pointers are fake
and never dereferenced: every call ends in the checks, none reaches a launch."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "linear_refusals.json")
FAKE = 0x10000   # 256-byte aligned
BIG = 1 << 40
W_F16, W_INT8, W_INT4, W_FP8, W_F32, W_MXFP4 = 0, 1, 2, 3, 4, 5
F32, F16 = 0, 1

# entry -> (argument order, a call that passes every check)
ENTRIES = {
    "linear": ("x w y M K N trans_b bias residual dtype ws ws_bytes stream",
               dict(x=FAKE, w=FAKE, y=FAKE, M=16, K=4096, N=4096, trans_b=1, bias=None, residual=None, dtype=F16, ws=None, ws_bytes=0)),
    "linear_swiglu": ("x w y M K N dtype ws ws_bytes stream",
                      dict(x=FAKE, w=FAKE, y=FAKE, M=16, K=4096, N=8192, dtype=F16, ws=None, ws_bytes=0)),
    "linear_w8a16": ("x w scale y M K N bias residual ws ws_bytes stream",
                     dict(x=FAKE, w=FAKE, scale=FAKE, y=FAKE, M=16, K=4096, N=4096, bias=None, residual=None, ws=None, ws_bytes=0)),
    "linear_w4a16": ("x w scale y M K N group bias residual ws ws_bytes stream",
                     dict(x=FAKE, w=FAKE, scale=FAKE, y=FAKE, M=16, K=4096, N=4096, group=128, bias=None, residual=None, ws=None, ws_bytes=0)),
    "linear_mxfp4": ("x w scale y M K N bias residual ws ws_bytes stream",
                     dict(x=FAKE, w=FAKE, scale=FAKE, y=FAKE, M=16, K=4096, N=4096, bias=None, residual=None, ws=None, ws_bytes=0)),
    "linear_fp8": ("x w scale y M K N bias residual ws ws_bytes stream",
                   dict(x=FAKE, w=FAKE, scale=FAKE, y=FAKE, M=16, K=4096, N=4096, bias=None, residual=None, ws=FAKE, ws_bytes=BIG)),
    "linear_fp8_swiglu": ("x w scale y M K N ws ws_bytes stream",
                          dict(x=FAKE, w=FAKE, scale=FAKE, y=FAKE, M=4096, K=4096, N=22016, ws=FAKE, ws_bytes=BIG)),
    "linear_packed": ("fmt x w scale y M K N swiglu x32 residual gamma pre_bias eps ws ws_bytes stream",
                      dict(fmt=W_INT8, x=FAKE, w=FAKE, scale=FAKE, y=FAKE, M=16, K=4096, N=4096, swiglu=0, x32=0, residual=None, gamma=None,
                           pre_bias=None, eps=1e-5, ws=None, ws_bytes=0)),
    "linear_route": ("fmt x w scale y M K N swiglu group bias residual ws ws_bytes",
                     dict(fmt=W_INT8, x=FAKE, w=FAKE, scale=FAKE, y=FAKE, M=16, K=4096, N=4096, swiglu=0, group=0, bias=None, residual=None,
                          ws=None, ws_bytes=0)),
}
NULLS = [dict(x=None), dict(w=None), dict(y=None)]
SHAPE = [dict(M=0), dict(K=-1), dict(N=0)]
WS16 = [dict(ws=FAKE + 8, ws_bytes=BIG)]
SMALL_SLABS = dict(ws=FAKE, ws_bytes=1024)   # split-K shapes: a workspace is there, so the split-K route is planned, and too small
# one rule each, in the order the entry checks them; the planner's refusals behind the entry's own
RULES = {
    "linear": NULLS + SHAPE + WS16 + [dict(dtype=7), SMALL_SLABS, dict(SMALL_SLABS, M=100)],
    "linear_swiglu": NULLS + SHAPE + [dict(N=8191), dict(dtype=F32)] + WS16 + [dict(M=100, N=22016), dict(M=65, K=4100), SMALL_SLABS],
    "linear_w8a16": NULLS + [dict(scale=None)] + SHAPE + WS16 + [dict(M=100, K=1000, N=1000), dict(M=9, x=FAKE + 2), SMALL_SLABS,
                                                               dict(SMALL_SLABS, M=150)],
    "linear_w4a16": NULLS + [dict(scale=None)] + SHAPE + [dict(group=48), dict(group=0), dict(group=96)] + WS16 +
                    [dict(M=100, x=FAKE + 2), dict(scale=FAKE + 2, ws=FAKE, ws_bytes=BIG), SMALL_SLABS, dict(SMALL_SLABS, scale=FAKE + 2)],
    "linear_mxfp4": NULLS + [dict(scale=None)] + SHAPE + WS16 + [dict(K=1000), dict(x=FAKE + 2), dict(w=FAKE + 4), dict(M=300, K=4112)],
    "linear_fp8": NULLS + [dict(scale=None), dict(ws=None)] + SHAPE + [dict(ws_bytes=16), dict(K=1000), dict(K=256), dict(w=FAKE + 8),
                                                                     dict(ws=FAKE + 16), dict(M=100, K=4224), dict(M=16, K=1152)],
    "linear_fp8_swiglu": NULLS + [dict(scale=None), dict(ws=None)] + SHAPE + [dict(N=22015), dict(M=16), dict(K=4160), dict(w=FAKE + 8),
                                                                            dict(ws=FAKE + 16), dict(y=FAKE + 4), dict(ws_bytes=16)],
    "linear_packed": NULLS + SHAPE + [dict(swiglu=1, residual=FAKE), dict(fmt=W_F32), dict(fmt=W_MXFP4), dict(M=33), dict(x=FAKE + 2),
                                      dict(y=FAKE + 4), dict(scale=None), dict(gamma=FAKE, residual=FAKE), dict(K=4100), dict(x32=1, K=4112), dict(K=11008), dict(K=11008, ws=FAKE + 8, ws_bytes=BIG),
                                      dict(K=11008, ws=FAKE, ws_bytes=1024)],
    "linear_route": NULLS + [dict(scale=None)] + SHAPE + [dict(swiglu=1, N=4095), dict(swiglu=1, bias=FAKE),
                                                          dict(fmt=W_INT4, group=48)] + WS16 +
                    [dict(swiglu=1, M=100, N=8192), dict(fmt=W_MXFP4, swiglu=1), dict(fmt=W_MXFP4, K=1000), dict(fmt=W_MXFP4, swiglu=1, K=1000),
                     dict(fmt=W_F16, swiglu=1, M=100, N=22016), dict(fmt=W_INT4, group=128, scale=FAKE + 2, ws=FAKE, ws_bytes=BIG)],
}
# two rules at once beyond the neighbours in an entry's order
EXTRA = {
    "linear": [dict(x=None, dtype=7), dict(M=0, ws=FAKE + 8), dict(dtype=7, ws=FAKE, ws_bytes=1024)],
    "linear_fp8": [dict(K=1000, ws_bytes=16), dict(ws=None, M=0), dict(w=FAKE + 8, ws=FAKE + 16), dict(K=1000, ws=FAKE + 16)],
    "linear_fp8_swiglu": [dict(M=16, ws_bytes=16), dict(x=None, N=22015)],
    "linear_w4a16": [dict(group=48, M=0), dict(group=48, ws=FAKE + 8)],
    "linear_packed": [dict(fmt=W_F32, M=0), dict(fmt=W_F32, swiglu=1, residual=FAKE), dict(M=33, fmt=W_F32)],
    "linear_mxfp4": [dict(K=1000, ws=FAKE + 8), dict(K=1000, M=0)],
}


def _call(llmie, entry, kw):
    order, base = ENTRIES[entry]
    a = dict(base, stream=None)
    a.update(kw)
    r = getattr(llmie.lib(), "llmie_" + entry)(*[a[k] for k in order.split()])
    if entry == "linear_route":   # a query: the route's name, or NULL with the reason
        r = 0 if r is not None else None
    return [r, llmie.lib().llmie_last_error().decode()]


def _name(entry, kw):
    return entry + ":" + ",".join("%s=%s" % (k, kw[k]) for k in sorted(kw))


def cases():
    out = {}
    for entry, rules in RULES.items():
        calls = list(rules)
        for x, y in zip(rules, rules[1:]):   # neighbours in the order, where they do not set the same operand
            if not set(x) & set(y):
                calls.append(dict(x, **y))
        for kw in calls + EXTRA.get(entry, []):
            out[_name(entry, kw)] = (entry, kw)
    return out


CASES = cases()


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_recording_covers_the_cases(recorded):
    assert sorted(recorded) == sorted(CASES)
    assert len(CASES) > 150
    # every one is a refusal (none reached a launch), and all three codes occur
    assert {rc for rc, _ in recorded.values()} == {-1, -2, -4, None}
    texts = " | ".join(text for _, text in recorded.values())
    for words in ("fused SwiGLU epilogue without a split-K workspace", "slab workspace too small or misaligned", "linear(split-K int4): needs",
                  "linear_mxfp4: needs K % 32 == 0", "linear_mxfp4: plain epilogue", "linear_fp8: needs K % 256 == 0",
                  "linear_fp8: workspace too small", "linear_wq: fused SwiGLU needs", "linear_wq: unsupported shape",
                  "workspace must be 16-byte aligned", "linear(packed): unsupported shape"):
        assert words in texts, words


@pytest.mark.parametrize("entry", sorted(RULES))
def test_every_refusal_is_the_recorded_one(llmie, recorded, entry):
    for name, (e, kw) in CASES.items():
        if e == entry:
            assert _call(llmie, e, kw) == recorded[name], name


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_linear_refusals_cpu.py --record")
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from conftest import load_llmie
    mod = load_llmie()
    rec = {name: _call(mod, e, kw) for name, (e, kw) in sorted(CASES.items())}
    bad = [name for name, (rc, _) in rec.items() if rc not in (-1, -2, -4, None)]
    if bad:
        sys.exit("NOT recorded: these calls are no refusals of the host checks: %s" % bad)
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded %d refusals" % len(CASES))
