"""The flash prefill kernel with a learned sink logit per query head (csrc/prefill.hip: the SINK instantiations of
prefill_flash_kernel), through Decoder.set_head_sinks + Decoder.prefill / prefill_paged on the one-layer engine of
tests/test_prefill_attn_gpu.py (QKV weight columns ARE the tokens' rows, o = identity, gate_up = 0: hidden_out - hidden_in is the
attention output), at head size 128.

Cases, sink classes and the float64 restatement come from tests/sink_attn_cases.py, which builds them on the windowed prefill cases:
one ragged batch of lengths {1, 63, 64, 65, 130, 300} over histories {0, 37, 128, 200}; full attention, W = 5 (below a tile: query
rows meet walked tiles in which they see nothing -- the output must be finite and match) and W = 100 with 4 sink tokens; native and
e4m3 cache; dense and paged; two larger batches reach the 4-wave x 2-row-tile and the 8-wave form (by plan text).  Held to the bound
of tests/prefill_attn_cases.py.  Exact: sinks that are all -inf, and set_head_sinks(None), give the bits of the pass without sinks;
the appended rows are those of that pass.
"""
import numpy as np
import pytest
import torch

import prefill_attn_cases as pc
import sink_attn_cases as sc
import window_attn_cases as wc
from test_prefill_attn_gpu import _dev, _engine, _pool
from test_window_prefill_gpu import _same, _split

pytestmark = pytest.mark.gpu
DEV, F16 = "cuda", torch.float16
WINDOWS = [(0, 0), (5, 0), (100, 4)]


def _run_case(llmie, c):
    dec = _engine(llmie, c)
    i32 = lambda v: torch.tensor(np.asarray(v), dtype=torch.int32, device=DEV)
    lens, hist = i32(c.lens), i32(c.hist)
    x = torch.zeros((c.T, c.H), dtype=F16, device=DEV)
    x[torch.arange(c.T), torch.arange(c.T)] = pc.X_ONE_HOT
    k0, v0 = _dev(c.k0), _dev(c.v0)
    form = "W=%d S=%d kv=%s" % (c.W, c.S, c.kv)
    sink = torch.from_numpy(c.sink).to(DEV).view(1, c.nh)

    def dense():
        kd, vd, out = k0.clone(), v0.clone(), torch.full_like(x, 9.0)
        dec.prefill(x, out, kd, vd, lens, hist, c.max_q_len)
        return out, kd, vd

    try:
        dec.set_window([c.W] if c.W > 0 else None, c.S)
        plain, kp0, vp0 = dense()   # no head sinks yet
        dec.set_head_sinks(sink)
        out, kd, vd = dense()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all()), form + ": NaN / Inf in the output"
        assert torch.equal(kd, kp0) and torch.equal(vd, vp0), form + ": the pass with sinks appended other rows"
        r = [pc.check_case(_split(out, x, c), c, "dense " + form)]
        # paged behind a shuffled table
        rng = np.random.default_rng(5)
        mp = c.max_seq // 128
        num_pages = c.bs * mp + 1
        perm = i32(rng.permutation(num_pages)[:c.bs * mp].reshape(c.bs, mp))
        shape = (1, num_pages, c.kvh, 128, pc.HS)
        fill = lambda: torch.randint(0, 0x58, shape, device=DEV, dtype=torch.uint8) if c.scales else (torch.randn(shape, device=DEV) * 0.5).to(F16)
        fk, fv = fill(), fill()
        kp, vp, out_p = _pool(k0, perm, fk), _pool(v0, perm, fv), torch.full_like(x, 9.0)
        dec.prefill_paged(x, out_p, kp, vp, perm, lens, hist, c.max_q_len)
        r.append(pc.check_case(_split(out_p, x, c), c, "paged " + form))
        assert _same(kp, _pool(kd, perm, fk)) and _same(vp, _pool(vd, perm, fv)), form + ": paged and dense appended differently"
        # all -inf, and no sinks again: the bits of the pass without
        dec.set_head_sinks(torch.full_like(sink, float("-inf")))
        assert torch.equal(dense()[0], plain), form + ": sinks of -inf are not the pass without sinks"
        dec.set_head_sinks(None)
        assert torch.equal(dense()[0], plain), form + ": set_head_sinks(None) did not restore the pass"
        # (and the sinks mattered: the pass without them misses this case's reference by far)
        with pytest.raises(AssertionError):
            pc.check_case(_split(plain, x, c), c, "no sinks " + form)
    finally:
        dec.set_head_sinks(None)
        dec.set_window(None)
    torch.cuda.synchronize()
    return max(r)


@pytest.mark.parametrize("kv", ["f16", "np2"])
@pytest.mark.parametrize("W,S", WINDOWS)
def test_sink_prefill(llmie, kv, W, S):
    c = sc.make_prefill_case("sink-%s-W%d-S%d" % (kv, W, S), 8, 2, wc.PREFILL_LENS, wc.PREFILL_HIST, kv, "q64w4t1", W, S, shift=W % 3)
    text, _ = llmie.decoder_prefill_layer_plan(c.config(llmie), c.T, c.bs, c.max_q_len, call_flags=2 | llmie.PLAN_HEAD_SINK)
    assert text is not None and "attn=q64w4t1" in text.split(" ") and text.endswith(" attn_head_sink=1"), text
    print("kv=%s W=%d S=%d: largest error / bound %.3f" % (kv, W, S, _run_case(llmie, c)))


@pytest.mark.parametrize("kv", ["f16", "pow2"])
@pytest.mark.parametrize("entry", wc.PREFILL_FORMS, ids=[e[0] for e in wc.PREFILL_FORMS])
def test_sink_prefill_other_flash_forms(llmie, entry, kv):
    """the 4-wave x 2-row-tile and the 8-wave instantiation (the plan text names the form), without a window and with W = 100, S = 4"""
    name, nh, kvh, lens, hist, form = entry
    for W, S in ((0, 0), (100, 4)):
        c = sc.make_prefill_case("sink-%s-%s-W%d" % (name, kv, W), nh, kvh, lens, hist, kv, form, W, S, shift=1)
        flags = 2 | llmie.PLAN_HEAD_SINK | (llmie.PLAN_WINDOW if W else 0)
        text, _ = llmie.decoder_prefill_layer_plan(c.config(llmie), c.T, c.bs, c.max_q_len, call_flags=flags)
        assert text is not None and "attn=" + form in text.split(" ") and text.endswith(" attn_head_sink=1"), text
        print("%s kv=%s W=%d S=%d: error / bound %.3f" % (name, kv, W, S, _run_case(llmie, c)))
