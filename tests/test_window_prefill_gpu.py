"""The flash prefill kernel under a sliding window with sink tokens (csrc/prefill.hip: the windowed instantiations of
prefill_flash_kernel), through Decoder.set_window + Decoder.prefill / prefill_paged on the one-layer engine of
tests/test_prefill_attn_gpu.py (QKV weight columns ARE the tokens' rows, o = identity, gate_up = 0: hidden_out - hidden_in is the
attention output).

Cases and the float64 restatement of the masked softmax come from tests/window_attn_cases.py: owners inside the mask of their query
row, dominating rows planted just outside it (in front of the window, behind the sinks, in the future).  One ragged batch of lengths
{1, 63, 64, 65, 130, 300} over histories {0, 37, 128, 200}; W in {1, 5, 17, 64, 65, 200, >= every context} x S in {0, 4, 70}; native
and e4m3 cache; two larger batches reach the 4-wave x 2-row-tile and the 8-wave form.  Held to the bound of
tests/prefill_attn_cases.py.  Exact conditions: no NaN / Inf anywhere (windows below a tile make a query row meet walked tiles in which
it sees no key); a window over every context gives the bits of the unwindowed pass; history rows that no query sees overwritten with
NaN change no bit; paged, the table entries of pages made only of such rows pointed at a poison page of NaNs change no bit.
"""
import numpy as np
import pytest
import torch

import prefill_attn_cases as pc
import window_attn_cases as wc
from test_prefill_attn_gpu import _dev, _engine, _pool

pytestmark = pytest.mark.gpu
DEV, F16 = "cuda", torch.float16


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _split(out, x, c):
    attn = (out.double() - x.double()).cpu().numpy()
    return [attn[c.cum[s]:c.cum[s + 1]] for s in range(c.bs)]


def _run_case(llmie, c, full_bits=False):
    dec = _engine(llmie, c)
    i32 = lambda v: torch.tensor(np.asarray(v), dtype=torch.int32, device=DEV)
    lens, hist = i32(c.lens), i32(c.hist)
    x = torch.zeros((c.T, c.H), dtype=F16, device=DEV)
    x[torch.arange(c.T), torch.arange(c.T)] = pc.X_ONE_HOT
    k0, v0 = _dev(c.k0), _dev(c.v0)
    form = "W=%d S=%d kv=%s" % (c.W, c.S, c.kv)
    nan = wc.NAN_CODE if c.scales else float("nan")

    def dense(kin, vin):
        kd, vd, out = kin.clone(), vin.clone(), torch.full_like(x, 9.0)
        dec.prefill(x, out, kd, vd, lens, hist, c.max_q_len)
        return out, kd, vd

    try:
        dec.set_window([c.W], c.S)
        out, kd, vd = dense(k0, v0)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all()), form + ": NaN / Inf in the output"
        r = [pc.check_case(_split(out, x, c), c, "dense " + form)]
        # history rows no query sees -> NaN: same bits, same appended rows
        dead = _dev(wc.prefill_dead_rows(c)).bool()
        kn, vn = k0.clone(), v0.clone()
        kn[0].permute(0, 2, 1, 3)[dead] = nan
        vn[0].permute(0, 2, 1, 3)[dead] = nan
        out_n, kdn, vdn = dense(kn, vn)
        assert torch.equal(out_n, out), form + ": a dead history row was read"
        # paged behind a shuffled table; then with the entries of wholly dead pages pointed at a poison page
        rng = np.random.default_rng(5)
        mp = c.max_seq // 128
        num_pages = c.bs * mp + 2
        perm = i32(rng.permutation(num_pages - 1)[:c.bs * mp].reshape(c.bs, mp))
        shape = (1, num_pages, c.kvh, 128, pc.HS)
        fill = lambda: torch.randint(0, 0x58, shape, device=DEV, dtype=torch.uint8) if c.scales else (torch.randn(shape, device=DEV) * 0.5).to(F16)
        fk, fv = fill(), fill()
        fk[:, num_pages - 1], fv[:, num_pages - 1] = nan, nan
        outs = []
        for table in (perm, None):
            if table is None:
                table = perm.clone()
                table[_dev(wc.prefill_dead_rows(c).reshape(c.bs, mp, 128).all(axis=2)).bool()] = num_pages - 1
            kp, vp, out_p = _pool(k0, perm, fk), _pool(v0, perm, fv), torch.full_like(x, 9.0)
            dec.prefill_paged(x, out_p, kp, vp, table, lens, hist, c.max_q_len)
            outs.append((out_p, kp, vp))
        r.append(pc.check_case(_split(outs[0][0], x, c), c, "paged " + form))
        assert torch.equal(outs[1][0], outs[0][0]), form + ": the table entry of a dead page was followed"
        assert _same(outs[1][1], outs[0][1]) and _same(outs[1][2], outs[0][2])
        assert _same(outs[0][1], _pool(kd, perm, fk)) and _same(outs[0][2], _pool(vd, perm, fv)), form + ": paged and dense appended differently"
    finally:
        dec.set_window(None)
    # the appended rows are those of the unwindowed pass
    out_f, kf, vf = dense(k0, v0)
    torch.cuda.synchronize()
    assert torch.equal(kf, kd) and torch.equal(vf, vd), form + ": the windowed pass appended other rows than the unwindowed one"
    if full_bits:
        assert torch.equal(out_f, out), form + ": a window over every context is not the unwindowed pass"
    return max(r)


@pytest.mark.parametrize("kv", ["f16", "np2"])
@pytest.mark.parametrize("W", wc.PREFILL_WINDOWS)
def test_window_prefill(llmie, kv, W):
    worst = 0.0
    for S in wc.PREFILL_SINKS:
        c = wc.make_prefill_case("window-%s-W%d-S%d" % (kv, W, S), 8, 2, wc.PREFILL_LENS, wc.PREFILL_HIST, kv, "q64w4t1", W, S)
        worst = max(worst, _run_case(llmie, c, full_bits=W >= max(c.ctx)))
    print("kv=%s W=%d: largest error / bound %.3f" % (kv, W, worst))


@pytest.mark.parametrize("kv", ["f16", "pow2"])
@pytest.mark.parametrize("entry", wc.PREFILL_FORMS, ids=[e[0] for e in wc.PREFILL_FORMS])
def test_window_prefill_other_flash_forms(llmie, entry, kv):
    """the 4-wave x 2-row-tile and the 8-wave instantiation (the plan text names the form), a window below and one above a tile"""
    name, nh, kvh, lens, hist, form = entry
    for W, S in ((17, 4), (200, 70)):
        c = wc.make_prefill_case("window-%s-%s-W%d" % (name, kv, W), nh, kvh, lens, hist, kv, form, W, S)
        text, _ = llmie.decoder_prefill_layer_plan(c.config(llmie), c.T, c.bs, c.max_q_len, call_flags=2 | llmie.PLAN_WINDOW)
        assert text is not None and "attn=" + form in text.split(" ") and text.endswith(" attn_window=1"), text
        r = _run_case(llmie, c)
        print("%s kv=%s W=%d S=%d: error / bound %.3f" % (name, kv, W, S, r))
