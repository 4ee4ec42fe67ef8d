"""Sliding-window attention on an engine (llmie_decoder_set_window) and the page ring (llmie_kv_window_advance) under a captured
decode loop.

A 2-layer fp16 engine with layer_window = [W, 0] (one local, one global layer) and one with [W, W] runs a prefill and then three
decode steps -- batch 1 (the fused GEMV sequence), a batch in the packed range, the paged-ragged entry, and an engine with an e4m3
cache -- and is held to the window-aware float64 layer restatement of tests/window_attn_cases.py at model_param_cases.bounds().
The full-attention restatement of the same inputs misses the same bounds by far (asserted), so a layer that silently attended to
everything would fail.  With an e4m3 cache the restatement attends to the new rows as the device stored them (checked against its own
rounding to within one e4m3 step): the device's fp16 k / v values differ from float64 ones in the last bit, and a value next to an
e4m3 rounding boundary then lands a whole step away.  set_window(None) restores the bits of
an engine that never had a window.

The ring: W = 200, S = 4, 200 decode steps captured once and replayed, the pool holding exactly the pages the formula gives and
kv_window_advance running in the loop, must give bit for bit the hidden rows of the same loop over a fully mapped table with status
0 throughout; with one page less the helper must say 1 at the first step that needs the missing page and not before (that loop runs
the helper alone: a forward through an unmapped page must not be launched).
"""
import numpy as np
import pytest
import torch

import model_param_cases as mpc
import window_attn_cases as wc
from conftest import systematic_error

pytestmark = pytest.mark.gpu
DEV, F16 = "cuda", torch.float16
NH, KVH, HS, INTER, MAX_SEQ = 8, 2, 128, 512, 1024
H = NH * HS
W, S = 37, 4


def _cfg(llmie, max_batch, e4m3=False):
    cfg = dict(head_num=NH, kv_head_num=KVH, head_size=HS, inter_size=INTER, num_layers=2, vocab_size=100, max_seq_len=MAX_SEQ,
               max_batch=max_batch, rotary_dim=HS, rotary_base=10000.0, rms_eps=1e-5, dtype=llmie.F16, wfmt=llmie.W_F16, int4_group=128)
    if e4m3:
        cfg.update(kv_fmt=llmie.KV_FP8, k_scale=mpc.KS, v_scale=mpc.VS)
    return cfg


def _model(seed):
    rng = np.random.default_rng(seed)
    return rng, mpc.draw_layers(rng, NH, KVH, HS, INTER, 2)


def _check(got, exp, full, bounds, what):
    """element-wise and systematic bounds against the windowed restatement; the full-attention one must miss them (else the case
    could not tell a layer that ignored its window)"""
    rtol, atol = bounds["elem"]
    got = got.double().cpu().numpy()
    err = np.abs(got - exp)
    assert (err <= atol + rtol * np.abs(exp)).all(), "%s: worst error / bound %.3g" % (what, (err / (atol + rtol * np.abs(exp))).max())
    fro, proj = systematic_error(got, exp)
    assert fro <= bounds["fro"] and proj <= bounds["proj"], (what, fro, proj)
    if full is not None:
        assert systematic_error(full, exp)[0] > 10 * bounds["fro"], what + ": the window does not matter to this case"
    return fro


@pytest.mark.parametrize("windows", [[W, 0], [W, W]], ids=["local_global", "local_local"])
@pytest.mark.parametrize("kind", ["batch1", "packed", "paged_ragged", "e4m3"])
def test_windowed_engine_prefill_then_decode(llmie, kind, windows):
    lens = {"batch1": [150], "packed": [60] * 12, "paged_ragged": [150, 70, 129], "e4m3": [150, 70]}[kind]
    bs, e4m3 = len(lens), kind == "e4m3"
    rng, layers = _model(3)
    eng, ref_layers = mpc.engine_layers(llmie, layers, "f16")
    cfg = _cfg(llmie, bs, e4m3)
    dec = llmie.Decoder(cfg, eng)
    bounds = mpc.bounds("f16", "paged_e4m3" if e4m3 else "dense")
    ks, vs = (cfg["k_scale"], cfg["v_scale"]) if e4m3 else (1.0, 1.0)
    store = (lambda rows, which: mpc.e4m3_cache_rounding(rows, (ks, vs)[which])) if e4m3 else (lambda rows, which: mpc.h16(rows))
    shape = (2, bs, KVH, MAX_SEQ, HS)
    kc_ref, vc_ref = np.zeros(shape), np.zeros(shape)
    kc_full, vc_full = np.zeros(shape), np.zeros(shape)
    T = sum(lens)
    x = mpc.h16(rng.standard_normal((T, H)).astype(np.float32))
    xd = torch.from_numpy(x).to(DEV).to(F16)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    paged = kind == "paged_ragged"
    mp = MAX_SEQ // 128
    table = i32(np.random.default_rng(5).permutation(bs * mp + 2)[:bs * mp].reshape(bs, mp)) if paged else None
    cshape = (2, bs * mp + 2, KVH, 128, HS) if paged else shape
    new_cache = lambda: torch.zeros(cshape, dtype=torch.uint8 if e4m3 else F16, device=DEV)

    def prefill(kd, vd):
        out = torch.full_like(xd, 9.0)
        if paged:
            dec.prefill_paged(xd, out, kd, vd, table, i32(lens), i32([0] * bs), max(lens))
        else:
            dec.prefill(xd, out, kd, vd, i32(lens), i32([0] * bs), max(lens))
        return out

    try:
        plain = prefill(new_cache(), new_cache())   # before any window
        dec.set_window(windows, S)
        kd, vd = new_cache(), new_cache()
        out = prefill(kd, vd)
        torch.cuda.synchronize()
        dev = lambda: (mpc.TAB[kd.cpu().numpy()] * np.float32(ks), mpc.TAB[vd.cpu().numpy()] * np.float32(vs)) if e4m3 else None
        exp = wc.window_layer_restatement(cfg, ref_layers, x, kc_ref, vc_ref, lens, [0] * bs, windows, S, store, dev())
        full = wc.window_layer_restatement(cfg, ref_layers, x, kc_full, vc_full, lens, [0] * bs, [0, 0], 0, store)
        _check(out, exp, full, bounds, "%s prefill %s" % (kind, windows))
        ctx = list(lens)
        for step in range(3):
            xs = mpc.h16(rng.standard_normal((bs, H)).astype(np.float32))
            xsd, od = torch.from_numpy(xs).to(DEV).to(F16), torch.full((bs, H), 9.0, dtype=F16, device=DEV)
            new_ctx = [c + 1 for c in ctx]
            if kind in ("batch1", "packed"):
                dec.forward(xsd, od, kd, vd, new_ctx[0])
            elif paged:
                dec.forward_paged_ragged(xsd, od, kd, vd, table, i32(new_ctx))
            else:
                dec.forward_ragged(xsd, od, kd, vd, i32(new_ctx))
            torch.cuda.synchronize()
            exp = wc.window_layer_restatement(cfg, ref_layers, xs, kc_ref, vc_ref, [1] * bs, ctx, windows, S, store, dev())
            full = wc.window_layer_restatement(cfg, ref_layers, xs, kc_full, vc_full, [1] * bs, ctx, [0, 0], 0, store)
            _check(od, exp, full, bounds, "%s decode step %d %s" % (kind, step, windows))
            ctx = new_ctx
        dec.set_window(None)
        again = prefill(new_cache(), new_cache())
        torch.cuda.synchronize()
        assert torch.equal(again, plain), "set_window(None) did not restore the unwindowed pass"
    finally:
        dec.close()


def test_set_window_refusals(llmie):
    rng, layers = _model(3)
    eng, _ = mpc.engine_layers(llmie, layers, "f16")
    dec = llmie.Decoder(_cfg(llmie, 2), eng)
    try:
        for windows, sinks, word in (([-1, 0], 0, "negative"), ([5, 5], -1, "negative"), ([0, 0], 4, "without a window")):
            with pytest.raises(llmie.LlmieError, match=word):
                dec.set_window(windows, sinks)
        with pytest.raises(llmie.LlmieError, match="without a window"):
            llmie._check(llmie.lib().llmie_decoder_set_window(dec.handle, None, 3), "decoder_set_window")
        dec.set_window([0, 0], 0)   # no window anywhere: accepted, nothing set
        dec.set_window(7)
        dec.set_window(None)
    finally:
        dec.close()
    # an engine whose decode attention has no windowed form: head size 32
    cfg = dict(head_num=8, kv_head_num=8, head_size=32, inter_size=512, num_layers=1, vocab_size=100, max_seq_len=256, max_batch=2,
               rotary_dim=32, rotary_base=10000.0, rms_eps=1e-5, dtype=llmie.F16, wfmt=llmie.W_F16, int4_group=128)
    e32, _ = mpc.engine_layers(llmie, mpc.draw_layers(rng, 8, 8, 32, 512, 1), "f16")
    dec = llmie.Decoder(cfg, e32)
    try:
        with pytest.raises(llmie.LlmieError, match="sliding window"):
            dec.set_window([16], 0)
    finally:
        dec.close()
    assert llmie.decoder_plan_name(cfg, False, 2, call_flags=llmie.PLAN_WINDOW) is None
    assert llmie.decoder_plan_name(_cfg(llmie, 2), False, 2, call_flags=llmie.PLAN_WINDOW) == llmie.decoder_plan_name(_cfg(llmie, 2), False, 2)


def test_page_ring_under_a_captured_decode_loop(llmie):
    RW, RS, STEPS, START, bs, mp = 200, 4, 200, 380, 2, 8
    pool = wc.ring_pages(RW, RS)
    assert pool == 4
    rng, layers = _model(4)
    eng, _ = mpc.engine_layers(llmie, layers, "f16")
    dec = llmie.Decoder(_cfg(llmie, bs), eng)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    xp = torch.from_numpy(mpc.h16(rng.standard_normal((bs * START, H)).astype(np.float32))).to(DEV).to(F16)
    xs = torch.from_numpy(mpc.h16(rng.standard_normal((STEPS, bs, H)).astype(np.float32))).to(DEV).to(F16)

    def run(table_rows, num_pages, ring):
        """prefill START tokens per sequence, then STEPS decode steps: one captured, all replayed"""
        table = i32(table_rows)
        kp = torch.zeros((2, num_pages, KVH, 128, HS), dtype=F16, device=DEV)
        vp = torch.zeros_like(kp)
        dec.prefill_paged(xp, torch.empty_like(xp), kp, vp, table, i32([START] * bs), i32([0] * bs), START)
        cached, ctx, idx = i32([START] * bs), i32([START + 1] * bs), torch.zeros(1, dtype=torch.int64, device=DEV)
        hid, out = torch.empty((bs, H), dtype=F16, device=DEV), torch.empty((bs, H), dtype=F16, device=DEV)
        rows = torch.zeros((STEPS, bs, H), dtype=F16, device=DEV)
        status, stats = torch.zeros(bs, dtype=torch.int32, device=DEV), torch.full((STEPS, bs), -1, dtype=torch.int32, device=DEV)

        def step():
            hid.copy_(xs.index_select(0, idx)[0])
            if ring:
                llmie.kv_window_advance(table, cached, RW, RS, status=status)
            dec.forward_paged_ragged(hid, out, kp, vp, table, ctx)
            rows.index_copy_(0, idx, out[None])
            stats.index_copy_(0, idx, status[None])
            cached.add_(1), ctx.add_(1), idx.add_(1)

        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        step()   # (eager once: step 0)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            step()   # captured: enqueues nothing
        for _ in range(STEPS - 1):
            graph.replay()
        torch.cuda.synchronize()
        return rows, stats, table.cpu().tolist()

    try:
        dec.set_window([RW, RW], RS)
        full_rows, _, _ = run([[b * mp + p for p in range(mp)] for b in range(bs)], bs * mp, ring=False)
        # the formula's pages: 0..2 hold the prompt, the fourth is the caller's spare, mapped where the next token goes
        ring_table = [[b * pool + p for p in range(pool)] + [-1] * (mp - pool) for b in range(bs)]
        ring_rows, stats, table = run(ring_table, bs * pool, ring=True)
        assert bool((stats == 0).all()), stats.cpu().tolist()
        assert torch.equal(ring_rows, full_rows), "the ring changed a hidden row"
        assert bool(torch.isfinite(ring_rows).all())
        for row in table:   # the sink page stayed, the ring moved on: page 1 went to index 4
            assert row[0] >= 0 and row[1] == -1 and row[4] >= 0 and sorted(x for x in row if x >= 0) == sorted(set(x for x in row if x >= 0))
        # one page short (no spare): the helper alone, same positions
        short = i32([[b * pool + p for p in range(pool - 1)] + [-1] * (mp - pool + 1) for b in range(bs)])
        before = short.clone()
        first_bad = None
        for step in range(8):
            st = llmie.kv_window_advance(short, i32([START + step] * bs), RW, RS).cpu().tolist()
            if st != [0] * bs:
                first_bad = (START + step, st)
                break
        assert first_bad == (384, [1] * bs), first_bad   # the first token of page 3
        assert torch.equal(short, before)
    finally:
        dec.set_window(None)
        dec.close()
