"""Decode attention with a learned sink logit per query head (llmie_decoder_mha_sink: the SINK instantiations of the split-KV kernel,
of its merge kernel and of the in-launch ticket merge) on the GPU.

Cases, sink classes and the float64 reference come from tests/sink_attn_cases.py (tests/test_sink_cases_cpu.py checks them on the
CPU).  Ragged batches of 3 over 2 KV heads whose lengths are chosen FROM THE PLAN TEXT'S CHUNK so that the splits per sequence are 1
(the split kernel's direct store), 2, 16 and 17 (a second merge round); head sizes 128 / 64 at ratios 1 and 8 over the fp16 cache and
ratio 4 over the e4m3 cache; full attention, a window below a chunk with 4 sink tokens and a window spanning three chunks; every case
dense and paged, with the merge kernel and (native cache) with tickets, at attn_cases.BOUNDS["rope"] -- the sink only multiplies a
row by an fp32 factor in (0, 1], so it adds no error term of its own.

Exact conditions, bit for bit: head_sink = NULL is llmie_decoder_mha_window's call; so are sinks that are all -inf; tickets and the
separate merge agree; a row's bits do not depend on its batch slot; the caches after the call are the caches after the plain call.
A form without a kernel writes nothing.  One captured launch, replayed after the sink array was overwritten on the device, gives the
new reference.
"""
import re

import numpy as np
import pytest
import torch

import attn_cases as ac
import sink_attn_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUNDS = ac.BOUNDS["rope"][ac.F16]
CASES = sc.decode_cases()
FORMS = ("rope", "ragged", "step_dev", "head_sink")


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _plan_chunk(llmie, geo, batch=3, **kw):
    """tokens per workgroup and chunks per workgroup of the launch the entry plans, from its plan text"""
    _, hs, ratio, _, scales = geo
    text, status = llmie.decoder_mha_sink_plan(llmie.F16, batch, sc.KVH * ratio, sc.KVH, hs, 4096, kv_e4m3=scales is not None, forms=FORMS, **kw)
    assert status == 0 and text.endswith(" head_sink"), text
    m = re.search(r" cpw(\d+) chunk(\d+) ", text)
    return int(m.group(2)), int(m.group(1))


class _Inputs:
    def __init__(self, llmie, c):
        self.c, self.e4m3 = c, c.scales is not None
        self.qkv = _dev(c.qkv, torch.float16)
        self.kc, self.vc = (_dev(c.kq), _dev(c.vq)) if self.e4m3 else (_dev(c.kc, torch.float16), _dev(c.vc, torch.float16))
        self.bias = None if c.bias is None else _dev(c.bias, torch.float16)
        self.tab = _dev(c.tab)
        self.ctx = torch.tensor(c.steps, dtype=torch.int32, device=DEV)
        self.ws = torch.full((llmie.decoder_mha_workspace_bytes(c.bs, c.nh, c.hs, c.max_seq) // 4,), float("nan"), device=DEV)
        self.sink = _dev(c.sink)
        self.pages = c.max_seq // sc.KV_PAGE

    def out(self):
        return torch.full((self.c.bs, self.c.nh * self.c.hs), 9.0, dtype=torch.float16, device=DEV)

    def call(self, llmie, kc, vc, sink, table=None, tickets=None, qkv=None, ctx=None, out=None):
        c, out = self.c, self.out() if out is None else out
        llmie.decoder_mha_sink(self.qkv if qkv is None else qkv, self.bias, kc, vc, out, 0, c.nh, c.kvh, self.ctx if ctx is None else ctx, self.ws,
                               self.tab, c.rot, c.max_seq, sink, window=c.W, sinks=c.S, block_table=table, tickets=tickets, kv_scales=c.scales)
        return out

    def pool(self, dense, perm, filler):
        L, bs, kvh, max_seq, hs = dense.shape
        pages = dense.view(L, bs, kvh, self.pages, 128, hs).permute(0, 1, 3, 2, 4, 5).reshape(L, bs * self.pages, kvh, 128, hs)
        pool = filler.clone()
        pool[:, perm.flatten().long()] = pages
        return pool


def _finish_e4m3(c, kd, vd):
    """the reference attends to the appended rows as the device stored them (one e4m3 step of slack against the CPU's rounding)"""
    rows = {}
    for name, got, want, scale in (("K", kd, c.k_codes_new, c.scales[0]), ("V", vd, c.v_codes_new, c.scales[1])):
        rows[name] = np.stack([got[0, b, :, s - 1].cpu().numpy() for b, s in enumerate(c.steps)])
        a, e = ac.E4M3[rows[name]].astype(np.float64) * scale, ac.E4M3[want].astype(np.float64) * scale
        assert (np.abs(a - e) <= 0.126 * np.abs(e) + scale * 2.0 ** -9).all(), sc.describe(c, "e4m3 append " + name)
    sc.finish(c, rows["K"], rows["V"])


def _one_case(llmie, c, rng):
    x = _Inputs(llmie, c)
    tickets = lambda: None if x.e4m3 else torch.zeros(c.bs * c.kvh, dtype=torch.int32, device=DEV)
    # the plain call: llmie_decoder_mha_window on the same inputs
    k0, v0, out0 = x.kc.clone(), x.vc.clone(), x.out()
    llmie.decoder_mha_window(x.qkv, x.bias, k0, v0, out0, 0, c.nh, c.kvh, x.ctx, x.ws, x.tab, c.rot, c.max_seq, c.W, c.S, kv_scales=c.scales)
    # head_sink = NULL, and sinks that are all -inf: its bits, its caches
    for what, sink in (("NULL", None), ("all -inf", torch.full_like(x.sink, float("-inf")))):
        k1, v1 = x.kc.clone(), x.vc.clone()
        out1 = x.call(llmie, k1, v1, sink)
        assert torch.equal(out1, out0) and torch.equal(k1, k0) and torch.equal(v1, v0), sc.describe(c, "head_sink " + what) + ": not the plain call"
        if not x.e4m3:
            t = tickets()
            assert torch.equal(x.call(llmie, x.kc.clone(), x.vc.clone(), sink, tickets=t), out0), sc.describe(c, "tickets, head_sink " + what)
    # dense, merge kernel
    kd, vd = x.kc.clone(), x.vc.clone()
    out = x.call(llmie, kd, vd, x.sink)
    torch.cuda.synchronize()
    assert torch.equal(kd, k0) and torch.equal(vd, v0), sc.describe(c, "dense") + ": caches differ from the plain call's"
    if x.e4m3:
        _finish_e4m3(c, kd, vd)
    assert bool(torch.isfinite(out).all())
    rs = [sc.check(out.double().cpu().numpy(), c, "dense", BOUNDS)]
    # dense, in-launch merge: the bits of the merge kernel
    if not x.e4m3:
        t, kt, vt = tickets(), x.kc.clone(), x.vc.clone()
        out_t = x.call(llmie, kt, vt, x.sink, tickets=t)
        assert torch.equal(out_t, out), sc.describe(c, "dense, tickets") + ": not the bits of the separate merge"
        assert int(t.abs().sum()) == 0 and torch.equal(kt, k0) and torch.equal(vt, v0)
    # the rows in other batch slots: the same bits
    order = [2, 0, 1] if c.bs == 3 else list(rng.permutation(c.bs))
    idx = torch.tensor(order, device=DEV)
    out_r = x.call(llmie, x.kc[:, idx].contiguous(), x.vc[:, idx].contiguous(), x.sink, qkv=x.qkv[idx].contiguous(), ctx=x.ctx[idx].contiguous())
    assert torch.equal(out_r, out[idx]), sc.describe(c, "dense, batch order %s" % order) + ": a row's bits depend on its slot"
    # paged: the same rows behind a shuffled block table
    num_pages = c.bs * x.pages + 1
    perm = _dev(rng.permutation(num_pages)[:c.bs * x.pages].astype(np.int32).reshape(c.bs, x.pages))
    if x.e4m3:
        filler = torch.randint(0, 0x58, (1, num_pages, c.kvh, 128, c.hs), dtype=torch.uint8, device=DEV)
    else:
        filler = (torch.randn((1, num_pages, c.kvh, 128, c.hs), device=DEV) * 0.5).to(torch.float16)
    kp, vp = x.pool(x.kc, perm, filler), x.pool(x.vc, perm, filler)
    kp1, vp1 = kp.clone(), vp.clone()
    out_p = x.call(llmie, kp1, vp1, x.sink, table=perm)
    rs.append(sc.check(out_p.double().cpu().numpy(), c, "paged", BOUNDS))
    assert _same(kp1, x.pool(k0, perm, filler)) and _same(vp1, x.pool(v0, perm, filler)), sc.describe(c, "paged") + ": pools"
    if not x.e4m3:
        t = tickets()
        out_pt = x.call(llmie, kp.clone(), vp.clone(), x.sink, table=perm, tickets=t)
        assert torch.equal(out_pt, out_p) and int(t.abs().sum()) == 0, sc.describe(c, "paged, tickets")
    torch.cuda.synchronize()
    return max(rs)


@pytest.mark.parametrize("cid,geo,W,S", CASES, ids=[d[0] for d in CASES])
def test_sink_decode_attention(llmie, cid, geo, W, S):
    chunk, cpw = _plan_chunk(llmie, geo)
    assert cpw == 1 and chunk == ac.chunk_len(ac.F16, geo[1], e4m3=geo[4] is not None), (chunk, cpw)
    rng = np.random.default_rng(5)
    worst = 0.0
    for i, steps in enumerate(sc.step_sets(chunk)):
        worst = max(worst, _one_case(llmie, sc.build(geo, W, S, steps, chunk, sc.max_seq_of(chunk), shift=2 - i), rng))
    print("%s: largest error / bound %.3f" % (cid, worst))


def test_sink_decode_attention_two_chunks_per_workgroup(llmie):
    """e4m3 cache at batch 64: cpw = 2 (asserted from the plan text): the sink enters once per row there too"""
    geo = sc.CPW_GEOMETRY
    span, cpw = _plan_chunk(llmie, geo, batch=sc.CPW_BATCH)
    assert cpw == 2 and span == 512, (span, cpw)
    rng = np.random.default_rng(5)
    pool = [1, 255, 256, 257, 511, 512, 513, 700, 1024, 1025, 1500, 2 * span + 1, 4 * span, 4 * span + 37]
    steps = [pool[(5 * b) % len(pool)] for b in range(sc.CPW_BATCH)]
    for W, S in ((0, 0), (257, 4)):
        r = _one_case(llmie, sc.build(geo, W, S, steps, span, 5 * span, shift=2), rng)
        print("cpw2 W=%d S=%d: largest error / bound %.3f" % (W, S, r))


def test_a_replayed_launch_reads_the_sinks_of_the_replay(llmie):
    """one captured decode launch; the sink array is overwritten on the device between replays"""
    geo = sc.GEOMETRIES[1]   # fp16, head size 128, ratio 8
    chunk, _ = _plan_chunk(llmie, geo)
    c = sc.build(geo, 0, 0, sc.step_sets(chunk)[0], chunk, sc.max_seq_of(chunk), shift=2)
    x = _Inputs(llmie, c)
    kd, vd, out = x.kc.clone(), x.vc.clone(), x.out()
    x.call(llmie, kd, vd, x.sink, out=out)   # eager once
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(graph, stream=side):
        x.call(llmie, kd, vd, x.sink, out=out)
    for shift in (3, 0, 2):
        values, _ = sc.sink_values(c.nh, shift)
        x.sink.copy_(_dev(values))
        out.fill_(9.0)
        graph.replay()
        torch.cuda.synchronize()
        rtol, atol = BOUNDS
        exp = sc.attend(c, values)
        err = np.abs(out.double().cpu().numpy() - exp) / (atol + rtol * np.abs(exp))
        assert err.max() <= 1.0, "replay with shift %d: error / bound %.3g" % (shift, err.max())
        if shift != 2:   # (and the values of the capture would have missed it)
            assert sc.distance(c, exp, BOUNDS) >= 10.0


def test_sink_forms_without_a_kernel_write_nothing(llmie):
    """fp32 / head size 32 / unaligned qkv with a head sink: LLMIE_ERR_UNSUPPORTED, caches and output untouched"""
    for dtype, hs, skew in ((torch.float32, 128, 0), (torch.float16, 32, 0), (torch.float16, 128, 4)):
        bs, nh, kvh, max_seq = 2, 4, 2, 256
        qkv = torch.randn((bs * (nh + 2 * kvh) * hs + 8,), device=DEV).to(dtype)[skew:skew + bs * (nh + 2 * kvh) * hs].view(bs, nh + 2 * kvh, hs)
        kc = torch.randn((1, bs, kvh, max_seq, hs), device=DEV).to(dtype)
        vc, out = kc.clone(), torch.full((bs, nh * hs), 9.0, dtype=dtype, device=DEV)
        k0 = kc.clone()
        ws = torch.zeros(llmie.decoder_mha_workspace_bytes(bs, nh, hs, max_seq) // 4, device=DEV)
        ctx = torch.tensor([200, 7], dtype=torch.int32, device=DEV)
        tab = _dev(ac.rope_table(max_seq, hs, hs))
        sink = torch.zeros(nh, device=DEV)
        with pytest.raises(llmie.LlmieError, match=r"\(-2\).*head sink"):
            llmie.decoder_mha_sink(qkv, None, kc, vc, out, 0, nh, kvh, ctx, ws, tab, hs, max_seq, sink)
        torch.cuda.synchronize()
        assert torch.equal(kc, k0) and torch.equal(vc, k0) and bool((out == 9.0).all())
