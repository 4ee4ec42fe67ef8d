"""Sliding-window decode attention (llmie_decoder_mha_window: the windowed instantiations of the split-KV kernel, its merge kernel
and the in-launch ticket merge) and the page ring (llmie_kv_window_advance) on the GPU.

Cases, planted rows, the rows planted just outside the mask and the float64 reference come from tests/window_attn_cases.py
(tests/test_window_cases_cpu.py checks them on the CPU).  max_seq_len 2048, a ragged batch of 3, 2 KV heads:

    activations / cache   head_size   tokens per chunk   128-token pages per chunk   head ratios
    fp16 / fp16           128 / 64    128 / 256          1 / 2                       1, 4
    fp16 / e4m3           128         256                2                           1, 4
    fp16 / e4m3           64          512                4                           2

Each (geometry, W) runs S in {0, 1, 4, chunk + 3} on three step sets (step - W on a chunk start, a chunk end, a page boundary, mid
chunk; step <= W; step = 1; the longest context) plus S touching and overlapping the window start; every case runs dense and
paged, with the merge kernel and (native cache) with tickets, at the project's bound for this entry (attn_cases.BOUNDS["rope"]).

Three conditions are exact, bit for bit, because they follow from what the kernel may read, not from arithmetic:
  (a) a window >= the context gives the output -- and the caches -- of the unwindowed call on the same inputs;
  (b) with every dead cache row (masked, or past the context) overwritten with NaN no output bit changes, and the output is finite;
  (c) paged, with the table entries of wholly dead pages pointed at a poison page of NaNs (a valid page: a test must not be able to
      fault the card), the output has the bits of the fully mapped call.
The appended row lands in the cache exactly as in the unwindowed call.
"""
import numpy as np
import pytest
import torch

import attn_cases as ac
import window_attn_cases as wc

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUNDS = ac.BOUNDS["rope"][ac.F16]
CASES = wc.decode_cases()
MAX_PAGES = wc.MAX_SEQ // wc.KV_PAGE


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


class _Inputs:
    def __init__(self, llmie, c):
        self.c, self.e4m3 = c, c.scales is not None
        self.qkv = _dev(c.qkv, torch.float16)
        self.kc, self.vc = (_dev(c.kq), _dev(c.vq)) if self.e4m3 else (_dev(c.kc, torch.float16), _dev(c.vc, torch.float16))
        self.bias = None if c.bias is None else _dev(c.bias, torch.float16)
        self.tab = _dev(c.tab)
        self.ctx = torch.tensor(c.steps, dtype=torch.int32, device=DEV)
        self.ws = torch.full((llmie.decoder_mha_workspace_bytes(c.bs, c.nh, c.hs, c.max_seq) // 4,), float("nan"), device=DEV)
        self.nan = wc.NAN_CODE if self.e4m3 else float("nan")

    def out(self):
        return torch.full((self.c.bs, self.c.nh * self.c.hs), 9.0, dtype=torch.float16, device=DEV)

    def call(self, llmie, kc, vc, window, sinks, table=None, tickets=None):
        c, out = self.c, self.out()
        llmie.decoder_mha_window(self.qkv, self.bias, kc, vc, out, 0, c.nh, c.kvh, self.ctx, self.ws, self.tab, c.rot, c.max_seq, window,
                                 sinks, block_table=table, tickets=tickets, kv_scales=c.scales)
        return out


def _same(a, b):
    """bit equality (torch.equal calls a NaN different from itself; the poison page holds NaNs)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _pool(dense, perm, filler):
    """dense [1, bs, kvh, max_seq, hs] -> pool [1, num_pages, kvh, 128, hs] under the block table perm [bs, max_pages]"""
    L, bs, kvh, max_seq, hs = dense.shape
    pages = dense.view(L, bs, kvh, MAX_PAGES, 128, hs).permute(0, 1, 3, 2, 4, 5).reshape(L, bs * MAX_PAGES, kvh, 128, hs)
    pool = filler.clone()
    pool[:, perm.flatten().long()] = pages
    return pool


def _finish_e4m3(c, x, kd, vd):
    """the reference attends to the appended rows as the device stored them (one e4m3 step of slack against the CPU's rounding)"""
    rows = {}
    for name, got, want, scale in (("K", kd, c.k_codes_new, c.scales[0]), ("V", vd, c.v_codes_new, c.scales[1])):
        rows[name] = np.stack([got[0, b, :, s - 1].cpu().numpy() for b, s in enumerate(c.steps)])
        a, e = ac.E4M3[rows[name]].astype(np.float64) * scale, ac.E4M3[want].astype(np.float64) * scale
        assert (rows[name] != want).mean() < 0.02, "%s: appended %s codes differ in %.3f of the elements" % (
            wc.describe(c, "e4m3 append"), name, (rows[name] != want).mean())
        assert (np.abs(a - e) <= 0.126 * np.abs(e) + scale * 2.0 ** -9).all(), wc.describe(c, "e4m3 append " + name)
    wc.finish(c, rows["K"], rows["V"])


def _one_case(llmie, c, rng):
    x = _Inputs(llmie, c)
    W, S = c.W, c.S
    # the unwindowed call: what the caches must look like afterwards
    k0, v0 = x.kc.clone(), x.vc.clone()
    if x.e4m3:
        x.call(llmie, k0, v0, 0, 0)
    else:
        llmie.decoder_mha_ragged(x.qkv, x.bias, k0, v0, x.out(), 0, c.nh, c.kvh, x.ctx, x.ws, x.tab, c.rot, c.max_seq)
    # dense, merge kernel
    kd, vd = x.kc.clone(), x.vc.clone()
    out = x.call(llmie, kd, vd, W, S)
    torch.cuda.synchronize()
    assert torch.equal(kd, k0) and torch.equal(vd, v0), wc.describe(c, "dense") + ": caches differ from the unwindowed call's"
    for b, s in enumerate(c.steps):   # (and that call appended: the slot differs from the input's decoy)
        assert not torch.equal(kd[0, b, :, s - 1], x.kc[0, b, :, s - 1])
    if x.e4m3:
        _finish_e4m3(c, x, kd, vd)
    rs = [wc.check(out.double().cpu().numpy(), c, "dense", BOUNDS)]
    assert bool(torch.isfinite(out).all())
    # (b) dead rows -> NaN: same bits
    dead = _dev(wc.dead_rows(c))
    kn, vn = x.kc.clone(), x.vc.clone()
    kn[0].permute(0, 2, 1, 3)[dead] = x.nan
    vn[0].permute(0, 2, 1, 3)[dead] = x.nan
    out_nan = x.call(llmie, kn, vn, W, S)
    assert torch.equal(out_nan, out), wc.describe(c, "dense, dead rows NaN") + ": a dead row was read"
    # dense, in-launch merge (native cache)
    if not x.e4m3:
        tickets = torch.zeros(c.bs * c.kvh, dtype=torch.int32, device=DEV)
        kt, vt = x.kc.clone(), x.vc.clone()
        out_t = x.call(llmie, kt, vt, W, S, tickets=tickets)
        rs.append(wc.check(out_t.double().cpu().numpy(), c, "dense, tickets", BOUNDS))
        assert int(tickets.abs().sum()) == 0, wc.describe(c, "dense, tickets") + ": tickets not back to zero"
        assert torch.equal(kt, k0) and torch.equal(vt, v0)
    # paged: the same rows behind a shuffled block table; two spare pages, the last one the poison page
    num_pages = c.bs * MAX_PAGES + 2
    perm = _dev(rng.permutation(num_pages - 1)[:c.bs * MAX_PAGES].astype(np.int32).reshape(c.bs, MAX_PAGES))
    if x.e4m3:
        filler = torch.randint(0, 0x58, (1, num_pages, c.kvh, 128, c.hs), dtype=torch.uint8, device=DEV)
    else:
        filler = (torch.randn((1, num_pages, c.kvh, 128, c.hs), device=DEV) * 0.5).to(torch.float16)
    filler[:, num_pages - 1] = x.nan
    kp, vp = _pool(x.kc, perm, filler), _pool(x.vc, perm, filler)
    kp1, vp1 = kp.clone(), vp.clone()
    out_p = x.call(llmie, kp1, vp1, W, S, table=perm)
    rs.append(wc.check(out_p.double().cpu().numpy(), c, "paged", BOUNDS))
    assert _same(kp1, _pool(k0, perm, filler)) and _same(vp1, _pool(v0, perm, filler)), wc.describe(c, "paged") + ": pools"
    # (c) wholly dead pages -> the poison page: same bits
    poisoned = perm.clone()
    poisoned[_dev(wc.dead_pages(c))] = num_pages - 1
    kp2, vp2 = kp.clone(), vp.clone()
    out_pp = x.call(llmie, kp2, vp2, W, S, table=poisoned)
    assert torch.equal(out_pp, out_p), wc.describe(c, "paged, dead pages poisoned") + ": the table entry of a dead page was followed"
    assert _same(kp2, kp1) and _same(vp2, vp1)
    if not x.e4m3:
        tickets = torch.zeros(c.bs * c.kvh, dtype=torch.int32, device=DEV)
        out_pt = x.call(llmie, kp.clone(), vp.clone(), W, S, table=poisoned, tickets=tickets)
        rs.append(wc.check(out_pt.double().cpu().numpy(), c, "paged, dead pages poisoned, tickets", BOUNDS))
        assert int(tickets.abs().sum()) == 0
    torch.cuda.synchronize()
    return max(rs)


@pytest.mark.parametrize("cid,geo,W", CASES, ids=[d[0] for d in CASES])
def test_window_decode_attention(llmie, cid, geo, W):
    rng = np.random.default_rng(5)
    worst = 0.0
    for S, steps in wc.sink_sets(W, wc.chunk_of(geo)):
        worst = max(worst, _one_case(llmie, wc.build(geo, W, S, steps), rng))
    print("%s: largest error / bound %.3f" % (cid, worst))


def test_window_decode_attention_two_chunks_per_workgroup(llmie):
    """e4m3 cache at batch 64: cpw = 2 (asserted from the plan), every condition of the test above"""
    geo = wc.CPW_GEOMETRY
    text, status = llmie.decoder_mha_window_plan(llmie.F16, wc.CPW_BATCH, wc.KVH, wc.KVH, geo[1], wc.MAX_SEQ, 100, 4, kv_e4m3=True,
                                                 forms=("rope", "ragged", "step_dev"))
    assert status == 0 and " cpw2 " in text and " chunk512 " in text, text
    rng = np.random.default_rng(5)
    for W, S, steps in wc.cpw_cases():
        r = _one_case(llmie, wc.build(geo, W, S, steps), rng)
        print("cpw2 W=%d S=%d: largest error / bound %.3f" % (W, S, r))


@pytest.mark.parametrize("geo", wc.GEOMETRIES, ids=[g[0] for g in wc.GEOMETRIES])
def test_a_window_over_the_context_has_the_unwindowed_bits(llmie, geo):
    """(a): W >= step for every sequence (W = the longest context, and far more); native cache against llmie_decoder_mha_ragged,
    e4m3 cache against the same entry without a window (the unwindowed kernel)"""
    C = wc.chunk_of(geo)
    for steps in wc.step_sets(C + 1, C) + [[1, 2, 3]]:
        c = wc.build(geo, 0, 0, steps)
        x = _Inputs(llmie, c)
        k0, v0, out0 = x.kc.clone(), x.vc.clone(), x.out()
        if x.e4m3:
            out0 = x.call(llmie, k0, v0, 0, 0)
        else:
            llmie.decoder_mha_ragged(x.qkv, x.bias, k0, v0, out0, 0, c.nh, c.kvh, x.ctx, x.ws, x.tab, c.rot, c.max_seq)
        for W, S in ((max(steps), 0), (max(steps), 4), (wc.MAX_SEQ, C + 3), (2 ** 31 - 1, 2 ** 31 - 1)):
            k1, v1 = x.kc.clone(), x.vc.clone()
            out1 = x.call(llmie, k1, v1, W, S)
            assert torch.equal(out1, out0) and torch.equal(k1, k0) and torch.equal(v1, v0), wc.describe(c, "W=%d S=%d" % (W, S))
        if not x.e4m3:
            assert torch.equal(x.call(llmie, x.kc.clone(), x.vc.clone(), 0, 0), out0)
    torch.cuda.synchronize()


def test_windowed_forms_without_a_kernel_write_nothing(llmie):
    """fp32 / head size 32 with a window: an error, caches and output untouched"""
    for dtype, hs in ((torch.float32, 128), (torch.float16, 32)):
        bs, nh, kvh, max_seq = 2, 4, 2, 256
        qkv = torch.randn((bs, nh + 2 * kvh, hs), device=DEV).to(dtype)
        kc = torch.randn((1, bs, kvh, max_seq, hs), device=DEV).to(dtype)
        vc, out = kc.clone(), torch.full((bs, nh * hs), 9.0, dtype=dtype, device=DEV)
        k0 = kc.clone()
        ws = torch.zeros(llmie.decoder_mha_workspace_bytes(bs, nh, hs, max_seq) // 4, device=DEV)
        ctx = torch.tensor([200, 7], dtype=torch.int32, device=DEV)
        tab = _dev(ac.rope_table(max_seq, hs, hs))
        with pytest.raises(llmie.LlmieError, match="window"):
            llmie.decoder_mha_window(qkv, None, kc, vc, out, 0, nh, kvh, ctx, ws, tab, hs, max_seq, 16, 4)
        torch.cuda.synchronize()
        assert torch.equal(kc, k0) and torch.equal(vc, k0) and bool((out == 9.0).all())


def test_the_page_ring_follows_its_restatement(llmie):
    """llmie_kv_window_advance against wc.ring_advance: four sequences at different phases walked one token at a time through the
    same loop, with exactly the formula's pages / one page less / more tokens per step / a prefill-sized first step"""
    max_pages, W, S = 6, 200, 4
    pool = wc.ring_pages(W, S)
    rows = [[-1] * max_pages for _ in range(4)]
    free = [list(range(100 * b, 100 * b + pool - (1 if b == 1 else 0))) for b in range(4)]
    cached, n_new = [0, 0, 5, 0], [1, 1, 3, 1]
    table = torch.full((4, max_pages), -1, dtype=torch.int32, device=DEV)
    seen_fail = None
    for it in range(800):
        for b in range(4):   # the caller supplies its own pages while it has any
            for p in range(cached[b] // 128, (cached[b] + n_new[b] - 1) // 128 + 1):
                if p < max_pages and rows[b][p] < 0 and free[b]:
                    rows[b][p] = free[b].pop(0)
        exp = [wc.ring_advance(rows[b], cached[b], n_new[b], W, S) for b in range(4)]
        table.copy_(torch.tensor(rows, dtype=torch.int32))
        status = llmie.kv_window_advance(table, torch.tensor(cached, dtype=torch.int32, device=DEV), W, S,
                                         new_tokens=torch.tensor(n_new, dtype=torch.int32, device=DEV))
        got_rows, got_status = table.cpu().tolist(), status.cpu().tolist()
        assert got_status == [e[1] for e in exp] and got_rows == [e[0] for e in exp], (it, cached, got_status, got_rows, exp)
        if got_status[1] == 1 and seen_fail is None:
            seen_fail = cached[1]
        for b in range(4):
            if got_status[b] == 0:
                rows[b] = got_rows[b]
                cached[b] += n_new[b]
        if all(s != 0 for s in got_status):
            break
    assert seen_fail == 3 * 128, seen_fail                       # one page short: the first token of the page it lacks
    assert got_status[0] == 2 and cached[0] == max_pages * 128   # the full pool ran to the end of the table with status 0
    assert got_status[2] == 2 and cached[2] > max_pages * 128 - 3
    # new_tokens = NULL is one token each
    table.copy_(torch.tensor([[0, 1, 2, -1] + [-1] * (max_pages - 4)] * 4, dtype=torch.int32))
    status = llmie.kv_window_advance(table, torch.tensor([384] * 4, dtype=torch.int32, device=DEV), 100, 0)
    assert status.cpu().tolist() == [0] * 4 and table.cpu().tolist() == [[-1, 1, 2, 0] + [-1] * (max_pages - 4)] * 4
