"""llmie_decoder_mha_qknorm (the QKN instantiations of the decode split kernel) against the composition it fuses, BIT FOR BIT:
llmie_qk_norm on a copy of qkv, then llmie_decoder_mha_sink(head_sink = NULL) on the same operands -- the output, the caches and,
paged, the pools.  The un-normed entry is held to its float64 reference by its own tests and the operator by
tests/test_qknorm_op_gpu.py, so no tolerance enters here.

Batch 3 ragged over 2 KV heads, qknorm_cases.op_inputs rows as qkv, caches uniform +-0.5 (e4m3: random codes at
model_param_cases' scales); head sizes 128 / 64 at ratios 1, 2, 8 over the fp16 cache and 1, 4 over e4m3.  The context lengths come
FROM THE PLAN TEXT'S CHUNK: {1, 2, chunk, chunk + 1, 129, 2 chunk + 37} over two launches -- the new token alone, the new token as
the first row of a second split, a page boundary, several splits.  Each launch dense and paged (shuffled block table), with the merge
kernel and (fp16 cache) with tickets.  Also: the norm matters (the plain call on the raw rows differs), both gammas NULL is
llmie_decoder_mha_sink's call, a row's bits do not depend on its batch slot, a captured launch replays with the gammas of the replay,
and a form without a kernel writes nothing.
"""
import re

import numpy as np
import pytest
import torch

import attn_cases as ac
import model_param_cases as mpc
import qknorm_cases as qc

pytestmark = pytest.mark.gpu
DEV, F16 = "cuda", torch.float16
KVH, BS, EPS = 2, 3, 1e-6
FORMS = ("rope", "ragged", "step_dev", "qk_norm")
# head size, head ratio, e4m3 cache
GEOMETRIES = [(hs, r, False) for hs in (128, 64) for r in (1, 2, 8)] + [(hs, r, True) for hs in (128, 64) for r in (1, 4)]


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _plan_chunk(llmie, hs, ratio, e4m3, **kw):
    text, status = llmie.decoder_mha_qknorm_plan(llmie.F16, BS, KVH * ratio, KVH, hs, 4096, kv_e4m3=e4m3, forms=FORMS, **kw)
    assert status == 0 and text.endswith(" qk_norm"), text
    m = re.search(r" cpw(\d+) chunk(\d+) ", text)
    assert int(m.group(1)) == 1
    return int(m.group(2))


class _Case:
    def __init__(self, llmie, hs, ratio, e4m3, steps, max_seq, seed):
        rng = np.random.default_rng(seed)
        self.hs, self.nh, self.e4m3, self.max_seq, self.llmie = hs, KVH * ratio, e4m3, max_seq, llmie
        self.qkv = _dev(qc.op_inputs(BS, self.nh, KVH, hs, seed))
        qg, kg = qc.gammas(1, hs, seed + 1)
        self.qg, self.kg = _dev(qg[0]), _dev(kg[0])
        shape = (1, BS, KVH, max_seq, hs)
        if e4m3:
            code = lambda: (rng.integers(0, 0x58, shape).astype(np.uint8) | (rng.integers(0, 2, shape).astype(np.uint8) << 7))
            self.kc, self.vc, self.scales = _dev(code()), _dev(code()), (mpc.KS, mpc.VS)
        else:
            self.kc, self.vc, self.scales = _dev(rng.uniform(-0.5, 0.5, shape), F16), _dev(rng.uniform(-0.5, 0.5, shape), F16), None
        self.tab = _dev(ac.rope_table(max_seq, hs, hs))
        self.ctx = torch.tensor(steps, dtype=torch.int32, device=DEV)
        self.ws = torch.full((llmie.decoder_mha_workspace_bytes(BS, self.nh, hs, max_seq) // 4,), float("nan"), device=DEV)
        self.pages = max_seq // 128

    def out(self):
        return torch.full((BS, self.nh * self.hs), 9.0, dtype=F16, device=DEV)

    def fused(self, kc, vc, table=None, tickets=None, qkv=None, ctx=None, gammas=True, out=None):
        out = self.out() if out is None else out
        self.llmie.decoder_mha_qknorm(self.qkv if qkv is None else qkv, None, kc, vc, out, 0, self.nh, KVH, self.ctx if ctx is None else ctx, self.ws,
                                      self.tab, self.hs, self.max_seq, self.qg if gammas else None, self.kg if gammas else None, EPS,
                                      block_table=table, tickets=tickets, kv_scales=self.scales)
        return out

    def composed(self, kc, vc, table=None, tickets=None, qkv=None, ctx=None, norm=True):
        q = (self.qkv if qkv is None else qkv).clone()
        if norm:
            self.llmie.qk_norm(q, self.nh, KVH, self.qg, self.kg, EPS)
        out = self.out()
        self.llmie.decoder_mha_sink(q, None, kc, vc, out, 0, self.nh, KVH, self.ctx if ctx is None else ctx, self.ws, self.tab, self.hs, self.max_seq,
                                    None, block_table=table, tickets=tickets, kv_scales=self.scales)
        return out

    def pool(self, dense, perm, filler):
        L, bs, kvh, max_seq, hs = dense.shape
        pages = dense.view(L, bs, kvh, self.pages, 128, hs).permute(0, 1, 3, 2, 4, 5).reshape(L, bs * self.pages, kvh, 128, hs)
        pool = filler.clone()
        pool[:, perm.flatten().long()] = pages
        return pool


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _one_launch(x, rng, what):
    tickets = lambda: torch.zeros(BS * KVH, dtype=torch.int32, device=DEV)
    # dense, merge kernel
    kc1, vc1, kc2, vc2 = x.kc.clone(), x.vc.clone(), x.kc.clone(), x.vc.clone()
    exp, got = x.composed(kc1, vc1), x.fused(kc2, vc2)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(exp.float()).all())
    assert _same(got, exp), what + ": output differs from qk_norm + decoder_mha_sink in %d elements" % int((got != exp).sum())
    assert _same(kc2, kc1) and _same(vc2, vc1) and not _same(kc1, x.kc), what + ": caches"
    # the norm matters; both gammas NULL: the plain call's bits
    kc3, vc3, kc4, vc4 = x.kc.clone(), x.vc.clone(), x.kc.clone(), x.vc.clone()
    plain, null = x.composed(kc3, vc3, norm=False), x.fused(kc4, vc4, gammas=False)
    assert _same(null, plain) and _same(kc4, kc3) and _same(vc4, vc3), what + ": gammas NULL is not decoder_mha_sink's call"
    assert not _same(plain, exp) and not _same(kc3, kc1) and _same(vc3, vc1), what + ": the norm does not matter (or touched v)"
    if not x.e4m3:   # in-launch merge: the bits of the merge kernel
        t, kt, vt = tickets(), x.kc.clone(), x.vc.clone()
        assert _same(x.fused(kt, vt, tickets=t), exp) and int(t.abs().sum()) == 0 and _same(kt, kc1) and _same(vt, vc1), what + ": tickets"
    # the rows in other batch slots
    idx = torch.tensor([2, 0, 1], device=DEV)
    out_r = x.fused(x.kc[:, idx].contiguous(), x.vc[:, idx].contiguous(), qkv=x.qkv[idx].contiguous(), ctx=x.ctx[idx].contiguous())
    assert _same(out_r, exp[idx]), what + ": a row's bits depend on its batch slot"
    # paged: the same rows behind a shuffled block table
    num_pages = BS * x.pages + 1
    perm = _dev(rng.permutation(num_pages)[:BS * x.pages].astype(np.int32).reshape(BS, x.pages))
    if x.e4m3:
        filler = torch.randint(0, 0x58, (1, num_pages, KVH, 128, x.hs), dtype=torch.uint8, device=DEV)
    else:
        filler = (torch.randn((1, num_pages, KVH, 128, x.hs), device=DEV) * 0.5).to(F16)
    kp1, vp1, kp2, vp2 = x.pool(x.kc, perm, filler), x.pool(x.vc, perm, filler), x.pool(x.kc, perm, filler), x.pool(x.vc, perm, filler)
    exp_p, got_p = x.composed(kp1, vp1, table=perm), x.fused(kp2, vp2, table=perm)
    assert _same(got_p, exp_p) and _same(got_p, exp), what + ", paged: output"
    assert _same(kp2, kp1) and _same(vp2, vp1) and _same(kp2, x.pool(kc1, perm, filler)), what + ", paged: pools"
    if not x.e4m3:
        t = tickets()
        assert _same(x.fused(x.pool(x.kc, perm, filler), x.pool(x.vc, perm, filler), table=perm, tickets=t), exp) and int(t.abs().sum()) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("hs,ratio,e4m3", GEOMETRIES, ids=["hs%d-r%d-%s" % (h, r, "e4m3" if e else "f16") for h, r, e in GEOMETRIES])
def test_fused_equals_the_composition(llmie, hs, ratio, e4m3):
    chunk = _plan_chunk(llmie, hs, ratio, e4m3)
    assert chunk == ac.chunk_len(ac.F16, hs, e4m3=e4m3)
    max_seq = (2 * chunk + 37 + 127) // 128 * 128
    rng = np.random.default_rng(5)
    for i, steps in enumerate(([1, chunk, 129], [2, chunk + 1, 2 * chunk + 37])):
        _one_launch(_Case(llmie, hs, ratio, e4m3, steps, max_seq, seed=10 * hs + ratio + i), rng, "hs %d ratio %d %s steps %s" % (hs, ratio, "e4m3" if e4m3 else "f16", steps))


def test_a_replayed_launch_reads_the_gammas_of_the_replay(llmie):
    chunk = _plan_chunk(llmie, 128, 8, False)
    x = _Case(llmie, 128, 8, False, [2, chunk + 1, 2 * chunk + 37], (2 * chunk + 37 + 127) // 128 * 128, seed=3)
    kd, vd, out = x.kc.clone(), x.vc.clone(), x.out()
    x.fused(kd, vd, out=out)   # eager once
    torch.cuda.synchronize()
    first = out.clone()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(graph, stream=side):
        x.fused(kd, vd, out=out)
    for seed in (21, 22):
        qg, kg = qc.gammas(1, 128, seed)
        x.qg.copy_(_dev(qg[0]))
        x.kg.copy_(_dev(kg[0]))
        out.fill_(9.0)
        graph.replay()
        torch.cuda.synchronize()
        exp = x.composed(x.kc.clone(), x.vc.clone())
        assert _same(out, exp) and not _same(out, first), "replay with the gammas of seed %d" % seed


def test_forms_without_a_kernel_write_nothing(llmie):
    """a QKV bias, a window, a head sink, fp32, head size 32, unaligned qkv, ratio 8 over e4m3: LLMIE_ERR_UNSUPPORTED, nothing written"""
    forms = [("bias", dict(bias=True)), ("window", dict(window=64)), ("head sink", dict(sink=True)), ("fp32", dict(dtype=torch.float32)),
             ("head size 32", dict(hs=32)), ("unaligned qkv", dict(skew=4)), ("ratio 8 over e4m3", dict(nh=16, e4m3=True))]
    for what, f in forms:
        dtype, hs, skew, nh, e4m3 = f.get("dtype", F16), f.get("hs", 128), f.get("skew", 0), f.get("nh", 4), f.get("e4m3", False)
        bs, kvh, max_seq = 2, 2, 256
        n = bs * (nh + 2 * kvh) * hs
        qkv = torch.randn((n + 8,), device=DEV).to(dtype)[skew:skew + n].view(bs, nh + 2 * kvh, hs)
        kc = torch.randint(0, 0x58, (1, bs, kvh, max_seq, hs), dtype=torch.uint8, device=DEV) if e4m3 else torch.randn((1, bs, kvh, max_seq, hs), device=DEV).to(dtype)
        vc, out = kc.clone(), torch.full((bs, nh * hs), 9.0, dtype=dtype, device=DEV)
        k0 = kc.clone()
        ws = torch.zeros(llmie.decoder_mha_workspace_bytes(bs, nh, hs, max_seq) // 4, device=DEV)
        ctx = torch.tensor([200, 7], dtype=torch.int32, device=DEV)
        tab = _dev(ac.rope_table(max_seq, hs, hs))
        g = torch.ones(hs, dtype=dtype, device=DEV)
        with pytest.raises(llmie.LlmieError, match=r"\(-2\)"):
            llmie.decoder_mha_qknorm(qkv, torch.zeros((nh + 2 * kvh) * hs, dtype=dtype, device=DEV) if f.get("bias") else None, kc, vc, out, 0, nh,
                                     kvh, ctx, ws, tab, hs, max_seq, g, g, EPS, head_sink=torch.zeros(nh, device=DEV) if f.get("sink") else None,
                                     window=f.get("window", 0), kv_scales=(0.5, 0.5) if e4m3 else None)
        torch.cuda.synchronize()
        assert torch.equal(kc, k0) and torch.equal(vc, k0) and bool((out == 9.0).all()), what
