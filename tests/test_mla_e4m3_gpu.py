"""MLA on the e4m3 latent cache, on the GPU.  Decode against a float64 plain softmax in the absorbed form over the rows AS STORED:
latent = LUT[byte] * c_scale (LUT: torch's uint8 -> float8_e4m3fn -> float64 on the CPU), k_pe = the fp16 bits, the query = the fp16
q_lat the kernel is given.  The latent bytes are written directly, uniform over the 254 finite codes, so subnormal codes and +-448 sit
in every tile; c_scale = 0.0123 is no power of two.  Bound per element, that of tests/test_mla_gpu.py by the same derivation (the
code -> fp16 conversion is exact and c_scale is applied in fp32, so P and the output are the two fp16 roundings):
|err| <= 2^-10 max_t |v_t| + 2^-10 |ref|, v_t the dequantised latent.  Append, bulk append and dequant are checked bit for bit.

Measured on an MI355X, worst error / bound: 16 heads 0.217 (ctx 33), 32 heads 0.203 (ctx 32); ragged batch 0.209 (dense = paged);
chain 0.230 (o_lat) / 0.183 (out).
"""
import functools
import re
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV, EPS, L, LAYER, SCALE, RMS_EPS, SENTINEL = "cuda:0", 2.0 ** -10, 2, 1, 1.0 / 6.0, 1e-6, 777.0
CS = float(np.float32(0.0123))
LUT = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).double().numpy()
FINITE = np.array([c for c in range(256) if c not in (0x7f, 0xff)], np.uint8)
DECOY = np.concatenate([np.full(512, 0x7e, np.uint8), np.full(64, 1e4, np.float16).view(np.uint8)])
d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
f16 = lambda a: a.astype(np.float16)
quant = lambda x, cs: (torch.as_tensor(x).float() / cs).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


@pytest.fixture(scope="module")
def mla(llmie):
    llmie.build()
    m = re.search(r"tile(\d+) chunk(\d+)", llmie.mla_decode_e4m3_plan(1, 16, 128)[0])
    return types.SimpleNamespace(lib=llmie, T=int(m[1]), C=int(m[2]))


def rows_of(cache_bytes, cs=CS):
    return np.concatenate([LUT[cache_bytes[..., :512]] * cs, cache_bytes[..., 512:].copy().view(np.float16).astype(np.float64)], -1)


@functools.lru_cache(maxsize=None)
def make_case(T, heads, ctxs):
    rng = np.random.default_rng(1000 * heads + sum(ctxs))
    c = types.SimpleNamespace(heads=heads, ctxs=ctxs, B=len(ctxs), S=max(128, -(-max(ctxs) // 128) * 128))
    c.cache = np.empty((L, c.B, c.S, 640), np.uint8)
    c.cache[..., :512] = rng.choice(FINITE, (L, c.B, c.S, 512))
    c.cache[..., 512:] = (0.5 * rng.standard_normal((L, c.B, c.S, 64))).astype(np.float16).view(np.uint8)
    rms = np.sqrt((rows_of(c.cache[LAYER]) ** 2).mean())
    c.q_lat = (rng.standard_normal((c.B, heads, 576)) * 2 / (SCALE * rms * 24)).astype(np.float16)   # logit std ~2: sqrt(576) = 24
    for b, ctx in ((b, x) for b, x in enumerate(ctxs) if x >= 1):
        for h, t in ((0, ctx - 1), (1, (ctx - 1) // T * T)):   # dominant keys: logit ~16 above the rest
            ql = c.q_lat[b, h, :512].astype(np.float64)
            c.cache[LAYER, b, t, :512] = quant(16 / SCALE * ql / (ql ** 2).sum(), CS)
        if ctx < c.S:
            c.cache[LAYER, b, ctx] = DECOY
    return c


def reference(c, b, ctx):
    rows, q = rows_of(c.cache[LAYER, b, :ctx]), c.q_lat[b].astype(np.float64)
    logits = SCALE * q @ rows.T
    p = np.exp(logits - logits.max(-1, keepdims=True))
    o = p / p.sum(-1, keepdims=True) @ rows[:, :512]
    return o, EPS * np.abs(rows[:, :512]).max(0) + EPS * np.abs(o), logits


def paged_copy(dense, B, S, row=640, fill=DECOY):
    mp = S // 128   # shuffled table, two spare pages, decoys (`fill`) wherever no row lives
    table = torch.randperm(B * mp + 2, generator=torch.Generator().manual_seed(B))[:B * mp].reshape(B, mp).to(DEV)
    cache = d(np.broadcast_to(fill, (dense.shape[0], B * mp + 2, 128, row)).copy()).to(dense.dtype)
    cache[:, table.flatten()] = dense.view(dense.shape[0], B * mp, 128, row)
    return cache, table.int().contiguous()


def decode(mla, c, paged, only=None):
    sl = slice(None) if only is None else slice(only, only + 1)
    ctxs = c.ctxs[sl]
    cache, kw = d(c.cache[:, sl]), {}
    if paged:
        cache, table = paged_copy(cache, len(ctxs), c.S)
        kw = dict(block_table=table, max_seq_len=c.S)
    o = torch.full((len(ctxs), c.heads, 512), SENTINEL, dtype=torch.float16, device=DEV)
    mla.lib.mla_decode_e4m3(d(c.q_lat[sl]), cache, CS, LAYER, d(np.asarray(ctxs, np.int32)), SCALE, o, mla.lib.mla_workspace(len(ctxs), c.heads, c.S), **kw)
    return o


def check(what, got, ref, bound):
    ratio = (np.abs(got.double().cpu().numpy().reshape(ref.shape) - ref) / bound).max()
    print("%s: worst error / bound %.3f" % (what, ratio))
    assert ratio <= 1.0, what


@pytest.mark.parametrize("expr", ("1", "T-1", "T", "T+1", "128", "129", "C", "C+1", "2*C+T+3"))
@pytest.mark.parametrize("heads", [16, 32])
def test_decode_dense_and_paged(mla, heads, expr):
    ctx = eval(expr, {"T": mla.T, "C": mla.C})
    c = make_case(mla.T, heads, (ctx,))
    o, bound, logits = reference(c, 0, ctx)
    if ctx > 1:   # (one key has no spread.)  Heads 2.. have no dominant key: their softmax is not one-hot, the PV product shows
        assert 1 <= logits[2:].std() <= 4, logits[2:].std()
    dense = decode(mla, c, False)
    check("heads %d ctx %d (%s) dense" % (heads, ctx, expr), dense[0], o, bound)
    assert torch.equal(decode(mla, c, True), dense), "paged differs from dense"


@pytest.mark.parametrize("paged", [False, True])
def test_ragged_batch_rows_equal_the_batch_1_calls(mla, paged):
    ctxs = (mla.C + 1, 0, mla.T - 1, 2 * mla.C + mla.T + 3)
    c = make_case(mla.T, 32, ctxs)
    o = decode(mla, c, paged)
    assert (o[1] == SENTINEL).all(), "the sequence at ctx_len 0 was written"
    for b in (0, 2, 3):
        ref, bound, _ = reference(c, b, ctxs[b])
        check("ragged row %d ctx %d paged=%s" % (b, ctxs[b], paged), o[b], ref, bound)
        assert torch.equal(decode(mla, c, paged, only=b)[0], o[b]), "row %d differs from its batch-1 call" % b


def append_inputs(llmie, n, S, seed):
    rng = np.random.default_rng(seed)
    return (f16(0.5 * rng.standard_normal((n, 576))), f16(1 + 0.1 * rng.uniform(-1, 1, 512)), d(llmie.rope_table(S, 64, 64, 10000.0)),
            rng.integers(0, 256, (L, 3, S, 640), dtype=np.uint8))


@pytest.mark.parametrize("gamma_scale", [1, 64])
@pytest.mark.parametrize("paged", [False, True])
def test_append_quantises_the_fp16_row(mla, paged, gamma_scale):
    llmie, S, ctxs, cs = mla.lib, 256, (129, 0, 256), 2.0 ** -5   # (the division by 2^-5 is exact)
    kv_a, gamma, tab, fill = append_inputs(llmie, 3, S, 5)
    gamma, ctx_len = d(gamma * np.float16(gamma_scale)), d(np.asarray(ctxs, np.int32))
    c8, c16, kw = d(fill), torch.zeros((L, 3, S, 576), dtype=torch.float16, device=DEV), {}
    if paged:
        (c8, table), c16 = paged_copy(c8, 3, S, fill=np.uint8(9)), paged_copy(c16, 3, S, 576, np.float16(0))[0]
        kw = dict(block_table=table, max_seq_len=S)
    before = c8.clone()
    llmie.mla_kv_append(d(kv_a), gamma, RMS_EPS, tab, c16, LAYER, ctx_len, **kw)
    llmie.mla_kv_append_e4m3(d(kv_a), gamma, RMS_EPS, tab, c8, cs, LAYER, ctx_len, **kw)
    for b, ctx in ((b, x) for b, x in enumerate(ctxs) if x >= 1):
        at = (int(table[b, (ctx - 1) // 128]), (ctx - 1) % 128) if paged else (b, ctx - 1)
        got, row16 = c8[LAYER, at[0], at[1]].cpu().numpy(), c16[LAYER, at[0], at[1]].cpu()
        assert np.array_equal(got[:512], quant(row16[:512], cs)), "latent bytes of sequence %d" % b
        assert np.array_equal(got[512:].view(np.float16), row16[512:].numpy()), "k_pe bits of sequence %d" % b
        assert not np.isin(got[:512], (0x7f, 0xff)).any() and (gamma_scale == 1 or {0x7e, 0xfe} <= set(got[:512]))
        before[LAYER, at[0], at[1]] = c8[LAYER, at[0], at[1]]
    assert torch.equal(c8, before), "the append changed something outside the appended rows"


@pytest.mark.parametrize("paged", [False, True])
def test_bulk_append_equals_single_token_appends(mla, paged):
    llmie, S, lens, hists = mla.lib, 256, (3, 0, 5), (0, 7, 126)   # sequence 2 crosses the page boundary at 128
    cum = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    kv_a, gamma, tab, fill = append_inputs(llmie, int(cum[-1]), S, 6)
    bulk, kw = d(fill), {}
    if paged:
        bulk, table = paged_copy(bulk, 3, S, fill=np.uint8(9))
        kw = dict(block_table=table, max_seq_len=S)
    start, single = bulk.clone(), bulk.clone()
    llmie.mla_kv_append_rows_e4m3(d(kv_a), d(gamma), RMS_EPS, tab, bulk, CS, LAYER, d(cum), d(np.asarray(hists, np.int32)), max(lens), S, **kw)
    for i in range(max(lens)):
        step = np.stack([kv_a[cum[b] + i] if i < n else kv_a[0] for b, n in enumerate(lens)])
        ctx_len = np.asarray([h + i + 1 if i < n else 0 for h, n in zip(hists, lens)], np.int32)
        llmie.mla_kv_append_e4m3(d(step), d(gamma), RMS_EPS, tab, single, CS, LAYER, d(ctx_len), **kw)
    assert (bulk != start).any(dim=-1).sum() == sum(lens) and torch.equal(bulk, single)   # 8 rows written, the same bytes both ways


@pytest.mark.parametrize("paged", [False, True])
def test_dequant_is_exact_and_stops_at_ctx(mla, paged):
    ctxs = (mla.C + 1, 0, mla.T - 1)
    c = make_case(mla.T, 16, ctxs)
    c8, c16, kw = d(c.cache), torch.full((L, c.B, c.S, 576), SENTINEL, dtype=torch.float16, device=DEV), {}
    want = c16.clone()
    for b, ctx in enumerate(ctxs):
        rows = torch.from_numpy(c.cache[LAYER, b, :ctx])
        want[LAYER, b, :ctx, :512] = (rows[:, :512].view(torch.float8_e4m3fn).float() * torch.tensor(CS)).half().to(DEV)
        want[LAYER, b, :ctx, 512:] = rows[:, 512:].contiguous().view(torch.float16).to(DEV)
    if paged:
        (c8, table), c16, want = paged_copy(c8, c.B, c.S), paged_copy(c16, c.B, c.S, 576, np.float16(SENTINEL))[0], paged_copy(want, c.B, c.S, 576, np.float16(SENTINEL))[0]
        kw = dict(block_table=table, max_seq_len=c.S)
    mla.lib.mla_cache_dequant_e4m3(c8, c16, CS, LAYER, d(np.asarray(ctxs, np.int32)), **kw)
    assert torch.equal(c16.view(torch.int16), want.view(torch.int16))


def test_chain_append_absorb_decode_out_project(mla):
    """the un-absorbed float64 reference (k = W_UK c || k_pe, v = W_UV c) over the stored rows; bounds of test_chain_absorb_decode_out_project"""
    llmie, heads, ctx, S = mla.lib, 16, mla.C + 1, 384
    rng = np.random.default_rng(7)
    kv_b, q = f16(rng.standard_normal((heads, 256, 512)) / np.sqrt(128)), f16(rng.standard_normal((1, heads, 192)))
    cache = np.zeros((L, 1, S, 640), np.uint8)
    cache[..., :512] = quant(0.5 * rng.standard_normal((L, 1, S, 512)), CS)
    cache[..., 512:] = f16(0.5 * rng.standard_normal((L, 1, S, 64))).view(np.uint8)
    cache[LAYER, 0, ctx] = DECOY
    kv_a, gamma, tab, _ = append_inputs(llmie, 1, S, 8)
    c8, ctx_len = d(cache), d(np.asarray([ctx], np.int32))
    llmie.mla_kv_append_e4m3(d(kv_a), d(gamma), RMS_EPS, tab, c8, CS, LAYER, ctx_len)
    q_lat = llmie.mla_q_absorb(d(q), d(kv_b), tab, torch.empty((1, heads, 576), dtype=torch.float16, device=DEV), ctx_len, S)
    o = llmie.mla_decode_e4m3(q_lat, c8, CS, LAYER, ctx_len, SCALE, torch.empty((1, heads, 512), dtype=torch.float16, device=DEV),
                              llmie.mla_workspace(1, heads, S))
    out = llmie.mla_out_project(o, d(kv_b), torch.empty((1, heads * 128), dtype=torch.float16, device=DEV))
    rows, W, qd = rows_of(c8[LAYER, 0, :ctx].cpu().numpy()), kv_b.astype(np.float64), q[0].astype(np.float64)
    lat, pe, tb = rows[:, :512], rows[:, 512:], tab.cpu().numpy().astype(np.float64)[ctx - 1]
    q_rot = np.concatenate([qd[:, 128:160] * tb[:, 0] - qd[:, 160:] * tb[:, 1], qd[:, 160:] * tb[:, 0] + qd[:, 128:160] * tb[:, 1]], -1)
    k_nope, v = np.einsum("tc,hnc->htn", lat, W[:, :128]), np.einsum("tc,hvc->htv", lat, W[:, 128:])
    logits = SCALE * (np.einsum("hn,htn->ht", qd[:, :128], k_nope) + q_rot @ pe.T)
    p = np.exp(logits - logits.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    check("chain o_lat", o[0], p @ lat, EPS * np.abs(lat).max(0) + EPS * np.abs(p @ lat))
    check("chain out", out[0], np.einsum("ht,htv->hv", p, v), EPS * np.abs(v).max(1) + EPS * np.abs(np.einsum("ht,htv->hv", p, v)))
