"""MLA verify attention (llmie_mla_verify) on the GPU against a float64 softmax over the cache rows as stored, with the mask applied.
Bound, as derived in tests/test_mla_gpu.py (P rounded to fp16 before the PV MFMA, one fp16 rounding of the output, a factor 2 for the
fp32 accumulation order): |err| <= 2^-10 max_t |c_t| + 2^-10 |ref| per element, the maximum over the keys the row sees.  Inputs: latents
0.5 N(0, 1), q_lat N(0, 1) (logits of standard deviation 2 at scale 1/6), a decoy row of 1e4 at slot ctx (dense) and in every page
outside the block table (paged).  The masks are passed WITHOUT the self bit and with bit 63 set, which the convention of
llmie_decoder_set_tree forces and strips.  A tree case also asserts that the chain mask's reference lies outside the bound.
"""
import functools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV, EPS, L, LAYER, SCALE, RMS_EPS, SENTINEL = "cuda:0", 2.0 ** -10, 2, 1, 1.0 / 6.0, 1e-6, 777.0
PARENTS = {"forest": (-1, 0, 1, -1, 3, 2), "tree": (-1, 0, 0, 1, 1, 2, 3, 3, 5)}
CASES = [(0, 1, "chain"), (0, 5, "chain"), (31, 4, "chain"), (127, 3, "chain"), (254, 4, "chain"), (0, 6, "forest"), (130, 9, "tree"),
         (257, 64, "chain")]


@pytest.fixture(scope="module")
def lib(llmie):
    llmie.build()
    return llmie


def masks(kind, rows):
    """what row i sees among the nodes (python ints, self bit in)"""
    m = []
    for i, p in enumerate(range(-1, rows - 1) if kind == "chain" else PARENTS[kind]):
        m.append((1 << i) | (m[p] if p >= 0 else 0))
    return m


@functools.lru_cache(maxsize=None)
def make_case(heads, spans, rows):
    """spans: (hist, count) per sequence, count <= 0 or > rows: a dead sequence"""
    rng = np.random.default_rng(1000 * heads + 10 * sum(h for h, _ in spans) + rows)
    live = [h + n for h, n in spans if 1 <= n <= rows]
    c = types.SimpleNamespace(heads=heads, spans=spans, rows=rows, B=len(spans), S=max(128, -(-max(live) // 128) * 128))
    c.cache = (0.5 * rng.standard_normal((L, c.B, c.S, 576))).astype(np.float16)
    c.q_lat = rng.standard_normal((c.B, rows, heads, 576)).astype(np.float16)
    for b, (h, n) in enumerate(spans):
        if 1 <= n <= rows and h + n < c.S:
            c.cache[LAYER, b, h + n] = 1e4
    return c


def reference(q_lat, stored, hist, see):
    """(o_lat [rows, heads, 512], bound) in float64; see[i]: row i's node mask"""
    o, bound = [], []
    for i, m in enumerate(see):
        keys = stored[[t for t in range(hist + i + 1) if t < hist or (m >> (t - hist)) & 1]]
        logits = SCALE * q_lat[i].astype(np.float64) @ keys.T
        p = np.exp(logits - logits.max(-1, keepdims=True))
        o.append(p / p.sum(-1, keepdims=True) @ keys[:, :512])
        bound.append(EPS * np.abs(keys[:, :512]).max(0) + EPS * np.abs(o[-1]))
    return np.stack(o), np.stack(bound)


def run(lib, c, paged, kind="chain", only=None, max_ctx=0, q_lat=None, cache=None):
    """the verify call on the device (only = b: the batch-1 call of sequence b) -> o_lat [B, rows, heads, 512], sentinel where unwritten"""
    sl = slice(None) if only is None else slice(only, only + 1)
    spans, d = c.spans[sl], lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    B, cache, table, kw = len(spans), d(c.cache[:, sl]) if cache is None else cache, None, {}
    if paged:   # shuffled table, two spare pages, decoys wherever no row lives
        mp = c.S // 128
        table = torch.randperm(B * mp + 2, generator=torch.Generator().manual_seed(B))[:B * mp].reshape(B, mp).to(DEV)
        pool = torch.full((L, B * mp + 2, 128, 576), 1e4, dtype=torch.float16, device=DEV)
        pool[:, table.flatten()] = cache.view(L, B * mp, 128, 576)
        cache, kw = pool, dict(block_table=table.int().contiguous(), max_seq_len=c.S)
    anc = None
    if kind != "chain":   # no self bit, bit 63 set: the kernel forces the one and strips the other
        a = np.array([(m & ~(1 << i)) | (1 << 63) for i, m in enumerate(masks(kind, c.rows))], dtype=np.uint64)
        anc = d(np.tile(a, (B, 1)).view(np.int64))
    o = torch.full((B, c.rows, c.heads, 512), SENTINEL, dtype=torch.float16, device=DEV)
    lib.mla_verify(d(c.q_lat[sl]) if q_lat is None else q_lat, cache, LAYER, d(np.array([h for h, _ in spans], np.int32)), SCALE, o,
                   count=d(np.array([n for _, n in spans], np.int32)), anc=anc,
                   workspace=lib.mla_verify_workspace(B, c.rows, c.heads, max_ctx or c.S), max_ctx=max_ctx, **kw)
    torch.cuda.synchronize()
    return o


def check(what, got, ref, bound):
    err = np.abs(got.double().cpu().numpy() - ref)
    print("%s: worst error / bound %.3f" % (what, (err / bound).max()))
    assert (err <= bound).all(), what
    return err.max()


@pytest.mark.parametrize("hist,rows,kind", CASES)
@pytest.mark.parametrize("heads", [16, 32])
def test_verify_dense_and_paged(lib, heads, hist, rows, kind):
    c = make_case(heads, ((hist, rows),), rows)
    stored = c.cache[LAYER, 0].astype(np.float64)
    ref, bound = reference(c.q_lat[0], stored, hist, masks(kind, rows))
    if kind != "chain":   # the case discriminates: ignoring anc is outside the bound somewhere
        assert (np.abs(reference(c.q_lat[0], stored, hist, masks("chain", rows))[0] - ref) > bound).any()
    dense = run(lib, c, False, kind)
    err = check("heads %d hist %d rows %d %s" % (heads, hist, rows, kind), dense[0], ref, bound)
    assert hist + rows > 1 or err == 0.0, "a single key is exact"
    assert torch.equal(run(lib, c, True, kind), dense), "paged differs from dense"


@pytest.mark.parametrize("paged", [False, True])
def test_ragged_batch_rows_equal_the_batch_1_calls(lib, paged):
    spans = ((254, 4), (0, 1), (31, 2), (10, 5))
    c = make_case(32, spans, 4)
    o = run(lib, c, paged)
    assert torch.equal(run(lib, c, paged, max_ctx=258), o), "a host bound of the contexts changed bits"
    assert (o[3] == SENTINEL).all(), "the sequence with count > rows was written"
    for b, (hist, n) in enumerate(spans[:3]):
        ref, bound = reference(c.q_lat[b], c.cache[LAYER, b].astype(np.float64), hist, masks("chain", n))
        check("ragged sequence %d" % b, o[b, :n], ref, bound)
        assert (o[b, n:] == SENTINEL).all(), "rows past the count of sequence %d were written" % b
        assert torch.equal(run(lib, c, paged, only=b)[0], o[b]), "sequence %d differs from its batch-1 call" % b


def test_chain_append_absorb_verify_out_project(lib):
    """append_rows -> q_absorb (per-row lengths) -> verify -> out_project against the UN-absorbed float64 form; bounds as tests/test_mla_gpu.py"""
    heads, hist, rows = 16, 33, 3
    c = make_case(heads, ((hist, rows),), rows)
    rng, d = np.random.default_rng(7), lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    tab = lib.rope_table(c.S, 64, 64, 10000.0)
    kv_b = (rng.standard_normal((heads, 256, 512)) / np.sqrt(128)).astype(np.float16)
    q = rng.standard_normal((rows, heads, 192)).astype(np.float16)
    kv_a = (0.5 * rng.standard_normal((rows, 576))).astype(np.float16)
    gamma, cache, i32 = (1 + 0.1 * rng.uniform(-1, 1, 512)).astype(np.float16), d(c.cache), lambda *v: d(np.array(v, np.int32))
    lib.mla_kv_append_rows(d(kv_a), d(gamma), RMS_EPS, d(tab), cache, LAYER, i32(0, rows), i32(hist), rows, hist + rows)
    q_lat = torch.full((rows, heads, 576), SENTINEL, dtype=torch.float16, device=DEV)
    lib.mla_q_absorb(d(q), d(kv_b), d(tab), q_lat, i32(*range(hist + 1, hist + rows + 1)), c.S)
    o = run(lib, c, False, q_lat=q_lat.view(1, rows, heads, 576), cache=cache)
    out = lib.mla_out_project(o.view(rows, heads, 512), d(kv_b), torch.empty((rows, heads * 128), dtype=torch.float16, device=DEV))
    torch.cuda.synchronize()
    stored, W, q64 = cache[LAYER, 0].double().cpu().numpy(), kv_b.astype(np.float64), q.astype(np.float64)
    for i in range(rows):
        ctx, x0, x1 = hist + i + 1, q64[i, :, 128:160], q64[i, :, 160:]
        lat, pe, cs, sn = stored[:ctx, :512], stored[:ctx, 512:], tab[hist + i, :, 0], tab[hist + i, :, 1]
        q_rot = np.concatenate([x0 * cs - x1 * sn, x1 * cs + x0 * sn], -1)
        k_nope, v = np.einsum("tc,hnc->htn", lat, W[:, :128]), np.einsum("tc,hvc->htv", lat, W[:, 128:])
        logits = SCALE * (np.einsum("hn,htn->ht", q64[i, :, :128], k_nope) + q_rot @ pe.T)
        p = np.exp(logits - logits.max(-1, keepdims=True))
        ref_o, ref_out = p / p.sum(-1, keepdims=True) @ lat, np.einsum("ht,htv->hv", p / p.sum(-1, keepdims=True), v)
        check("chain o_lat row %d" % i, o[0, i], ref_o, EPS * np.abs(lat).max(0) + EPS * np.abs(ref_o))
        check("chain out row %d" % i, out[i].view(heads, 128), ref_out, EPS * np.abs(v).max(1) + EPS * np.abs(ref_out))
