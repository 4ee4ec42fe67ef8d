"""MLA sparse decode on the GPU: the indexer's logits and top-k selection, and the gathered attention, each against float64.
Indexer: ref_t = sum_h w_h relu(q_h . k_t) from the fp16 inputs.  Bound, derived: fp16 products are exact in fp32; ~140 fp32 roundings
per logit (128-term dot, weight, 8 summation levels) are 2^-16.8 to first order, 2^-15 leaves ~3.5x for the MFMA's internal summation:
|logit - ref_t| <= B_t = 2^-15 sum_h |w_h| sum_d |q_hd k_td|.  A selection is right when every selected position has ref >= kth_ref -
B_t - B_max and every other one ref <= kth_ref + B_t + B_max; so that the band hides nothing, at most max(8, top_k / 64) positions may
lie inside it (N(0, 1) q and k, w ~ N(0, 1) / 8: logits of standard deviation 5.5-8; on the CPU at most 5 fell inside at top_k 40-256
and 14 at 2048, over three seeds).  Attention: float64 over the selected rows as stored, the bound of tests/test_mla_gpu.py,
|err| <= 2^-10 max_j |row_j| + 2^-10 |ref|; rows outside the selection hold 1e4.
Measured on an MI355X, worst error / bound: logits < 1e-3; 1-3 positions in the band at top_k 40-256, 9-16 at 2048; attention 0.22."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV, L, LAYER, SCALE, EPS, SENTINEL = "cuda:0", 2, 1, 1.0 / 6.0, 2.0 ** -10, 777.0
PAGED = pytest.mark.parametrize("use_pages", [False, True], ids=["dense", "paged"])
d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
i32 = lambda a: d(np.asarray(a, np.int32))


@pytest.fixture(scope="module")
def lib(llmie):
    llmie.build()
    return llmie


def paged(dense):
    """(pool, block table) of a dense [L, B, S, row] cache: shuffled pages, two spare ones, 1e4 wherever no row lives"""
    B, mp, row = dense.shape[1], dense.shape[2] // 128, dense.shape[3]
    table = torch.randperm(B * mp + 2, generator=torch.Generator().manual_seed(B + mp))[:B * mp].reshape(B, mp).to(DEV)
    pool = torch.full((L, B * mp + 2, 128, row), 1e4, dtype=torch.float16, device=DEV)
    pool[:, table.flatten()] = dense.reshape(L, B * mp, 128, row)
    return pool, table.int().contiguous()


@functools.lru_cache(maxsize=None)
def index_case(ctxs, S):
    """(q, w, k cache [L, B, S, 128], ref [B, S], bound [B, S]): fp16 / fp32 values, float64 reference of layer LAYER"""
    rng, B = np.random.default_rng(sum(ctxs) + S), len(ctxs)
    q, k = rng.standard_normal((B, 64, 128)).astype(np.float16), rng.standard_normal((L, B, S, 128)).astype(np.float16)
    w = (rng.standard_normal((B, 64)) / 8).astype(np.float32)
    q64, k64, w64 = q.astype(np.float64), k[LAYER].astype(np.float64), w.astype(np.float64)
    ref = np.einsum("bth,bh->bt", np.maximum(np.einsum("btd,bhd->bth", k64, q64), 0), w64)
    return q, w, k, ref, 2.0 ** -15 * np.einsum("bth,bh->bt", np.einsum("btd,bhd->bth", np.abs(k64), np.abs(q64)), np.abs(w64))


def run_index(lib, q, w, k, ctxs, top_k, use_pages, max_ctx=0):
    """(sel [B, top_k], count [B], logits_out [B, span]) as numpy; all three start as sentinels"""
    B, S = k.shape[1], k.shape[2]
    cache, kw = d(k), {}
    if use_pages:
        pool, table = paged(cache)
        cache, kw = pool.view(L, -1, 128), dict(block_table=table, max_seq_len=S)
    sel, cnt = torch.full((B, top_k), -7, dtype=torch.int32, device=DEV), torch.full((B,), -7, dtype=torch.int32, device=DEV)
    out = torch.full((B, max_ctx or S), SENTINEL, dtype=torch.float32, device=DEV)
    lib.mla_index_topk(d(q), d(w), cache, LAYER, i32(ctxs), sel, cnt, lib.mla_index_workspace(B, S), out, max_ctx=max_ctx, **kw)
    torch.cuda.synchronize()
    return sel.cpu().numpy(), cnt.cpu().numpy(), out.double().cpu().numpy()


@PAGED
@pytest.mark.parametrize("ctx,top_k", [(257, 64), (700, 40), (700, 256), (3000, 2048)])
def test_logits_and_selection(lib, ctx, top_k, use_pages):
    ctxs, S = (ctx, ctx - 100), -(-ctx // 128) * 128
    q, w, k, ref, bound = index_case(ctxs, S)
    sel, cnt, got = run_index(lib, q, w, k, ctxs, top_k, use_pages)
    for b, n in enumerate(ctxs):
        ratio = (np.abs(got[b, :n] - ref[b, :n]) / bound[b, :n]).max()
        assert ratio <= 1.0 and (got[b, n:] == SENTINEL).all()
        assert cnt[b] == top_k and (np.diff(sel[b]) > 0).all() and sel[b, 0] >= 0 and sel[b, -1] < n
        kth, band = np.sort(ref[b, :n])[-top_k], bound[b, :n] + bound[b, :n].max()
        chosen = np.zeros(n, bool)
        chosen[sel[b]] = True
        inside = int((np.abs(ref[b, :n] - kth) <= band).sum())
        print("ctx %d top_k %d: logits worst error / bound %.2e, %d positions inside the band" % (n, top_k, ratio, inside))
        assert (ref[b, :n][chosen] >= kth - band[chosen]).all() and (ref[b, :n][~chosen] <= kth + band[~chosen]).all()
        assert inside <= max(8, top_k // 64)


@pytest.mark.parametrize("kind", ["equal_rows", "all_negative"])
def test_ties_go_to_the_lower_positions(lib, kind):
    q, w, k, _, _ = index_case((700, 600), 768)
    # equal key rows give equal logit bits; with every dot negative every logit is 0
    q, k = (q, np.broadcast_to(k[:, :, :1], k.shape)) if kind == "equal_rows" else (np.abs(q), -np.abs(k))
    sel, cnt, _ = run_index(lib, q, w, k, (700, 600), 40, False)
    assert (sel == np.arange(40)).all() and (cnt == 40).all()


def test_identity_dead_sequences_and_batch_rows(lib):
    """ctx <= top_k selects everything; a dead sequence (0, or above max_ctx) keeps its row and counts 0; a row equals its batch-1 call"""
    ctxs = (300, 0, 50, 64, 290, 301)
    q, w, k, _, _ = index_case(ctxs, 384)
    sel, cnt, _ = run_index(lib, q, w, k, ctxs, 64, True, max_ctx=300)
    assert cnt.tolist() == [64, 0, 50, 64, 64, 0] and (sel[[1, 5]] == -7).all()
    assert (sel[2] == np.where(np.arange(64) < 50, np.arange(64), -1)).all() and (sel[3] == np.arange(64)).all()
    for b in (0, 4):
        alone = run_index(lib, q[b:b + 1], w[b:b + 1], k[:, b:b + 1], ctxs[b:b + 1], 64, False)
        assert (alone[0][0] == sel[b]).all() and alone[1][0] == 64


@functools.lru_cache(maxsize=None)
def attend_case(heads, B=2, S=768):
    """(q_lat, latent cache [L, B, S, 576]): logits of standard deviation 2"""
    rng = np.random.default_rng(heads + B)
    return rng.standard_normal((B, heads, 576)).astype(np.float16), (0.5 * rng.standard_normal((L, B, S, 576))).astype(np.float16)


def attend_check(what, o_lat, q_lat, rows):
    """o_lat [heads, 512] of one sequence against float64 attention over its gathered rows [n, 576]"""
    q, rows = q_lat.astype(np.float64), rows.astype(np.float64)
    s = SCALE * q @ rows.T
    p = np.exp(s - s.max(-1, keepdims=True))
    o = (p / p.sum(-1, keepdims=True)) @ rows[:, :512]
    ratio = (np.abs(o_lat.double().cpu().numpy() - o) / (EPS * np.abs(rows[:, :512]).max(0) + EPS * np.abs(o))).max()
    print("%s: worst error / bound %.3f" % (what, ratio))
    assert ratio <= 1.0, what


def run_sparse(lib, q_lat, cache, ctxs, sel, counts, use_pages, keep=()):
    """(o_lat [B, heads, 512], the device cache, its paging arguments); rows of LAYER outside the selection of every sequence not in
    `keep` are overwritten with 1e4"""
    B, S = cache.shape[1], cache.shape[2]
    cache = cache.copy()
    for b in set(range(B)) - set(keep):
        live = np.zeros(S, bool)
        live[np.clip(sel[b, :counts[b]], 0, max(ctxs[b] - 1, 0))] = True
        cache[LAYER, b, ~live] = 1e4
    dev_cache, kw = d(cache), {}
    if use_pages:
        dev_cache, table = paged(dev_cache)
        kw = dict(block_table=table, max_seq_len=S)
    o_lat = torch.full((B, q_lat.shape[1], 512), SENTINEL, dtype=torch.float16, device=DEV)
    lib.mla_decode_sparse(d(q_lat), dev_cache, LAYER, i32(ctxs), i32(sel), i32(counts), SCALE, o_lat,
                          lib.mla_workspace(B, q_lat.shape[1], sel.shape[1]), **kw)
    torch.cuda.synchronize()
    return o_lat, dev_cache, kw


def subsets(seed, B, ctx, count, top_k=320):
    """[B, top_k]: `count` sorted random positions below ctx per sequence, -1 behind them"""
    rng = np.random.default_rng(seed)
    return np.stack([np.concatenate([np.sort(rng.choice(ctx, count, replace=False)), np.full(top_k - count, -1)]) for _ in range(B)])


@PAGED
@pytest.mark.parametrize("heads", [16, 32])
@pytest.mark.parametrize("count", [1, 31, 32, 33, 256, 257, 300])
def test_random_sorted_subsets(lib, count, heads, use_pages):
    q_lat, cache = attend_case(heads)
    sel = subsets(count, 2, 700, count)
    o_lat = run_sparse(lib, q_lat, cache, (700, 700), sel, (count, count), use_pages)[0]
    for b in range(2):
        attend_check("count %d heads %d sequence %d" % (count, heads, b), o_lat[b], q_lat[b], cache[LAYER, b, sel[b, :count]])


@PAGED
@pytest.mark.parametrize("ctx", [33, 257, 547])
def test_the_whole_context_gives_the_bits_of_mla_decode(lib, ctx, use_pages):
    q_lat, cache = attend_case(16)
    sel = np.tile(np.where(np.arange(640) < ctx, np.arange(640), -1), (2, 1))
    sparse, dev_cache, kw = run_sparse(lib, q_lat, cache, (ctx, ctx), sel, (ctx, ctx), use_pages, keep=(0, 1))
    dense = lib.mla_decode(d(q_lat), dev_cache, LAYER, i32((ctx, ctx)), SCALE, torch.full_like(sparse, SENTINEL), lib.mla_workspace(2, 16, 768), **kw)
    assert torch.equal(sparse, dense)


def test_ragged_batch_dead_rows_and_bad_entries(lib):
    """counts (300, 0, 33, 280, 40, 290): row 1 (count 0), row 3 (a dead context: 0) and row 5 (a dead context: past max_seq_len = 768)
    stay untouched, the dead ones under counts that reach the second split, so the merge runs for them; row 4 holds -1 and ctx + 5
    inside its count and attends the clamped rows; the live rows have the bits of their batch-1 calls"""
    q_lat, cache = attend_case(16, B=6)
    ctxs, counts, sel = (700, 650, 40, 0, 500, 800), (300, 0, 33, 280, 40, 290), subsets(5, 6, 700, 300)
    sel[2, :33], sel[4, :40] = subsets(6, 1, 40, 33, 33)[0], subsets(7, 1, 500, 40, 40)[0]
    sel[4, 0], sel[4, 39] = -1, 505
    o_lat = run_sparse(lib, q_lat, cache, ctxs, sel, counts, True, keep=(1, 3, 5))[0]
    assert (o_lat[1] == SENTINEL).all() and (o_lat[3] == SENTINEL).all() and (o_lat[5] == SENTINEL).all()
    for b in (0, 2, 4):
        alone = run_sparse(lib, q_lat[b:b + 1], cache[:, b:b + 1], ctxs[b:b + 1], sel[b:b + 1], counts[b:b + 1], False)[0]
        assert torch.equal(alone[0], o_lat[b])
        attend_check("ragged row %d" % b, o_lat[b], q_lat[b], cache[LAYER, b, np.clip(sel[b, :counts[b]], 0, ctxs[b] - 1)])
