"""llmie_kv_tree_commit against a numpy gather: caches of random bytes, dense and paged (a permuted block table with spare pages),
fp16 and e4m3 rows, head sizes 64 and 128, and every path shape -- the identity, [0, 63], a path whose destinations are later
sources ([0, 2, 3, 5]: slot 2 is both), a count of 0 -- with one move across a page boundary (base_len 126).  Every byte outside
the moved rows must stay as it was."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
L, KVH, N, MAX_SEQ = 2, 3, 64, 256
#           path                          base_len
CASES = [([0, 1, 2, 3],                   5),      # the identity: nothing moves
         ([0, 63],                        37),
         ([0, 2, 3, 5],                   126),    # slot 2 is a destination and a later source; sources 129, 131 -> slots 128, 129 cross the page
         ([0, 5, 9, 11],                  0),      # count 0 below: nothing moves
         ([0, 3, 1],                      190),    # not a walk's path (it descends): "all sources read, then all destinations written"
         ([0, 2, 6, 14, 30, 62],          64)]
COUNTS = [4, 2, 4, 0, 3, 6]


def _expect(cache, base, paths, counts):
    """cache: numpy uint8 [L, B, KVH, MAX_SEQ, row_bytes] (dense view)"""
    out = cache.copy()
    for b, (path, cnt) in enumerate(zip(paths, counts)):
        for m in range(cnt):
            out[:, b, :, base[b] + m] = cache[:, b, :, base[b] + path[m]]
    return out


@pytest.mark.parametrize("paged", [False, True], ids=["dense", "paged"])
@pytest.mark.parametrize("elem", [2, 1], ids=["f16", "e4m3"])
@pytest.mark.parametrize("hs", [64, 128])
def test_commit_equals_a_gather(llmie, paged, elem, hs):
    rng = np.random.default_rng(hs + elem + 7 * paged)
    B = len(CASES)
    row = hs * elem
    dense = [rng.integers(0, 256, (L, B, KVH, MAX_SEQ, row), dtype=np.uint8) for _ in range(2)]
    path = np.full((B, N), -1, np.int32)
    for b, (p, _) in enumerate(CASES):
        path[b, :len(p)] = p
    base = np.array([c[1] for c in CASES], np.int32)
    want = [_expect(d, base, [c[0] for c in CASES], COUNTS) for d in dense]
    assert any((w != d).any() for w, d in zip(want, dense))
    dt = torch.float16 if elem == 2 else torch.uint8
    as_dev = lambda a: torch.from_numpy(a).to(DEV).view(dt).reshape(a.shape[:-1] + (hs,))
    d_path, d_cnt, d_base = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (path, np.array(COUNTS, np.int32), base))
    if not paged:
        k, v = as_dev(dense[0]), as_dev(dense[1])
        llmie.kv_tree_commit(k, v, d_base, d_path, d_cnt)
        torch.cuda.synchronize()
        got = [t.contiguous().view(torch.uint8).reshape(L, B, KVH, MAX_SEQ, row).cpu().numpy() for t in (k, v)]
    else:
        mp = MAX_SEQ // 128
        num_pages = B * mp + 3
        table = rng.permutation(num_pages)[:B * mp].reshape(B, mp).astype(np.int32)
        pools, fill = [], []
        for d in dense:
            pool = rng.integers(0, 256, (L, num_pages, KVH, 128, row), dtype=np.uint8)
            fill.append(pool.copy())
            pool[:, table.flatten()] = d.reshape(L, B, KVH, mp, 128, row).transpose(0, 1, 3, 2, 4, 5).reshape(L, B * mp, KVH, 128, row)
            pools.append(pool)
        kp, vp = as_dev(pools[0]), as_dev(pools[1])
        llmie.kv_tree_commit(kp, vp, d_base, d_path, d_cnt, block_table=torch.from_numpy(table).to(DEV))
        torch.cuda.synchronize()
        got = []
        for t, f in zip((kp, vp), fill):
            pool = t.contiguous().view(torch.uint8).reshape(L, num_pages, KVH, 128, row).cpu().numpy()
            got.append(pool[:, table.flatten()].reshape(L, B, mp, KVH, 128, row).transpose(0, 1, 3, 2, 4, 5).reshape(L, B, KVH, MAX_SEQ, row))
            spare = np.setdiff1d(np.arange(num_pages), table.flatten())
            assert np.array_equal(pool[:, spare], f[:, spare]), "pages outside the block table changed"
    for name, g, w in (("K", got[0], want[0]), ("V", got[1], want[1])):
        if not np.array_equal(g, w):
            l, b, h, t, _ = np.argwhere(g != w)[0]
            raise AssertionError("%s cache differs first at layer %d sequence %d kv_head %d slot %d (base %d, path %s, count %d)" % (
                name, l, b, h, t, base[b], CASES[b][0], COUNTS[b]))


def test_rows_outside_the_cache_are_skipped(llmie):
    """a path entry whose source or destination lies past the slab (or is no node) moves nothing and touches nothing"""
    rng = np.random.default_rng(3)
    dense = [rng.integers(0, 256, (L, 2, KVH, 128, 128), dtype=np.uint8) for _ in range(2)]
    k, v = (torch.from_numpy(d).to(DEV) for d in dense)
    path = torch.tensor([[0, 5, 64, -1, -1, -1, -1, -1], [0, 3, 2, 1, -1, -1, -1, -1]], dtype=torch.int32, device=DEV)   # 64 is no node of n = 8
    llmie.kv_tree_commit(k, v, torch.tensor([10, 126], dtype=torch.int32, device=DEV), path, torch.tensor([4, 4], dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    want = [d.copy() for d in dense]
    for w, d in zip(want, dense):
        w[:, 0, :, 11] = d[:, 0, :, 15]
        # sequence 1: m = 1 reads slot 129 (outside: skipped), m = 2 is the identity, m = 3 writes slot 129 (outside: skipped)
    assert np.array_equal(k.cpu().numpy(), want[0]) and np.array_equal(v.cpu().numpy(), want[1])
