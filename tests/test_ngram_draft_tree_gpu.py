"""llmie_ngram_draft_tree against a numpy restatement of its rule (include/llmie.h): the candidates per suffix length, the first
`branches` distinct starts, the trie merge in that order with the node budget; the branches = 1 identity with llmie_ngram_draft;
the budget cut-off; prefix sharing between candidates; finished and short rows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV, PAD = "cuda", -5


def _reference(tokens, length, finished, n, k, branches, max_n, min_n):
    B, stride = tokens.shape
    ids, parent, count = np.full((B, n), PAD, np.int32), np.full((B, n), -1, np.int32), np.ones(B, np.int32)
    for b in range(B):
        t, L = tokens[b], min(max(int(length[b]), 0), stride)
        ids[b, 0] = t[L - 1] if L > 0 else PAD
        if (finished is not None and finished[b]) or L < min_n + 1:
            continue
        starts = []
        for m in range(min(max_n, L - 1), min_n - 1, -1):
            ends = [p + m for p in range(0, L - m) if np.array_equal(t[p:p + m], t[L - m:L])]   # p <= L - m - 1
            if not ends:
                continue
            full = [e for e in ends if e + k <= L]
            e = max(full) if full else max(ends)
            if e not in starts and len(starts) < branches:
                starts.append(e)
        cnt = 1
        for e in starts:
            cur = 0
            for tok in t[e:e + min(k, L - e)]:
                kids = [c for c in range(cur + 1, cnt) if parent[b, c] == cur and ids[b, c] == tok]
                if kids:
                    cur = kids[0]
                    continue
                if cnt >= n:
                    break
                ids[b, cnt], parent[b, cnt] = tok, cur
                cur = cnt
                cnt += 1
        count[b] = cnt
    return ids, parent, count


def _rows(rng, B, stride, vocab):
    """rows with many repeated n-grams: a small vocabulary, and copies of earlier spans pasted in"""
    tokens = rng.integers(0, vocab, (B, stride)).astype(np.int32)
    for b in range(B):
        for _ in range(6):
            a, ln = rng.integers(0, stride - 12), rng.integers(3, 12)
            d = rng.integers(0, stride - ln)
            tokens[b, d:d + ln] = tokens[b, a:a + ln].copy()
    return tokens


def _run(llmie, tokens, length, n, k, branches, max_n=3, min_n=1, finished=None):
    fin = None if finished is None else torch.tensor(finished, dtype=torch.uint8, device=DEV)
    out = llmie.ngram_draft_tree(torch.from_numpy(tokens).to(DEV), torch.tensor(length, dtype=torch.int32, device=DEV), n, k, branches=branches,
                                 max_n=max_n, min_n=min_n, pad_id=PAD, finished=fin)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("n,k,branches,max_n,min_n", [(16, 4, 4, 3, 1), (64, 15, 8, 8, 1), (5, 4, 3, 4, 2), (1, 3, 2, 3, 1), (33, 7, 2, 5, 1)])
def test_drafter_equals_the_rule(llmie, n, k, branches, max_n, min_n):
    rng = np.random.default_rng(n + k)
    B, stride = 9, 203   # (an odd stride: rows 1, 2, ... are not 16-byte aligned)
    tokens = _rows(rng, B, stride, 6)
    length = [stride, 150, 2, 1, 0, 77, stride + 9, 40, 119]
    finished = [0, 0, 0, 0, 0, 1, 0, 0, 0]
    got = _run(llmie, tokens, length, n, k, branches, max_n, min_n, finished)
    want = _reference(tokens, length, finished, n, k, branches, max_n, min_n)
    for name, g, w in zip(("ids", "parent", "node_count"), got, want):
        assert np.array_equal(g, w), (name, g, w)
    assert got[2][5] == 1 and got[2][4] == 1 and got[0][4, 0] == PAD
    assert all(got[1][b, j] < j for b in range(B) for j in range(1, got[2][b]))
    if n == 16:
        assert got[2].max() > k + 1, "no row with two branches"


def test_one_branch_is_the_linear_drafter(llmie):
    rng = np.random.default_rng(4)
    B, stride, k = 8, 160, 5
    tokens = _rows(rng, B, stride, 5)
    length = [stride, 100, 3, 1, 64, 33, 159, 12]
    for max_n, min_n in ((3, 1), (8, 2)):
        ids, parent, count = _run(llmie, tokens, length, k + 1, k, 1, max_n, min_n)
        l_ids, l_drafts, l_len = (o.cpu().numpy() for o in llmie.ngram_draft(torch.from_numpy(tokens).to(DEV), torch.tensor(length, dtype=torch.int32, device=DEV),
                                                                            k, max_n=max_n, min_n=min_n, pad_id=PAD))
        assert np.array_equal(ids, l_ids) and np.array_equal(count - 1, l_len)
        for b in range(B):
            assert parent[b].tolist() == [-1] + list(range(count[b] - 1)) + [-1] * (k + 1 - count[b])
        assert l_len.max() == k and l_len.min() == 0


def test_prefix_sharing_and_budget(llmie):
    # suffix "1 2 3": the 3-gram match continues 7 8 9, the later 2-gram match ("2 3") continues 7 8 5, the 1-gram match ("3") 6 6 6
    row = [1, 2, 3, 7, 8, 9, 0, 2, 3, 7, 8, 5, 0, 0, 3, 6, 6, 6, 0, 1, 2, 3]
    tokens = np.array([row], np.int32)
    ids, parent, count = _run(llmie, tokens, [len(row)], 16, 3, 4)
    assert count[0] == 8 and ids[0, :8].tolist() == [3, 7, 8, 9, 5, 6, 6, 6] and parent[0, :8].tolist() == [-1, 0, 1, 2, 2, 0, 5, 6]
    assert (ids[0, 8:] == PAD).all() and (parent[0, 8:] == -1).all()
    # the budget ends inside the second candidate, the third is cut at its first token
    ids, parent, count = _run(llmie, tokens, [len(row)], 5, 3, 4)
    assert count[0] == 5 and ids[0].tolist() == [3, 7, 8, 9, 5] and parent[0].tolist() == [-1, 0, 1, 2, 2]
    ids, parent, count = _run(llmie, tokens, [len(row)], 16, 3, 2)
    assert count[0] == 5   # two branches only
    assert np.array_equal(np.stack([ids[0], parent[0]]), np.stack(_reference(tokens, [len(row)], None, 16, 3, 2, 3, 1)[:2])[:, 0])
