"""llmie_ngram_draft against a restatement of the header's rule in a dozen lines of Python: strides 16 and 4099, odd strides (rows
that are not 16-byte aligned), every length at which the rule changes, periodic streams, the second tier of the rule, the longer n
beating a more recent shorter n, no match, finished rows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV, PAD = "cuda", -5


def rule(t, L, k, max_n, min_n, finished):
    """-> (ids [k + 1], drafts [k], m) of one row, word for word from include/llmie.h"""
    ids, drafts = [PAD] * (k + 1), [PAD] * k
    ids[0] = int(t[L - 1]) if L > 0 else PAD
    if finished or L < min_n + 1:
        return ids, drafts, 0
    for n in range(min(max_n, L - 1), min_n - 1, -1):
        starts = np.lib.stride_tricks.sliding_window_view(t[:L - 1], n)          # p = 0 .. L - n - 1
        match = np.nonzero((starts == t[L - n:L]).all(axis=1))[0]
        if match.size == 0:
            continue
        full = match[match + n + k <= L]
        p = int(full.max() if full.size else match.max())
        m = min(k, L - p - n)
        drafts[:m] = [int(x) for x in t[p + n:p + n + m]]
        ids[1:1 + m] = drafts[:m]
        return ids, drafts, m
    return ids, drafts, 0


def check(llmie, tokens, lens, k, max_n, min_n, finished=None):
    tokens = np.ascontiguousarray(tokens, dtype=np.int32)
    B, stride = tokens.shape
    fin = None if finished is None else torch.tensor(finished, dtype=torch.uint8, device=DEV)
    ids, drafts, dlen = llmie.ngram_draft(torch.from_numpy(tokens).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), k, max_n=max_n,
                                          min_n=min_n, pad_id=PAD, finished=fin)
    torch.cuda.synchronize()
    want = [rule(tokens[b], min(max(int(lens[b]), 0), stride), k, max_n, min_n, bool(finished[b]) if finished is not None else False)
            for b in range(B)]
    assert dlen.tolist() == [w[2] for w in want]
    assert drafts.tolist() == [w[1] for w in want]
    assert ids.tolist() == [w[0] for w in want]
    return dlen.tolist()


GRID = [(k, max_n, min_n) for k in (1, 4, 15) for max_n, min_n in ((3, 1), (8, 2))]


@pytest.mark.parametrize("stride", [16, 4099, 17, 4098])   # 17, 4099: odd strides leave most rows off 16-byte alignment
@pytest.mark.parametrize("k,max_n,min_n", GRID)
def test_lengths_and_periodic_streams(llmie, stride, k, max_n, min_n):
    rng = np.random.default_rng(stride * 100 + k * 10 + max_n)
    rows, lens, fin = [], [], []
    for period in (3, k + 2, 2 * k + 3):                       # shorter and longer than k
        base = rng.integers(10, 10 + 4 * period, period)
        for L in (0, 1, min_n, min_n + 1, stride // 2 + 1, stride, stride + 7, -2):   # (the last two are clamped)
            rows.append(np.resize(base, stride))
            lens.append(L)
            fin.append(0)
    rows.append(np.resize(rng.integers(10, 20, 5), stride))    # a finished row that would match
    lens.append(stride)
    fin.append(1)
    rows.append(rng.integers(0, 4, stride))                    # a tiny alphabet: matches of every n all over the row
    lens.append(stride)
    fin.append(0)
    got = check(llmie, np.stack(rows), lens, k, max_n, min_n, fin)
    assert 0 in got and max(got) >= 1 and (stride < 100 or k in got)
    check(llmie, np.stack(rows), lens, k, max_n, min_n, None)  # finished == NULL


@pytest.mark.parametrize("k,max_n,min_n", GRID)
def test_the_rules_tiers(llmie, k, max_n, min_n):
    stride = 4099
    rng = np.random.default_rng(k * 10 + max_n)
    uniq = lambda n, lo: np.arange(lo, lo + n)                 # tokens that occur nowhere else
    n = max_n
    S = uniq(n, 100000)
    rows, lens = [], []
    # 0: no match at all
    r = uniq(stride, 0)
    rows.append(r); lens.append(stride)
    # 1: the only match sits so late that fewer than k tokens follow it: the second tier
    tail = uniq(2 if k > n + 2 else 0, 300000)
    second = k > n + len(tail)                                 # (k <= n: whatever follows a match of n tokens is a full continuation)
    r = np.concatenate([uniq(3000, 0), S, tail, S])
    rows.append(np.resize(np.concatenate([r, uniq(stride, 500000)]), stride)); lens.append(len(r))
    # 2: an early match with a full continuation AND a late one without: the first tier takes the early one
    r = np.concatenate([uniq(50, 0), S, uniq(k + 3, 200000), uniq(2000, 1000), S, tail, S])
    rows.append(np.resize(np.concatenate([r, uniq(stride, 500000)]), stride)); lens.append(len(r))
    # 3: a match of the full n far back must beat a more recent match of only min_n tokens
    short = S[-min_n:]
    r = np.concatenate([uniq(40, 0), S, uniq(k + 1, 200000), uniq(3000, 1000), [77777], short, uniq(k + 1, 300000), S])
    rows.append(np.resize(np.concatenate([r, uniq(stride, 500000)]), stride)); lens.append(len(r))
    # 4: only the short suffix matches (the token in front of it differs): n falls back to min_n
    r = np.concatenate([uniq(1000, 0), [77777], short, uniq(k + 1, 300000), uniq(500, 2000), S])
    rows.append(np.resize(np.concatenate([r, uniq(stride, 500000)]), stride)); lens.append(len(r))
    got = check(llmie, np.stack(rows), lens, k, max_n, min_n)
    assert got == [0, n + len(tail) if second else k, k, k, k], got
    # what row 3 drafted is what followed the LONG match
    tokens = np.stack(rows)
    ids, drafts, _ = llmie.ngram_draft(torch.from_numpy(tokens.astype(np.int32)).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), k,
                                       max_n=max_n, min_n=min_n, pad_id=PAD)
    assert drafts[3].tolist() == list(range(200000, 200000 + k)) and ids[3, 0].item() == int(S[-1])
    assert drafts[4].tolist() == list(range(300000, 300000 + k))
    if second:   # row 2 took the early match, which has k tokens behind it, not the late one
        assert drafts[2].tolist() == list(range(200000, 200000 + k))


def test_determinism(llmie):
    rng = np.random.default_rng(5)
    tokens = torch.from_numpy(rng.integers(0, 3, (6, 4099)).astype(np.int32)).to(DEV)
    lens = torch.tensor([4099, 4000, 17, 3, 2048, 4098], dtype=torch.int32, device=DEV)
    a = llmie.ngram_draft(tokens, lens, 7, max_n=8, min_n=1)
    b = llmie.ngram_draft(tokens, lens, 7, max_n=8, min_n=1)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
