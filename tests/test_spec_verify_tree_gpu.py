"""llmie_spec_verify_tree and llmie_spec_tree_prepare against their definitions.

1. The pinned equivalence: with parent[i] = i - 1, n = k + 1, node_ids[b, i] = draft_ids[b, i - 1] and node_count = draft_len + 1,
   every output and every state array equals llmie_spec_verify's bit for bit -- over the parameter mixes, shapes and extension
   cases of tests/test_spec_verify_gpu.py (whose helpers build the inputs), at V = 1000 and V = 7.
2. Real trees against a Python restatement of the walk that calls the existing sampler row by row with the history view and the
   Philox step of each node: two children with one token (the lowest index wins), a pick that matches only a dead node,
   node_count = 1, n = 64 at depth 63, histories that saturate inside a path, determinism and slot invariance.
3. llmie_spec_tree_prepare against tests/spec_tree_attn_cases.prepare_ref, bad parents and node counts included.
"""
import numpy as np
import pytest
import torch

import spec_tree_attn_cases as tc
import test_spec_verify_gpu as lin
from test_spec_verify_gpu import END, STRIDE, Ext, State, _logits, _params, _same

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _i32(a):
    return torch.tensor(np.asarray(a), dtype=torch.int32, device=DEV)


def _chain_tree(llmie, B, n, draft_len):
    parent = _i32(np.tile(np.arange(-1, n - 1), (B, 1)))
    count = None if draft_len is None else _i32(np.asarray(draft_len) + 1)
    depth, anc = llmie.spec_tree_prepare(parent, count)
    return parent, depth, anc


def _both(llmie, logits, params, st0, drafts, append=True, draft_len=None, ext=None, shared_step=None, step_dev=False, end_id=END):
    """llmie_spec_verify and llmie_spec_verify_tree (chain tree) on clones of st0: everything must be bit-equal -> the count"""
    B, n, V = logits.shape
    k = n - 1
    outs = []
    for tree in (False, True):
        got = st0.clone()
        vext = None if ext is None else ext.for_verify(llmie)
        lp = torch.zeros((B, n), dtype=torch.float32, device=DEV)
        state = llmie.SpecState(got.last, got.cached, None if shared_step is not None else got.steps)
        sdev = torch.tensor([shared_step], dtype=torch.int32, device=DEV) if step_dev else None
        kw = dict(state=state, history=got.hist, history_len=got.hlen, append=append, out_logprob=lp,
                  step=-77 if step_dev else (shared_step or 0), step_dev=sdev, ext=vext)
        prm = llmie.sampling_params(params)
        path = None
        if tree:
            ids = torch.cat([torch.full((B, 1), -12345, dtype=torch.int32, device=DEV), drafts], dim=1).contiguous()   # slot 0 is not read
            parent, depth, anc = _chain_tree(llmie, B, n, draft_len)
            tok, cnt, path = llmie.spec_verify_tree(logits.reshape(B * n, V), ids, parent, depth, anc, prm, got.seq, got.fin, end_id, **kw)
        else:
            d_len = None if draft_len is None else _i32(draft_len)
            tok, cnt = llmie.spec_verify(logits.reshape(B * n, V), drafts, prm, got.seq, got.fin, end_id, draft_len=d_len, **kw)
        torch.cuda.synchronize()
        outs.append(dict(tok=tok, cnt=cnt, lp=lp, top_ids=None if vext is None or not ext.top_n else vext.top_ids,
                         top_lp=None if vext is None or not ext.top_n else vext.top_logprobs, **got.fields()))
        if tree:   # the chain's path is 0, 1, ..., count - 1
            c = cnt.cpu().numpy()
            want = np.where(np.arange(n)[None, :] < c[:, None], np.arange(n)[None, :], -1)
            assert np.array_equal(path.cpu().numpy(), want), (path, c)
    for name in outs[0]:
        if outs[0][name] is not None:
            _same(name, outs[1][name], outs[0][name])
    return outs[0]["cnt"].cpu().numpy(), outs[0]["tok"].cpu().numpy()


def _drafts(llmie, logits, params, st0, append, corrupt, ext=None, step=None, end_id=END):
    """the chain of picks with one corrupted position per sequence (>= k: none), as tests/test_spec_verify_gpu.py builds them"""
    B, n, V = logits.shape
    prm = [llmie.sampling_params([p]) for p in params]
    chain, _, _ = lin._reference(llmie, logits, prm, st0.clone(), append, ext=ext, step=step, end_id=end_id)
    drafts = chain[:, :n - 1].copy()
    for b in range(B):
        if corrupt[b] < n - 1:
            drafts[b, corrupt[b]] = (drafts[b, corrupt[b]] + 1) % V
    return torch.from_numpy(drafts).to(DEV)


SHAPES = [(V, B, k) for V in (1000, 7) for B in (1, 5) for k in (1, 4, 15)]
MATRIX = [(V, B, k, lin.MIXES[i % 5]) for i, (V, B, k) in enumerate(SHAPES)] + [(V, 5, 4, m) for V in (1000, 7) for m in lin.MIXES]


@pytest.mark.parametrize("V,B,k,mix", MATRIX, ids=str)
def test_chain_equals_linear_verify(llmie, V, B, k, mix):
    case = MATRIX.index((V, B, k, mix))
    rng = np.random.default_rng(2000 + case)
    dtype = torch.float16 if case % 2 else torch.float32
    logits = _logits(rng, B, k, V, dtype)
    hlen = [STRIDE - 2, STRIDE, STRIDE - 1, STRIDE - k, 0][:B] if mix == "penal_edge" else None
    st0 = State(rng, B, V, hlen=hlen)
    corrupt = lin._corrupt(B, k, case)
    append = mix != "penal_keep"
    drafts = _drafts(llmie, logits, _params(mix, B), st0, append, corrupt)
    cnt, _ = _both(llmie, logits, _params(mix, B), st0, drafts, append=append)
    assert list(cnt) == [min(a, k) + 1 for a in corrupt], (cnt, corrupt)


@pytest.mark.parametrize("V", [1000, 7])
def test_chain_draft_len_and_shared_step(llmie, V):
    B, k = 5, 4
    rng = np.random.default_rng(51 + V)
    logits = _logits(rng, B, k, V, torch.float16)
    st0 = State(rng, B, V)
    drafts = _drafts(llmie, logits, _params("truncate", B), st0, True, [k] * B)
    cnt, _ = _both(llmie, logits, _params("truncate", B), st0, drafts, draft_len=[0, 1, k, -3, k + 9])
    assert list(cnt) == [1, 2, k + 1, 1, k + 1]
    for step_dev in (False, True):
        d = _drafts(llmie, logits, _params("truncate", B), st0, True, lin._corrupt(B, k, 0), step=41)
        cnt, _ = _both(llmie, logits, _params("truncate", B), st0, d, shared_step=41, step_dev=step_dev)
        assert list(cnt) == [1, 3, 5, 4, 2]


@pytest.mark.parametrize("V", [1000, 7])
def test_chain_stops_min_step_finished_masks_top_n(llmie, V):
    B, k = 3, 4
    rng = np.random.default_rng(61 + V)
    stop = 500 if V > 500 else 5
    # a stop id and end_id on an accepted node
    lg = _logits(rng, B, k, V, torch.float32, end_low=False)
    lg[0, 1, END], lg[1, 2, stop], lg[2, 3, stop] = 40.0, 40.0, 40.0
    lg[:, 0, END] = -30.0
    ext = Ext(B, k, V, stops=[[], [4, stop], [stop + 1]])
    st0 = State(rng, B, V)
    cnt, tok = _both(llmie, lg, _params("greedy", B), st0, _drafts(llmie, lg, _params("greedy", B), st0, True, [k] * B, ext=ext), ext=ext)
    if V == 1000:   # (at V = 7 a walk may meet a stop id by chance: the equivalence above is what is checked there)
        assert list(cnt) == [2, 3, k + 1] and tok[0, 1] == END and tok[1, 2] == stop
    # min_step inside the chunk
    lg = _logits(rng, 2, k, V, torch.float16)
    lg[:, :, END] = 40.0
    st0 = State(rng, 2, V, steps=[10, 20])
    ext = Ext(2, k, V, min_step=[12, 23])
    cnt, tok = _both(llmie, lg, _params("greedy", 2), st0, _drafts(llmie, lg, _params("greedy", 2), st0, True, [k, k], ext=ext), ext=ext)
    assert list(cnt) == [3, 4] and tok[0, 2] == END and tok[1, 3] == END
    # a finished sequence, top-N of every row
    B = 5
    lg = _logits(rng, B, k, V, torch.float16)
    st0 = State(rng, B, V)
    st0.fin[4] = 1
    ext = Ext(B, k, V, top_n=5)
    cnt, _ = _both(llmie, lg, _params("truncate", B), st0, _drafts(llmie, lg, _params("truncate", B), st0, True, [0, 1, k, 2, 0], ext=ext), ext=ext)
    assert list(cnt) == [1, 2, k + 1, 3, 0] or V == 7
    # one mask per row
    B = 2
    lg = _logits(rng, B, k, V, torch.float16)
    forced = rng.integers(3, V, B * (k + 1))
    masks = np.zeros((B * (k + 1) + 1, V), bool)
    masks[np.arange(B * (k + 1)), forced] = True
    masks[-1] = True
    index = list(rng.permutation(B * (k + 1)))
    index[3] = -1
    ext = Ext(B, k, V, masks=masks, mask_index=index)
    st0 = State(rng, B, V)
    cnt, tok = _both(llmie, lg, _params("truncate", B), st0, _drafts(llmie, lg, _params("truncate", B), st0, True, [k, 2], ext=ext), ext=ext)
    assert list(cnt) == [k + 1, 3] or V == 7


# ---------------------------------------------------------------------------------------------- real trees
class TreeRef:
    """the walk's definition on the existing sampler: pick(b, i) = sample_logits on row (b, i) alone, at step s_b + depth_i, on the
    stored history followed by the tokens of the path root -> i (as far as the appends reach)"""

    def __init__(self, llmie, logits, params, st, append, ext=None):
        self.llmie, self.logits, self.st, self.append, self.ext = llmie, logits, st, append, ext
        self.prm = [llmie.sampling_params([p]) for p in params]
        self.calls = 0

    def pick(self, b, i, ids, parent):
        """-> (token, logprob, finishes); ids / parent: python lists of sequence b (only the ancestors of i are read)"""
        path, j = [], i
        while j > 0:
            path.append(int(ids[j]))
            j = int(parent[j])
        path.reverse()
        st = self.st
        hist = st.hist[b:b + 1].clone()
        n = min(max(int(st.hlen[b]), 0), STRIDE)
        if self.append:
            for t in path:
                if n < STRIDE:
                    hist[0, n] = t
                    n += 1
        out, lp = torch.empty(1, dtype=torch.int32, device=DEV), torch.empty(1, dtype=torch.float32, device=DEV)
        fin, seq = torch.zeros(1, dtype=torch.uint8, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        self.llmie.sample_logits(self.logits[b, i:i + 1], self.prm[b], seq, fin, out, int(st.steps[b]) + len(path), END, history=hist,
                                 history_len=torch.tensor([n], dtype=torch.int32, device=DEV), append=False, out_logprob=lp,
                                 ext=None if self.ext is None else self.ext.for_row(self.llmie, b, i))
        self.calls += 1
        return int(out.item()), float(lp.item()), int(fin.item())

    def walk(self, ids, parent, count):
        """moves self.st as the entry must; -> tokens, count, path, logprob (numpy)"""
        st = self.st
        B, n = ids.shape
        tok, path = np.full((B, n), -1, np.int32), np.full((B, n), -1, np.int32)
        lp, cnt = np.full((B, n), -np.inf, np.float32), np.zeros(B, np.int32)
        for b in range(B):
            if int(st.fin[b]):
                continue
            _, anc = tc.prepare_ref(parent[b], None if count is None else count[b])
            cur, fin = 0, 0
            hl = int(st.hlen[b])
            while True:
                t, l, fin = self.pick(b, cur, ids[b], parent[b])
                tok[b, cnt[b]], lp[b, cnt[b]], path[b, cnt[b]] = t, l, cur
                cnt[b] += 1
                if self.append and 0 <= hl < STRIDE:
                    st.hist[b, hl] = t
                    hl += 1
                nxt = [j for j in range(cur + 1, n) if (anc[j] & 1) and parent[b][j] == cur and ids[b][j] == t]
                if fin or not nxt:
                    break
                cur = nxt[0]
            st.seq[b] += int(cnt[b])
            st.fin[b] = fin
            if self.append:
                st.hlen[b] = hl
            st.last[b] = int(tok[b, cnt[b] - 1])
            st.cached[b] += int(cnt[b])
            st.steps[b] += int(cnt[b])
        return tok, cnt, path, lp


def _grow(ref, b, parent, follow, V):
    """ids of sequence b for the tree `parent`: the children of node i named in follow[i] carry pick_i, every other child a wrong
    token.  Picks are taken in index order (a node's path is complete when it is reached)."""
    n = len(parent)
    ids = [-7] * n
    for i in range(n):
        kids = [j for j in range(i + 1, n) if parent[j] == i]
        if not kids:
            continue
        t = ref.pick(b, i, ids, parent)[0]
        for r, j in enumerate(kids):
            ids[j] = t if j in follow.get(i, ()) else (t + r + 1) % V
    return ids


def _run_tree(llmie, logits, params, st0, ids, parent, count, append=True, ext=None):
    B, n, V = logits.shape
    want = st0.clone()
    w_tok, w_cnt, w_path, w_lp = TreeRef(llmie, logits, params, want, append, ext).walk(np.asarray(ids), [list(p) for p in parent], count)
    got = st0.clone()
    d_parent = _i32(parent)
    depth, anc = llmie.spec_tree_prepare(d_parent, None if count is None else _i32(count))
    lp = torch.zeros((B, n), dtype=torch.float32, device=DEV)
    tok, cnt, path = llmie.spec_verify_tree(logits.reshape(B * n, V), _i32(ids), d_parent, depth, anc, llmie.sampling_params(params), got.seq,
                                            got.fin, END, state=llmie.SpecState(got.last, got.cached, got.steps), history=got.hist,
                                            history_len=got.hlen, append=append, out_logprob=lp,
                                            ext=None if ext is None else ext.for_verify(llmie))
    torch.cuda.synchronize()
    for name, g, w in (("tokens", tok, w_tok), ("count", cnt, w_cnt), ("path", path, w_path), ("out_logprob", lp, w_lp)):
        _same(name, g, w)
    for name in want.fields():
        _same(name, getattr(got, name), getattr(want, name))
    return dict(tok=tok, cnt=cnt, path=path, lp=lp, **got.fields())


@pytest.mark.parametrize("mix", ["greedy", "penal_append", "penal_keep"])
def test_trees_equal_the_walk_over_sampler_calls(llmie, mix):
    V, B, n = 1000, 5, 12
    rng = np.random.default_rng(70 + len(mix))
    logits = _logits(rng, B, n - 1, V, torch.float16)
    st0 = State(rng, B, V, hlen=[5, STRIDE - 2, 11, STRIDE, 9])   # sequences 1 and 3: the appends saturate inside the path
    params, append = _params(mix, B), mix != "penal_keep"
    ref = TreeRef(llmie, logits, params, st0.clone(), append)
    #            0   1  2  3  4  5  6  7  8  9 10 11
    parent = [[-1, 0, 0, 0, 2, 2, 4, 4, 6, 1, 9, 8],    # 0: the second child is right at every level: path 0 2 4 6 8 11
              [-1, 0, 0, 1, 2, 1, 2, 4, 7, 8, 9, 10],   # 1: nodes 1 and 2 BOTH carry the pick: the lowest index wins
              [-1, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5],    # 2: the right child of the root is dead (node_count): the walk stops
              [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10],   # 3: a chain, every draft right
              [-1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]]    # 4: node_count = 1: only the root's pick
    follow = [{0: (2,), 2: (4,), 4: (6,), 6: (8,), 8: (11,)}, {0: (1, 2), 1: (5,), 2: (6,)}, {}, {i: (i + 1,) for i in range(11)},
              {0: (3,)}]
    ids = [_grow(ref, b, parent[b], follow[b], V) for b in range(B)]
    count = [n, n, n, n, 1]
    # sequence 2: the only child that carries the pick is node 2 -- and it names a LATER parent, so it is dead, with its subtree
    t2 = ref.pick(2, 0, ids[2], parent[2])[0]
    ids[2][1], ids[2][2] = (t2 + 1) % V, t2
    parent[2][2] = 7
    out = _run_tree(llmie, logits, params, st0, ids, parent, count, append=append)
    assert out["cnt"].tolist() == [6, 3, 1, n, 1], out["cnt"]
    assert out["path"][0].tolist()[:6] == [0, 2, 4, 6, 8, 11] and out["path"][1].tolist()[:3] == [0, 1, 5]
    assert out["hlen"].tolist()[1] == (STRIDE if append else STRIDE - 2)


def test_n64_at_depth_63_and_a_wide_tree(llmie):
    V, B, n = 1000, 2, 64
    rng = np.random.default_rng(81)
    logits = _logits(rng, B, n - 1, V, torch.float32)
    st0 = State(rng, B, V)
    params = _params("truncate", B)
    ref = TreeRef(llmie, logits, params, st0.clone(), True)
    chain = list(range(-1, n - 1))
    heap = [-1] + [(i - 1) // 2 for i in range(1, n)]
    ids = [_grow(ref, 0, chain, {i: (i + 1,) for i in range(n - 1)}, V),
           _grow(ref, 1, heap, {i: (2 * i + 2,) for i in range(n)}, V)]    # the right child all the way: 0 2 6 14 30 62
    ext = Ext(B, n - 1, V, top_n=3)
    out = _run_tree(llmie, logits, params, st0, ids, [chain, heap], None, ext=ext)
    assert out["cnt"].tolist() == [64, 6] and out["path"][1].tolist()[:6] == [0, 2, 6, 14, 30, 62] and out["path"][0].tolist() == list(range(64))


def test_tree_determinism_and_slot_invariance(llmie):
    V, B, n = 1000, 4, 9
    rng = np.random.default_rng(91)
    logits = _logits(rng, B, n - 1, V, torch.float16)
    params = _params("penal_append", B)
    st0 = State(rng, B, V)
    ref = TreeRef(llmie, logits, params, st0.clone(), True)
    parent = [[-1, 0, 0, 1, 1, 2, 2, 5, 5]] * B
    follow = [{0: (2,), 2: (5,), 5: (8,)}, {0: (1,), 1: (4,)}, {}, {0: (2,), 2: (6,)}]
    ids = [_grow(ref, b, parent[b], follow[b], V) for b in range(B)]
    a = _run_tree(llmie, logits, params, st0, ids, parent, None)
    b = _run_tree(llmie, logits, params, st0, ids, parent, None)
    for name in a:
        _same(name, a[name], b[name])
    assert a["cnt"].tolist() == [4, 3, 1, 3]
    # every sequence alone in slot 0 against its slot in the batch
    for s in range(B):
        one = State(rng, 1, V)
        for name in one.fields():
            setattr(one, name, getattr(st0, name)[s:s + 1].clone())
        solo = _run_tree(llmie, logits[s:s + 1].contiguous(), [params[s]], one, [ids[s]], [parent[s]], None)
        for name in solo:
            _same("%s of sequence %d" % (name, s), solo[name], a[name][s:s + 1])


def test_prepare_against_numpy(llmie):
    rng = np.random.default_rng(5)
    for n in (1, 2, 17, 33, 64):
        B = 7
        parent = np.zeros((B, n), np.int32)
        for b in range(B):
            for i in range(n):
                parent[b, i] = rng.integers(0, i) if i else -1
        if n > 4:   # bad parents: negative, itself, a later node, far out of range
            parent[1, 3], parent[2, 2], parent[3, n // 2], parent[4, n - 1] = -1, 2, n - 1, 1 << 30
        parent[5, 0] = 5   # node 0's parent is not read
        count = np.array([n, n, n, n, n, max(1, n // 2), -3][:B], np.int32)
        for cnt in (None, count):
            depth, anc = llmie.spec_tree_prepare(_i32(parent), None if cnt is None else _i32(cnt))
            torch.cuda.synchronize()
            for b in range(B):
                d, a = tc.prepare_ref(parent[b], None if cnt is None else cnt[b])
                assert depth[b].tolist() == d, (n, b)
                assert np.array_equal(anc[b].cpu().numpy(), tc.anc_i64(a)), (n, b)
    for name, (parent, count) in tc.TREES.items():
        depth, anc = llmie.spec_tree_prepare(_i32([parent]), None if count is None else _i32([count]))
        d, a = tc.prepare_ref(parent, count)
        assert depth[0].tolist() == d and np.array_equal(anc[0].cpu().numpy(), tc.anc_i64(a)), name
