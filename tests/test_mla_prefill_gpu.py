"""MLA prefill on the GPU: bulk append, K/V up-projection and the 192/128 flash kernel, each against its own reference, so that a
wrong append, a wrong projection and a wrong attention fail differently.  append: torch.equal with single-token mla_kv_append calls
over the WHOLE cache.  kv_up: float64 W[h] c_t from the rows as stored, bound 2^-11 |ref| (one rounding) + 512 * 2^-24 * sum_k |W_k c_k|
(fp32 accumulation in any order).  prefill: float64 plain softmax over kv_up AS STORED and the stored k_pe, rope(q_pe) in float64;
bound as in test_mla_gpu.py, 2^-10 max_{t<=p} |v_t| + 2^-10 |ref|, plus the one thing new here, the fp16 rounding of the rotated q_pe:
it moves a logit by at most d = softmax_scale * 2^-11 * sum_j |q_pe_j| |k_pe_tj|, a softmax weight by a factor e^(+-2d), the output
by at most 2 * max_t d_t * max_t |v_t|.  Inputs: latents 0.5 N(0, 1); every new key is dominant for its own query (head 0); the first
key of the last visible tile for the last query (head 1); the LAST key also for head 2 of the last-but-one query, which must not see
it; decoys of 1e4 at cache slot ctx, in every page outside the block table and in every kv_up row at or past ctx (its sentinel too).

Measured on an MI355X, worst error / bound (Q = 64, KT = 32).  kv_up: 0.67-0.80 over ctx {1, 63, 64, 65, 129} x heads {16, 32}, 0.81
in the ragged batch.  Attention, 16 / 32 heads: (0, 1) exact; (0, 33) 0.109 / 0.090; (0, 65) 0.095 / 0.098; (31, 2) 0.055 / 0.072;
(130, 67) 0.078 / 0.078 (paged = dense); ragged 0.101, 0.062, 0.078; chunked = the one call bit for bit, 0.095; decode step 0.524.
"""
import functools
import re
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV, EPS, L, LAYER, SCALE, RMS_EPS, SENTINEL, DECOY = "cuda:0", 2.0 ** -10, 2, 1, 1.0 / 6.0, 1e-6, 777.0, 1e4


@pytest.fixture(scope="module")
def mla(llmie):
    llmie.build()
    m = re.search(r" q(\d+) kt(\d+) .* tt(\d+) ", llmie.mla_prefill_plan(1, 16, 64, 128, 128)[0])
    return types.SimpleNamespace(lib=llmie, Q=int(m[1]), KT=int(m[2]), TT=int(m[3]))


def rope64(x, tab, pos):
    c, s = (t[:, None] if x.ndim == 3 else t for t in (tab[pos, :, 0], tab[pos, :, 1]))   # pos: a number, or one per row of x [n, heads, 64]
    x0, x1 = x[..., :32], x[..., 32:]
    return np.concatenate([x0 * c - x1 * s, x1 * c + x0 * s], -1)


@functools.lru_cache(maxsize=None)
def make_case(llmie, KT, heads, seqs):
    rng = np.random.default_rng(1000 * heads + sum(h + 7 * n for h, n in seqs))
    f16 = lambda a: a.astype(np.float16)
    c = types.SimpleNamespace(heads=heads, seqs=seqs, B=len(seqs), span=max(h + n for h, n in seqs))
    c.S, c.cum = -(-c.span // 128) * 128, np.concatenate([[0], np.cumsum([n for _, n in seqs])]).astype(np.int32)
    c.tab = llmie.rope_table(c.S, 64, 64, 10000.0)
    c.kv_b, c.gamma = f16(rng.standard_normal((heads, 256, 512)) / np.sqrt(128)), f16(1 + 0.1 * rng.uniform(-1, 1, 512))
    c.q, c.kv_a = f16(rng.standard_normal((c.cum[-1], heads, 192))), f16(0.5 * rng.standard_normal((c.cum[-1], 576)))
    c.cache = f16(0.5 * rng.standard_normal((L, c.B, c.S, 576)))
    for b, (hist, n) in enumerate(seqs):
        ctx, t0 = hist + n, c.cum[b]
        if ctx < c.S:
            c.cache[LAYER, b, ctx] = DECOY
        if n == 0:
            continue
        q_abs = np.einsum("hnc,ihn->ihc", c.kv_b[:, :128].astype(np.float64), c.q[t0:t0 + n, :, :128].astype(np.float64))
        unit = q_abs / np.linalg.norm(q_abs, axis=-1, keepdims=True)
        c.kv_a[t0:t0 + n, :512] = f16(8 * unit[:, 0])          # the diagonal: head 0's direction (RMSNorm sets the length, ~22.6)
        first = (ctx - 1) // KT * KT                           # first key of the last query's last tile: head 1's
        if first < hist:
            c.cache[LAYER, b, first, :512] = f16(22.6 * unit[-1, 1])
        elif first != ctx - 1:
            c.kv_a[t0 + first - hist, :512] = f16(8 * unit[-1, 1])
        if n >= 2:                                             # the last key: a FUTURE key that head 2 of the row before would love
            c.kv_a[t0 + n - 1, :512] = f16(8 * (unit[-1, 0] + unit[-2, 2]))
    return c


class State:   # the device side of a case (all of it, or sequence `only` alone as a batch-1 call): cache, kv_up, out
    def __init__(self, mla, c, paged, only=None):
        self.mla, self.c, self.idx = mla, c, list(range(c.B)) if only is None else [only]
        self.d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        B, d = len(self.idx), self.d
        dense = d(c.cache[:, self.idx])
        self.cache, self.table, self.kw, self.tab = dense, None, {}, d(c.tab)
        if paged:   # shuffled table, two spare pages, decoys wherever no row lives
            mp = c.S // 128
            self.table = torch.randperm(B * mp + 2, generator=torch.Generator().manual_seed(B))[:B * mp].reshape(B, mp).to(DEV)
            self.cache = torch.full((L, B * mp + 2, 128, 576), DECOY, dtype=torch.float16, device=DEV)
            self.cache[:, self.table.flatten()] = dense.view(L, B * mp, 128, 576)
            self.kw = dict(block_table=self.table.int().contiguous(), max_seq_len=c.S)
        self.out = torch.full((int(c.cum[-1]), c.heads * 128), SENTINEL, dtype=torch.float16, device=DEV)

    def pack(self, ranges):   # tokens [a, e) of every sequence's new ones (default: all) -> (packed token ids, cum, hist, max_q_len)
        ranges = ranges or [(0, self.c.seqs[b][1]) for b in self.idx]
        tok = np.concatenate([np.arange(self.c.cum[b] + a, self.c.cum[b] + e) for b, (a, e) in zip(self.idx, ranges)]).astype(np.int64)
        cum = np.concatenate([[0], np.cumsum([e - a for a, e in ranges])]).astype(np.int32)
        hist = np.asarray([self.c.seqs[b][0] + a for b, (a, _) in zip(self.idx, ranges)], np.int32)
        return tok, self.d(cum), self.d(hist), max(e - a for a, e in ranges)

    def step(self, ranges=None, attend=True):   # append (+ up-project + attend: the outputs land in self.out at the case's packed rows)
        llmie, c = self.mla.lib, self.c
        tok, cum, hist, mq = self.pack(ranges)
        llmie.mla_kv_append_rows(self.d(c.kv_a[tok]), self.d(c.gamma), RMS_EPS, self.tab, self.cache, LAYER, cum, hist, mq, c.span, **self.kw)
        if not attend:
            return self
        self.kv_up = torch.full((len(self.idx), c.span, c.heads, 256), DECOY, dtype=torch.float16, device=DEV)
        llmie.mla_kv_up(self.cache, self.d(c.kv_b), self.kv_up, LAYER, cum, hist, mq, **self.kw)
        out = torch.full((len(tok), c.heads * 128), SENTINEL, dtype=torch.float16, device=DEV)
        llmie.mla_prefill(self.d(c.q[tok]), self.kv_up, self.cache, self.tab, LAYER, cum, hist, SCALE, out, mq, **self.kw)
        torch.cuda.synchronize()
        self.out[torch.from_numpy(tok).to(DEV)] = out
        return self

    def rows(self):   # the cache rows as stored, [B, S, 576] float64
        r = self.cache[LAYER, self.table.flatten().long()].view(len(self.idx), self.c.S, 576) if self.table is not None else self.cache[LAYER]
        return r.double().cpu().numpy()


def check(what, got, ref, bound):
    ratio = (np.abs(got.double().cpu().numpy().reshape(ref.shape) - ref) / bound).max()
    print("%s: worst error / bound %.3f" % (what, ratio))
    assert ratio <= 1.0, what


def check_state(st, what, out=None):
    """every sequence: kv_up against float64 W c, its rows at or past ctx untouched; the output rows against the float64 softmax"""
    c, W, rows, out = st.c, st.c.kv_b.astype(np.float64), st.rows(), st.out if out is None else out
    for i, b in enumerate(st.idx):
        hist, n = c.seqs[b]
        ctx, pos = (hist + n if n else 0), hist + np.arange(n)
        assert (st.kv_up[i, ctx:] == DECOY).all(), "%s: kv_up rows of sequence %d at or past %d were written" % (what, b, ctx)
        if n == 0:
            continue
        lat, pe, ku = rows[i, :ctx, :512], rows[i, :ctx, 512:], st.kv_up[i, :ctx].double().cpu().numpy()
        ref = np.einsum("tc,hnc->thn", lat, W)
        check("%s kv_up of sequence %d" % (what, b), st.kv_up[i, :ctx], ref,
              2.0 ** -11 * np.abs(ref) + 512 * 2.0 ** -24 * np.einsum("tc,hnc->thn", np.abs(lat), np.abs(W)))
        q = c.q[c.cum[b]:c.cum[b] + n].astype(np.float64)
        q_rot, seen = rope64(q[..., 128:], c.tab, pos), (np.arange(ctx)[None] <= pos[:, None])[:, None]   # seen: [n, 1, ctx]
        logits = SCALE * (np.einsum("ihn,thn->iht", q[..., :128], ku[..., :128]) + np.einsum("ihj,tj->iht", q_rot, pe))
        p = np.exp(np.where(seen, logits - np.where(seen, logits, -np.inf).max(-1, keepdims=True), -np.inf))
        ref = np.einsum("iht,thv->ihv", p / p.sum(-1, keepdims=True), ku[..., 128:])
        vmax = np.maximum.accumulate(np.abs(ku[..., 128:]), 0)[pos]
        d = SCALE * 2.0 ** -11 * np.where(seen, np.einsum("ihj,tj->iht", np.abs(q_rot), np.abs(pe)), 0).max(-1)
        check("%s sequence %d (hist %d, len %d)" % (what, b, hist, n), out[c.cum[b]:c.cum[b] + n], ref,
              EPS * vmax + EPS * np.abs(ref) + 2 * d[..., None] * vmax)


cases = lambda mla, *exprs: tuple(tuple(eval(e, dict(vars(mla))) for e in pair) for pair in exprs)   # noqa: E731


@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("hist,n", [(0, 1), (0, 3), (126, 5)])
def test_bulk_append_equals_single_token_appends(mla, hist, n, paged):
    c = make_case(mla.lib, mla.KT, 16, ((hist, n),))
    bulk, single = State(mla, c, paged).step(attend=False), State(mla, c, paged)
    for i in range(n):
        mla.lib.mla_kv_append(single.d(c.kv_a[i:i + 1]), single.d(c.gamma), RMS_EPS, single.tab, single.cache, LAYER,
                              single.d(np.asarray([hist + i + 1], np.int32)), **single.kw)
    assert torch.equal(bulk.cache, single.cache) and not torch.equal(bulk.cache, State(mla, c, paged).cache)


@pytest.mark.parametrize("ctx", ["1", "TT-1", "TT", "TT+1", "2*TT+1"])
@pytest.mark.parametrize("heads", [16, 32])
def test_kv_up_against_float64(mla, heads, ctx):
    ctx = cases(mla, (ctx,))[0][0]
    c = make_case(mla.lib, mla.KT, heads, ((ctx - 1, 1), (5, 0)))   # history ctx - 1 and one new token; a sequence without new tokens
    dense, paged = State(mla, c, False).step(), State(mla, c, True).step()
    check_state(dense, "heads %d ctx %d" % (heads, ctx))
    assert torch.equal(dense.kv_up, paged.kv_up), "paged differs from dense"


@pytest.mark.parametrize("expr", [("0", "1"), ("0", "KT+1"), ("0", "Q+1"), ("KT-1", "2"), ("130", "Q+3")])
@pytest.mark.parametrize("heads", [16, 32])
def test_attention_against_float64(mla, heads, expr):
    c = make_case(mla.lib, mla.KT, heads, cases(mla, expr))
    dense = State(mla, c, False).step()
    check_state(dense, "heads %d dense" % heads)
    if expr[0] == "130":
        paged = State(mla, c, True).step()
        check_state(paged, "heads %d paged" % heads)
        assert torch.equal(paged.out, dense.out) and np.array_equal(paged.rows()[0, :c.span], dense.rows()[0, :c.span]), "paged differs from dense"


@pytest.mark.parametrize("paged", [False, True])
def test_ragged_batch_rows_equal_the_batch_1_calls(mla, paged):
    c = make_case(mla.lib, mla.KT, 32, cases(mla, ("0", "Q+1"), ("3", "0"), ("129", "5"), ("KT-1", "2")))
    st = State(mla, c, paged).step()
    check_state(st, "ragged paged=%s" % paged)   # (and: the sequence without new tokens kept its sentinel rows)
    assert not (st.out == SENTINEL).all(1).any(), "a live output row was not written"
    for b in (0, 2, 3):
        one = State(mla, c, paged, only=b).step()
        assert torch.equal(one.out[c.cum[b]:c.cum[b + 1]], st.out[c.cum[b]:c.cum[b + 1]]), "sequence %d differs from its batch-1 call" % b


def test_chunked_prefill_equals_the_one_call(mla):
    """a row's tiles, and what a masked key adds (exactly 0), do not depend on the cut: caches AND outputs are bit-equal"""
    c = make_case(mla.lib, mla.KT, 16, ((0, mla.Q + 1),))
    whole = State(mla, c, False).step()
    cut = State(mla, c, False).step([(0, mla.KT - 1)]).step([(mla.KT - 1, mla.Q + 1)])
    check_state(whole, "one call")
    check_state(whole, "two calls", out=cut.out)   # (against the one-call reference)
    assert torch.equal(cut.cache, whole.cache) and torch.equal(cut.out, whole.out)


def test_prefill_then_one_decode_step(mla):
    """append + absorb + decode + out project at ctx KT + 2 against the float64 un-absorbed reference, from the rows as stored"""
    llmie, n, heads, rng = mla.lib, mla.KT + 1, 16, np.random.default_rng(5)
    c = make_case(llmie, mla.KT, heads, ((0, n),))
    st, empty = State(mla, c, False).step(attend=False), lambda *shape: torch.empty(shape, dtype=torch.float16, device=DEV)
    kv_a, q = (0.5 * rng.standard_normal((1, 576))).astype(np.float16), rng.standard_normal((1, heads, 192)).astype(np.float16)
    ctx_len, kv_b = st.d(np.asarray([n + 1], np.int32)), st.d(c.kv_b)
    llmie.mla_kv_append(st.d(kv_a), st.d(c.gamma), RMS_EPS, st.tab, st.cache, LAYER, ctx_len)
    q_lat = llmie.mla_q_absorb(st.d(q), kv_b, st.tab, empty(1, heads, 576), ctx_len, c.S)
    o_lat = llmie.mla_decode(q_lat, st.cache, LAYER, ctx_len, SCALE, empty(1, heads, 512), llmie.mla_workspace(1, heads, c.S))
    out = llmie.mla_out_project(o_lat, kv_b, empty(1, heads * 128))
    torch.cuda.synchronize()
    rows, W, q64 = st.rows()[0, :n + 1], c.kv_b.astype(np.float64), q[0].astype(np.float64)
    k_nope, v = np.einsum("tc,hnc->htn", rows[:, :512], W[:, :128]), np.einsum("tc,hvc->htv", rows[:, :512], W[:, 128:])
    logits = SCALE * (np.einsum("hn,htn->ht", q64[:, :128], k_nope) + rope64(q64[:, 128:], c.tab, n) @ rows[:, 512:].T)
    p = np.exp(logits - logits.max(-1, keepdims=True))
    ref = np.einsum("ht,htv->hv", p / p.sum(-1, keepdims=True), v)
    check("decode step after a prefill", out[0], ref, EPS * np.abs(v).max(1) + EPS * np.abs(ref))
