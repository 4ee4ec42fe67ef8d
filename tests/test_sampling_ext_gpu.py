"""llmie_sample_logits_ext / llmie_lm_head_sample_ext: allowed-token masks, logit bias, stop sets with min_step, top-N.

The header says the sampler works on the row "read as fp32", and that an excluded token is treated as a NaN logit is.  So the
main check needs no tolerance: the extension on (logits, mask, bias, min_step) must pick exactly what llmie_sample_logits picks
on an fp32 row built here in numpy -- float32(logits) + bias (last entry of an id wins, one fp32 add), NaN at every excluded
token.  Ignored bias entries (NaN, +inf, ids outside [0, V)) are dropped before "last wins" is applied, as the header states.
The top-N is checked against numpy's lexsort on the raw row and float64 log-softmax (1e-4, the bound test_sampling_params_gpu
applies to out_logprob).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import test_sampling_params_gpu as base

pytestmark = pytest.mark.gpu
DEV, END = base.DEV, base.END
DTYPES = [torch.float16, torch.float32]
VOCABS = [7, 1000, 32001]     # below one mask word and below top_n; a tail word with bits past V; several sweeps + an odd tail
BATCHES = [1, 5]
SETS = [dict(c) for c in base.CASES] + [dict(temperature=0.0),
                                        dict(temperature=0.9, repetition_penalty=1.4, presence_penalty=0.3, frequency_penalty=0.2)]
STRIDE = 16


def _words(allowed, rng, garbage=True):
    """bool [rows, V] -> uint32 words with one spare word per row; the bits at and past V hold garbage"""
    rows, V = allowed.shape
    stride = (V + 31) // 32 + 1
    bits = np.zeros((rows, stride * 32), bool)
    if garbage:
        bits[:] = rng.random(bits.shape) < 0.5
    bits[:, :V] = allowed
    return np.packbits(bits.reshape(rows, stride, 32), axis=-1, bitorder="little").view("<u4").reshape(rows, stride)


class Controls:
    """one batch's controls, as numpy, and what they make of a raw row"""

    def __init__(self, rng, bs, V, step):
        self.V, self.bs = V, bs
        self.allowed = rng.random((3, V)) < 0.4
        self.allowed[0, rng.integers(0, V)] = True
        self.mask_index = np.array([0, -1, 1, 1, 7][:bs], np.int32)   # rows 2 and 3 share a mask row; -1 and 7: unconstrained
        self.words = _words(self.allowed, rng)
        far = [-1, -5, V, V + 3, 2**31 - 1]
        self.bias = []
        for b in range(bs):
            n = [0, 3, 40, 300, 9][b % 5] if V > 7 else [0, 3, 12, 30, 9][b % 5]
            ids = rng.integers(0, V, n)
            if n >= 3:
                ids[n // 2:] = ids[:n - n // 2]             # every id of the first half again: duplicates
            vals = (rng.standard_normal(n) * 4).astype(np.float32)
            row = [(int(i), float(v)) for i, v in zip(ids, vals)]
            if n:
                row += [(int(rng.choice(far)), 50.0), (int(ids[0]), float("nan")), (int(rng.integers(0, V)), float("inf")),
                        (int(rng.integers(0, V)), float("-inf")), (int(rng.integers(0, V)), float("-inf"))]
            self.bias.append(row)
        self.stops = [[int(t) for t in rng.integers(0, V, [0, 2, 16, 0, 5][b % 5])] for b in range(bs)]
        self.min_step = np.array([step + 1, step, 0, step + 9, step - 1][:bs], np.int32)   # rows 0 and 3 hold end / stops back

    def ext(self, llmie, top_n=0, mask=True, bias=True, stops=True):
        return llmie.sampling_ext(self.bs, self.V, masks=self.words if mask else None, mask_index=self.mask_index if mask else None,
                                  bias=self.bias if bias else None, stops=self.stops if stops else None,
                                  min_step=self.min_step if stops else None, top_n=top_n)

    def rows(self, raw, step):
        """the fp32 rows llmie_sample_logits must be given to pick the same tokens"""
        out = raw.astype(np.float32).copy()
        for b in range(self.bs):
            last = {}
            for t, v in self.bias[b]:
                if 0 <= t < self.V and not np.isnan(v) and v != np.inf:
                    last[t] = np.float32(v)
            for t, v in last.items():
                out[b, t] = np.nan if v == -np.inf else np.float32(out[b, t] + v)
            m = self.mask_index[b]
            if 0 <= m < self.allowed.shape[0]:
                out[b, ~self.allowed[m]] = np.nan
            if step < self.min_step[b]:
                for t in self.stops[b] + [END]:
                    if 0 <= t < self.V:
                        out[b, t] = np.nan
        return out

    def finished(self, picks):
        return np.array([p == END or p in self.stops[b] for b, p in enumerate(picks)], np.uint8)


def _state(rng, bs, V):
    hist = rng.integers(0, V, (bs, STRIDE)).astype(np.int32)
    hlen = rng.integers(0, STRIDE, bs).astype(np.int32)
    return hist, hlen


def _run(llmie, logits, params, step, hist, ext=None, step_dev=None):
    st = base.State(logits.shape[0], STRIDE, hist)
    llmie.sample_logits(logits, llmie.sampling_params(params), st.seq, st.fin, st.out, step, END, history=st.hist,
                        history_len=st.hlen, append=True, out_logprob=st.lp, step_dev=step_dev, ext=ext)
    torch.cuda.synchronize()
    return st


def _raw(rng, bs, V, dtype):
    raw = base._logits(rng, bs, V, dtype, 2.0)
    raw[:, rng.integers(0, V, max(1, V // 50))] = np.nan
    return raw


# ------------------------------------------------------------------ 1. exact equivalence
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("bs", BATCHES)
def test_equals_plain_sampler_on_the_patched_row(llmie, dtype, V, bs):
    rng = np.random.default_rng(11 * V + bs)
    step = 77
    raw = _raw(rng, bs, V, dtype)
    ctl = Controls(rng, bs, V, step)
    hist = _state(rng, bs, V)
    logits, ref_logits = base._dev(raw, dtype), base._dev(ctl.rows(raw, step))
    ext = ctl.ext(llmie)
    for i, cfg in enumerate(SETS):
        params = [dict(cfg, seed=1000 + 17 * b + i) for b in range(bs)]
        got = _run(llmie, logits, params, step, hist, ext=ext)
        ref = _run(llmie, ref_logits, params, step, hist)
        assert torch.equal(got.out, ref.out), "%s: %s vs %s" % (cfg, got.out.tolist(), ref.out.tolist())
        assert torch.equal(got.seq, ref.seq) and torch.equal(got.hist, ref.hist) and torch.equal(got.hlen, ref.hlen)
        picks = got.out.cpu().numpy()
        fin = got.fin.cpu().numpy()
        assert np.array_equal(fin, ctl.finished(picks))
        empty = np.array([not s for s in ctl.stops])
        assert np.array_equal(fin[empty], ref.fin.cpu().numpy()[empty])


# ------------------------------------------------------------------ 2. identity
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", VOCABS)
def test_no_extension_is_the_existing_entry(llmie, dtype, V):
    rng = np.random.default_rng(V)
    bs, step = 5, 31
    logits = base._dev(_raw(rng, bs, V, dtype), dtype)
    hist = _state(rng, bs, V)
    params = [dict(SETS[(b + 3) % len(SETS)], seed=b) for b in range(bs)]
    old = _run(llmie, logits, params, step, hist)
    nulls = _run(llmie, logits, params, step, hist, ext=llmie.SamplingExt())
    # ext == NULL itself, through the raw entry
    st = base.State(bs, STRIDE, hist)
    ws = torch.empty(llmie.sample_logits_workspace_bytes(bs, V), dtype=torch.uint8, device=DEV)
    pd = llmie.sampling_params(params)
    rc = llmie.lib().llmie_sample_logits_ext(logits.data_ptr(), bs, V, pd.data_ptr(), st.hist.data_ptr(), STRIDE,
                                             st.hlen.data_ptr(), 1, st.seq.data_ptr(), st.fin.data_ptr(), st.out.data_ptr(),
                                             st.lp.data_ptr(), step, None, END, ws.data_ptr(), ws.numel(), llmie._dt(logits),
                                             torch.cuda.current_stream().cuda_stream, None)
    torch.cuda.synchronize()
    assert rc == 0
    for other in (nulls, st):
        assert torch.equal(other.out, old.out) and torch.equal(other.lp.view(torch.int32), old.lp.view(torch.int32))
        assert torch.equal(other.seq, old.seq) and torch.equal(other.fin, old.fin)
        assert torch.equal(other.hist, old.hist) and torch.equal(other.hlen, old.hlen)


# ------------------------------------------------------------------ 3. mask edges
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", VOCABS)
def test_mask_edges(llmie, dtype, V):
    rng = np.random.default_rng(5 * V)
    bs, step = 5, 9
    raw = _raw(rng, bs, V, dtype)
    logits = base._dev(raw, dtype)
    hist = _state(rng, bs, V)
    only = int(rng.integers(0, V))
    while np.isnan(raw[:, only]).any():
        only = (only + 1) % V
    allowed = np.zeros((3, V), bool)       # row 0: nothing; row 1: one token; row 2: a random set
    allowed[1, only] = True
    allowed[2] = rng.random(V) < 0.5
    allowed[2, only] = True
    index = np.array([0, 1, -1, 2, 1], np.int32)
    for cfg in SETS:
        params = [dict(cfg, seed=b) for b in range(bs)]
        plain = _run(llmie, logits, params, step, hist)
        outs = []
        for garbage in (True, False):
            ext = llmie.sampling_ext(bs, V, masks=_words(allowed, rng, garbage), mask_index=index)
            outs.append(_run(llmie, logits, params, step, hist, ext=ext))
        got = outs[0]
        for name in ("out", "fin", "seq", "hist", "lp"):   # garbage past V changes nothing
            assert torch.equal(getattr(outs[0], name), getattr(outs[1], name)), name
        picks, fin = got.out.cpu().numpy(), got.fin.cpu().numpy()
        assert picks[0] == END and fin[0] == 1                       # no token left
        assert picks[1] == only and picks[4] == only, cfg             # one token left, under every parameter set
        assert picks[2] == plain.out[2].item() and got.lp[2].item() == plain.lp[2].item()   # mask_index -1: unconstrained
        assert allowed[2, picks[3]]


# ------------------------------------------------------------------ 4. bias edges
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", VOCABS)
def test_bias_edges(llmie, dtype, V):
    rng = np.random.default_rng(3 * V)
    raw = base._logits(rng, 1, V, dtype, 1.0)
    order = np.lexsort((np.arange(V), -raw[0]))
    top, second, low = int(order[0]), int(order[1]), int(order[-1])
    inf, nan = float("inf"), float("nan")
    cases = [([], top), ([(low, 50.0), (low, -50.0)], top), ([(low, -50.0), (low, 50.0)], low),
             ([(low, 50.0), (top, 1.0), (low, -50.0), (low, 60.0)], low),
             ([(-1, 90.0), (V, 90.0), (V + 7, 90.0), (2**31 - 1, 90.0), (-2**31, 90.0)], top),
             ([(top, -inf)], second), ([(top, -inf), (second, -inf), (low, 0.5)], int(order[2])),
             ([(top, -inf), (top, 5.0)], top),            # the last entry wins over a ban too
             ([(low, nan), (second, inf)], top), ([(low, 50.0), (low, nan), (low, inf)], low)]   # ignored entries shadow nothing
    bs = len(cases)
    logits = base._dev(np.tile(raw, (bs, 1)), dtype)
    hist = (np.zeros((bs, STRIDE), np.int32), np.zeros(bs, np.int32))
    greedy = [dict(temperature=0.0)] * bs
    ext = llmie.sampling_ext(bs, V, bias=[c[0] for c in cases])
    got = _run(llmie, logits, greedy, 4, hist, ext=ext)
    assert got.out.tolist() == [c[1] for c in cases]
    # out_logprob stays that of the raw row
    lse = np.log(np.exp(raw[0].astype(np.float64) - raw[0].max()).sum()) + raw[0].max()
    for b, c in enumerate(cases):
        assert abs(got.lp[b].item() - (float(raw[0, c[1]]) - lse)) <= 1e-4
    # bias_len 0: nothing applies; bias_len above the stride: clamped to it
    full = [[(low, 50.0)] * 3 + [(second, 70.0)]] * bs
    ext = llmie.sampling_ext(bs, V, bias=full)
    ext.bias_len.copy_(torch.tensor([0, 4, 9, 3, 10**6, -5] + [4] * (bs - 6), dtype=torch.int32))
    got = _run(llmie, logits, greedy, 4, hist, ext=ext)
    assert got.out.tolist() == [top, second, second, low, second, top] + [second] * (bs - 6)


# ------------------------------------------------------------------ 5. top-N
def _top_rows(rng, V, dtype):
    """raw rows with ties across the N boundary, NaNs, and rows with fewer valid tokens than N"""
    raw = base._logits(rng, 5, V, dtype, 2.0)
    k = min(V, 24)
    tie = rng.choice(V, k, replace=False)
    raw[0, tie] = np.float32(9.5)             # k equal maxima: the boundary of every N < k cuts through them
    raw[1, tie[:k // 2]] = np.float32(7.0)
    raw[1, tie[k // 2:]] = np.nan
    raw[2, :] = np.nan
    raw[2, tie[:3]] = [1.0, 1.0, -2.0]        # 3 valid tokens
    raw[3, rng.integers(0, V, max(1, V // 3))] = np.nan
    raw[4, :] = np.nan                        # none
    return raw


def _top_ref(row, N):
    ok = np.nonzero(~np.isnan(row))[0]
    order = ok[np.lexsort((ok, -row[ok]))][:N]
    ids = np.full(N, -1, np.int64)
    lps = np.full(N, -np.inf)
    if ok.size:
        v = row[ok].astype(np.float64)
        lse = v.max() + np.log(np.exp(v - v.max()).sum())
        ids[:order.size] = order
        lps[:order.size] = row[order].astype(np.float64) - lse
    return ids, lps


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("N", [1, 20, 32])
def test_top_n(llmie, dtype, V, N):
    rng = np.random.default_rng(V + N)
    bs, step = 5, 3
    raw = _top_rows(rng, V, dtype)
    logits = base._dev(raw, dtype)
    hist = _state(rng, bs, V)
    ctl = Controls(rng, bs, V, step)
    alone = llmie.sampling_ext(bs, V, top_n=N)
    a = _run(llmie, logits, [dict(temperature=0.0)] * bs, step, hist, ext=alone)
    ids, lps = alone.top_ids.cpu().numpy(), alone.top_logprobs.cpu().numpy()
    for b in range(bs):
        eids, elps = _top_ref(raw[b], N)
        assert np.array_equal(ids[b], eids), "row %d: %s vs %s" % (b, ids[b], eids)
        n = int((eids >= 0).sum())
        assert np.abs(lps[b, :n] - elps[:n]).max(initial=0.0) <= 1e-4
        assert np.isneginf(lps[b, n:]).all()
        if n:   # the greedy pick of a plain row is the first alternative, with its log-probability
            assert a.out[b].item() == eids[0] and abs(a.lp[b].item() - elps[0]) <= 1e-4
    # independent of every control
    every = ctl.ext(llmie, top_n=N)
    params = [dict(temperature=1.3, top_k=5, top_p=0.8, repetition_penalty=1.5, frequency_penalty=0.3, seed=b) for b in range(bs)]
    got = _run(llmie, logits, params, step, hist, ext=every)
    assert torch.equal(every.top_ids, alone.top_ids)
    assert torch.equal(every.top_logprobs.view(torch.int32), alone.top_logprobs.view(torch.int32))
    picks, patched = got.out.cpu().numpy(), ctl.rows(raw, step)
    for b in range(bs):   # the pick's log-probability is the raw row's (a row with no token left reports -inf)
        if np.isnan(patched[b]).all():
            assert picks[b] == END and np.isneginf(got.lp[b].item())
            continue
        v = raw[b][~np.isnan(raw[b])].astype(np.float64)
        assert abs(got.lp[b].item() - (float(raw[b, picks[b]]) - (v.max() + np.log(np.exp(v - v.max()).sum())))) <= 1e-4


# ------------------------------------------------------------------ 6. stops and min_step
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", VOCABS)
def test_stops_and_min_step(llmie, dtype, V):
    rng = np.random.default_rng(V)
    raw = base._logits(rng, 1, V, dtype, 1.0)
    raw[0, END] = raw[0].max() + 1          # the arg-max is end_id
    order = np.lexsort((np.arange(V), -raw[0]))
    second, third = int(order[1]), int(order[2])
    logits = base._dev(raw, dtype)
    hist = (np.zeros((1, STRIDE), np.int32), np.zeros(1, np.int32))
    greedy = [dict(temperature=0.0)]
    ext = llmie.sampling_ext(1, V, stops=[[]], min_step=[10])
    step_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    for step in (0, 8, 9, 10, 11, 500):
        exp = second if step < 10 else END
        got = _run(llmie, logits, greedy, step, hist, ext=ext)
        assert got.out.item() == exp and got.fin.item() == (exp == END), step
        step_dev.fill_(step)
        got = _run(llmie, logits, greedy, -123, hist, ext=ext, step_dev=step_dev)
        assert got.out.item() == exp and got.fin.item() == (exp == END), step
    # the runner-up is a stop token: held back with end_id before min_step, finishing the row from min_step on
    ext = llmie.sampling_ext(1, V, stops=[[second, V + 4, -3]], min_step=[10])
    got = _run(llmie, logits, greedy, 9, hist, ext=ext)
    assert got.out.item() == third and got.fin.item() == 0
    ext.min_step.fill_(0)
    raw2 = raw.copy()
    raw2[0, END] = raw[0].min() - 1
    got = _run(llmie, base._dev(raw2, dtype), greedy, 9, hist, ext=ext)
    assert got.out.item() == second and got.fin.item() == 1 and got.seq.item() == 6
    # stops without a min_step: nothing is held back
    ext = llmie.sampling_ext(1, V, stops=[[second]])
    got = _run(llmie, logits, greedy, 0, hist, ext=ext)
    assert got.out.item() == END and got.fin.item() == 1


# ------------------------------------------------------------------ 7. determinism and batch invariance
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", VOCABS)
def test_determinism_and_batch_invariance(llmie, dtype, V):
    rng = np.random.default_rng(2 * V)
    bs, step, N = 5, 99, 20
    raw = _raw(rng, bs, V, dtype)
    ctl = Controls(rng, bs, V, step)
    hist = _state(rng, bs, V)
    params = [dict(SETS[(2 * b + 1) % len(SETS)], seed=7 * b) for b in range(bs)]
    logits = base._dev(raw, dtype)
    runs = []
    for _ in range(2):
        ext = ctl.ext(llmie, top_n=N)
        st = _run(llmie, logits, params, step, hist, ext=ext)
        runs.append((st.out, st.lp.view(torch.int32), st.hist, st.fin, ext.top_ids, ext.top_logprobs.view(torch.int32)))
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    # row 3 alone, with its own controls in slot 0
    b = 3
    one = llmie.sampling_ext(1, V, masks=ctl.words, mask_index=ctl.mask_index[b:b + 1], bias=[ctl.bias[b]], stops=[ctl.stops[b]],
                             min_step=ctl.min_step[b:b + 1], top_n=N)
    st = _run(llmie, logits[b:b + 1].contiguous(), [params[b]], step, (hist[0][b:b + 1], hist[1][b:b + 1]), ext=one)
    out, lp, _, fin, tid, tlp = runs[0]
    assert st.out[0] == out[b] and st.lp.view(torch.int32)[0] == lp[b] and st.fin[0] == fin[b]
    assert torch.equal(one.top_ids[0], tid[b]) and torch.equal(one.top_logprobs.view(torch.int32)[0], tlp[b])


# ------------------------------------------------------------------ 8. decoder entry under a graph
def test_lm_head_sample_ext_graph(llmie):
    dtype, V = torch.float16, 32000
    dec, x, gam, lm, emb = base._decoder(llmie, dtype, V, 1)
    rng = np.random.default_rng(8)
    pd = llmie.sampling_params([dict(temperature=0.8, top_p=0.9, repetition_penalty=1.3, seed=12345)])
    ws = torch.empty(llmie.sample_logits_workspace_bytes(1, V), dtype=torch.uint8, device=DEV)
    logits = torch.empty((1, V), dtype=dtype, device=DEV)
    hid, nxt = torch.empty_like(x), torch.empty_like(x)
    st = base.State(1, STRIDE, (np.zeros((1, STRIDE), np.int32), np.zeros(1, np.int32)))
    step_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    ext = llmie.sampling_ext(1, V, masks=np.ones((1, V), bool), stops=[[5, 6]], min_step=[0], top_n=5)

    def one():
        hid.copy_(x)
        dec.lm_head_sample_params(hid, gam, lm, llmie.W_F16, logits, pd, st.seq, st.fin, st.out, -1, END, history=st.hist,
                                  history_len=st.hlen, append=True, out_logprob=st.lp, step_dev=step_dev, embed=emb,
                                  next_hidden=nxt, advance=True, workspace=ws, ext=ext)

    def load(mask, min_step):
        st.hist.zero_(), st.hlen.zero_(), st.seq.zero_(), st.fin.zero_(), nxt.zero_()
        step_dev.fill_(100)
        ext.mask.copy_(torch.from_numpy(llmie.pack_token_mask(mask).view(np.int32)).to(DEV))
        ext.min_step.fill_(min_step)

    def result():
        torch.cuda.synchronize()
        return st.out.clone(), st.lp.clone(), st.fin.clone(), nxt.clone(), ext.top_ids.clone(), ext.top_logprobs.clone(), step_dev.clone()

    load(np.ones((1, V), bool), 0)
    one()
    free = int(st.out.item())
    contents = []
    for i in range(3):
        mask = rng.random((1, V)) < 0.3
        mask[0, free] = False           # the unconstrained pick is never allowed
        mask[0, END] = True
        contents.append((mask, [0, 10**6, 0][i]))
    eager = []
    for mask, ms in contents:
        load(mask, ms)
        one()
        eager.append(result())
        assert mask[0, int(st.out.item())] and int(st.out.item()) != free
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        one()   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        one()
    for (mask, ms), exp in zip(contents, eager):
        load(mask, ms)
        torch.cuda.synchronize()
        g.replay()
        for a, b in zip(result(), exp):
            assert torch.equal(a, b)
    dec.close()
