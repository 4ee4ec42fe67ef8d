"""Per-request sampling controls (llmie_sample_logits, llmie_lm_head_sample_params) against a float64 numpy oracle.

The oracle follows include/llmie.h step by step: penalties and temperature in fp32 (the values the device orders), masses
exp(v - max) in float64, top-k / top-p / min-p as prefixes of the (value desc, id asc) order, and the draw with
orc.uniform_philox(step, seed).  A pick may differ from the oracle's only where the oracle itself sits on a boundary (u, top_p
or min_p within 1e-5 of a cumulative mass), and on at most 0.4 % of the rows.
"""
import numpy as np
import pytest
import torch

import oracle as orc

DEV = "cuda"
DTYPES = [torch.float32, torch.float16]
VOCABS = [7, 1000, 32000, 32001, 128256]
BATCHES = [1, 5, 128]
END = 2
FLT_MAX = np.float32(np.finfo(np.float32).max)
TIE = 1e-5

pytestmark = pytest.mark.gpu


def _logits(rng, bs, V, dtype, scale=3.0):
    x = (rng.standard_normal((bs, V)) * scale).astype(np.float32)
    if dtype == torch.float16:
        x = x.astype(np.float16).astype(np.float32)
    return x


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.to(dtype) if dtype is not None else t


def _clamp(p, V):
    p = dict(dict(temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, repetition_penalty=1.0, presence_penalty=0.0,
                  frequency_penalty=0.0, seed=0), **p)
    f32 = lambda v: float(np.float32(v))
    t = f32(p["temperature"])
    t = t if t >= 0 else 0.0   # NaN -> 0 too
    k = min(max(int(p["top_k"]), 0), V)
    tp = f32(p["top_p"])
    if not tp > 0:
        k, tp = 1, 1.0
    tp = min(tp, 1.0)
    mp = f32(p["min_p"])
    mp = min(mp, 1.0) if mp >= 0 else 0.0
    rep = f32(p["repetition_penalty"])
    rep = rep if rep > 0 else 1.0
    return dict(temperature=t, top_k=k, top_p=tp, min_p=mp, rep=rep, presence=f32(p["presence_penalty"]),
                frequency=f32(p["frequency_penalty"]), seed=int(p["seed"]) & 0xffffffff)


def ref_row(raw, p, hist, step):
    """(pick, fragile, logprob) of one row; raw: the fp32 values the device reads"""
    V = raw.size
    c = _clamp(p, V)
    l = raw.astype(np.float32).copy()
    h = np.asarray(hist, np.int64)
    h = h[(h >= 0) & (h < V)]
    if h.size and (c["rep"] != 1 or c["presence"] != 0 or c["frequency"] != 0):
        ids, cnt = np.unique(h, return_counts=True)
        x = l[ids]
        x = np.where(x > 0, x / np.float32(c["rep"]), x * np.float32(c["rep"])).astype(np.float32)
        x = (x - np.float32(c["presence"])).astype(np.float32)
        x = (x - cnt.astype(np.float32) * np.float32(c["frequency"])).astype(np.float32)
        l[ids] = x
    valid = ~np.isnan(l)
    rv = raw.astype(np.float64)[~np.isnan(raw)]
    lse = rv.max() + np.log(np.exp(rv - rv.max()).sum()) if rv.size else 0.0
    if not valid.any():
        return END, False, None
    if c["temperature"] == 0:
        vals = np.where(valid, l, -np.inf)
        top = vals.max()
        cand = np.nonzero(valid & (vals == top))[0]
        pick = int(cand[0])
        return pick, False, float(raw[pick]) - lse
    v = np.clip((l / np.float32(c["temperature"])).astype(np.float32), -FLT_MAX, FLT_MAX)
    ids = np.nonzero(valid)[0]
    vv = v[ids]
    order = ids[np.lexsort((ids, -vv))]
    vo = v[order].astype(np.float64)
    mass = np.exp(vo - vo[0])
    n = order.size
    fragile = False
    if 0 < c["top_k"] < n:
        n = c["top_k"]
    if c["top_p"] < 1:
        cum = np.cumsum(mass[:n])
        tgt = c["top_p"] * cum[-1]
        i = int(np.searchsorted(cum, tgt, side="left"))
        i = min(i, n - 1)
        fragile |= bool(np.min(np.abs(cum - tgt)) < TIE * cum[-1])
        n = int(np.count_nonzero(vo[:n] >= vo[i]))
    if c["min_p"] > 0:
        keep = mass[:n] >= c["min_p"]
        fragile |= bool(np.min(np.abs(mass[:n] - c["min_p"])) < TIE)
        n = int(np.count_nonzero(keep))
    cum = np.cumsum(mass[:n])
    u = orc.uniform_philox(step & 0xffffffff, c["seed"])
    tgt = u * cum[-1]
    j = int(np.searchsorted(cum, tgt, side="right"))
    j = min(j, n - 1)
    fragile |= bool(np.min(np.abs(cum - tgt)) < TIE * cum[-1])
    pick = int(order[j])
    return pick, fragile, float(raw[pick]) - lse


class State:
    def __init__(self, bs, stride=0, hist=None, seq0=5):
        self.seq = torch.full((bs,), seq0, dtype=torch.int32, device=DEV)
        self.fin = torch.zeros(bs, dtype=torch.uint8, device=DEV)
        self.out = torch.full((bs,), -7, dtype=torch.int32, device=DEV)
        self.lp = torch.zeros(bs, dtype=torch.float32, device=DEV)
        self.hist = None if stride == 0 else _dev(hist[0].astype(np.int32))
        self.hlen = None if stride == 0 else _dev(hist[1].astype(np.int32))


def run(llmie, logits, params, step, st, append=False, step_dev=None):
    pd = llmie.sampling_params(params)
    llmie.sample_logits(logits, pd, st.seq, st.fin, st.out, step, END, history=st.hist, history_len=st.hlen, append=append,
                        out_logprob=st.lp, step_dev=step_dev)
    torch.cuda.synchronize()
    return st.out.cpu().numpy()


CASES = [dict(top_p=0.5), dict(top_p=0.9), dict(top_p=0.99), dict(min_p=0.05), dict(min_p=0.3), dict(temperature=0.3),
         dict(temperature=1.7), dict(temperature=0.7, top_p=0.9, min_p=0.02), dict(temperature=1.3, top_k=20, top_p=0.8),
         dict(top_k=50, min_p=0.1, temperature=0.5), dict(top_k=3, top_p=0.5, temperature=2.0)]


def _check_rows(got, raw, params, hists, step, lp=None, limit=0.004):
    bad = []
    for b in range(raw.shape[0]):
        pick, fragile, elp = ref_row(raw[b], params[b], hists[b] if hists else [], step)
        if got[b] != pick:
            assert fragile, "row %d: picked %d, the oracle %d (%s)" % (b, got[b], pick, params[b])
            bad.append(b)
        elif lp is not None and elp is not None:
            assert abs(lp[b] - elp) <= 1e-4, "row %d: logprob %g vs %g" % (b, lp[b], elp)
    assert len(bad) <= max(1, limit * raw.shape[0]), "%d of %d rows differ" % (len(bad), raw.shape[0])
    return bad


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("bs", BATCHES)
def test_greedy(llmie, dtype, V, bs):
    rng = np.random.default_rng(V + bs)
    raw = _logits(rng, bs, V, dtype)
    for b in range(bs):
        if b % 3 == 1:
            raw[b, rng.integers(0, V, max(1, V // 10))] = np.nan
        if b % 3 == 2 and V > 3:   # a tie at the maximum: the lower id wins
            i, j = sorted(rng.choice(V, 2, replace=False))
            raw[b, i] = raw[b, j] = np.nanmax(raw[b]) + 1
    if bs > 1:
        raw[bs - 1] = np.nan
    logits = _dev(raw, dtype)
    st = State(bs)
    got = run(llmie, logits, [dict(temperature=0.0, seed=b) for b in range(bs)], 11, st)
    for b in range(bs):
        v = np.where(np.isnan(raw[b]), -np.inf, raw[b])
        exp = END if np.isnan(raw[b]).all() else int(np.argmax(v))
        assert got[b] == exp, "row %d" % b
    fin = st.fin.cpu().numpy()
    assert np.array_equal(fin.astype(bool), got == END)
    assert np.array_equal(st.seq.cpu().numpy(), np.full(bs, 6))
    if bs > 1:
        assert got[bs - 1] == END and fin[bs - 1] == 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("bs", BATCHES)
@pytest.mark.parametrize("K", [1, 4, 32])
def test_matches_topk_sampling(llmie, dtype, V, bs, K):
    K = min(K, V)   # llmie_topk needs K <= vocab
    rng = np.random.default_rng(3 * V + bs + K)
    raw = _logits(rng, bs, V, dtype, 1.0)
    logits = _dev(raw, dtype)
    step = 1234
    tid = torch.empty((bs, 8, K), dtype=torch.int32, device=DEV)
    tv = torch.empty((bs, 8, K), dtype=dtype, device=DEV)
    ids = torch.empty((bs, K), dtype=torch.int32, device=DEV)
    vals = torch.empty((bs, K), dtype=dtype, device=DEV)
    llmie.topk(logits, tid, tv, ids, vals)
    seq = torch.zeros(bs, dtype=torch.int32, device=DEV)
    fin = torch.zeros(bs, dtype=torch.uint8, device=DEV)
    old = torch.empty(bs, dtype=torch.int32, device=DEV)
    llmie.sampling(ids, vals, seq, fin, old, step, END, V)
    st = State(bs, seq0=0)
    params = [dict(top_k=K, seed=b) for b in range(bs)]
    got = run(llmie, logits, params, step, st)
    old = old.cpu().numpy()
    diff = np.nonzero(got != old)[0]
    assert diff.size <= max(1, 0.004 * bs)
    for b in diff:
        pick, fragile, _ = ref_row(raw[b], params[b], [], step)
        assert fragile and pick in (got[b], old[b]), "row %d: %d vs %d is not a boundary tie" % (b, got[b], old[b])
    assert np.array_equal(st.seq.cpu().numpy(), seq.cpu().numpy())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("bs", BATCHES)
def test_oracle_agreement(llmie, dtype, V, bs):
    rng = np.random.default_rng(7 * V + bs)
    raw = _logits(rng, bs, V, dtype, 2.0)
    raw[:, rng.integers(0, V, max(1, V // 50))] = np.nan
    params = [dict(CASES[(b + V) % len(CASES)], seed=1000 + 17 * b) for b in range(bs)]
    stride = 16
    hist = rng.integers(0, V, (bs, stride)).astype(np.int32)
    hlen = rng.integers(0, stride, bs).astype(np.int32)
    st = State(bs, stride, (hist, hlen))
    seq0 = st.seq.cpu().numpy()
    step = 77
    got = run(llmie, _dev(raw, dtype), params, step, st, append=True)
    bad = _check_rows(got, raw, params, None, step, st.lp.cpu().numpy())
    ok = np.setdiff1d(np.arange(bs), bad)
    assert np.array_equal(st.seq.cpu().numpy()[ok], seq0[ok] + 1)
    assert np.array_equal(st.fin.cpu().numpy()[ok].astype(bool), got[ok] == END)
    h2, l2 = st.hist.cpu().numpy(), st.hlen.cpu().numpy()
    assert np.array_equal(l2, hlen + 1)
    for b in ok:
        assert h2[b, hlen[b]] == got[b] and np.array_equal(h2[b, :hlen[b]], hist[b, :hlen[b]])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [1000, 32000, 128256])
def test_penalties(llmie, dtype, V):
    rng = np.random.default_rng(V)
    bs, stride = 24, 64
    raw = _logits(rng, bs, V, dtype, 0.5)
    hist = np.empty((bs, stride), np.int32)
    hlen = np.empty(bs, np.int32)
    pens = [dict(repetition_penalty=1.8), dict(presence_penalty=0.7), dict(frequency_penalty=0.4),
            dict(repetition_penalty=1.3, presence_penalty=0.2, frequency_penalty=0.3), dict(repetition_penalty=0.6)]
    params = []
    for b in range(bs):
        top = np.argsort(-raw[b])[:8]   # the history names the leading tokens, with duplicates
        h = rng.choice(top, stride)
        h[rng.random(stride) < 0.2] = rng.choice([-1, -100, V, V + 5])   # ids outside [0, V): ignored
        hist[b] = h
        hlen[b] = [0, stride, 1, 7, 40][b % 5]
        params.append(dict(pens[b % len(pens)], temperature=0.0))
    st = State(bs, stride, (hist, hlen))
    got = run(llmie, _dev(raw, dtype), params, 5, st, append=True)
    for b in range(bs):
        pick, _, _ = ref_row(raw[b], params[b], hist[b, :hlen[b]], 5)
        assert got[b] == pick, "row %d (%s, history %d)" % (b, params[b], hlen[b])
    l2 = st.hlen.cpu().numpy()
    h2 = st.hist.cpu().numpy()
    assert np.array_equal(l2, np.minimum(hlen + 1, stride))   # a full stride is not appended past
    for b in range(bs):
        if hlen[b] < stride:
            assert h2[b, hlen[b]] == got[b]
        else:
            assert np.array_equal(h2[b], hist[b])
    # penalties change the pick: with them off the argmax of the raw row comes back
    st0 = State(bs)
    got0 = run(llmie, _dev(raw, dtype), [dict(temperature=0.0)] * bs, 5, st0)
    assert np.array_equal(got0, np.argmax(raw, axis=1))
    assert (got0 != got).any()


def test_distribution(llmie):
    bs, V = 20000, 100
    rng = np.random.default_rng(9)
    row = _logits(rng, 1, V, torch.float32, 1.5)[0]
    raw = np.tile(row, (bs, 1))
    T, top_p = 0.8, 0.9
    params = [dict(temperature=T, top_p=top_p, seed=b * 7919 + 1) for b in range(bs)]
    st = State(bs)
    got = run(llmie, _dev(raw), params, 3, st)
    v = (row / np.float32(T)).astype(np.float64)
    order = np.lexsort((np.arange(V), -v))
    p = np.exp(v[order] - v[order[0]])
    cum = np.cumsum(p)
    i = int(np.searchsorted(cum, top_p * cum[-1]))
    keep = v[order] >= v[order[i]]
    q = np.zeros(V)
    q[order[keep]] = p[keep] / p[keep].sum()
    freq = np.bincount(got, minlength=V)[:V] / bs
    assert (freq[q == 0] == 0).all()
    assert np.abs(freq - q).max() < 0.015


def _mixed(bs, V, rng):
    params = [dict(CASES[b % len(CASES)], seed=int(rng.integers(0, 2**32)),
                   repetition_penalty=[1.0, 1.2][b % 2], frequency_penalty=[0.0, 0.1][b % 3 == 0]) for b in range(bs)]
    params[3] = dict(temperature=0.0)
    return params


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [1000, 32000])
def test_determinism_and_batch_invariance(llmie, dtype, V):
    rng = np.random.default_rng(1)
    bs, stride = 64, 32
    raw = _logits(rng, bs, V, dtype, 2.0)
    params = _mixed(bs, V, rng)
    hist = rng.integers(0, V, (bs, stride)).astype(np.int32)
    hlen = rng.integers(0, stride, bs).astype(np.int32)
    logits = _dev(raw, dtype)
    outs = []
    for _ in range(2):
        st = State(bs, stride, (hist, hlen))
        outs.append((run(llmie, logits, params, 99, st, append=True), st.lp.cpu().numpy().copy(), st.hist.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32))
    assert np.array_equal(outs[0][2], outs[1][2])
    for b in (0, 3, 17, 63):
        st = State(1, stride, (hist[b:b + 1], hlen[b:b + 1]))
        g = run(llmie, logits[b:b + 1].contiguous(), [params[b]], 99, st, append=True)
        assert g[0] == outs[0][0][b]
        assert st.lp.cpu().numpy().view(np.uint32)[0] == outs[0][1].view(np.uint32)[b]


def test_clamping(llmie):
    rng = np.random.default_rng(2)
    V = 1000
    wild = [dict(temperature=-1.0), dict(temperature=float("nan")), dict(top_k=-5, top_p=0.7, seed=4),
            dict(top_k=5 * V, seed=5), dict(top_p=0.0, temperature=1.5, seed=6), dict(top_p=-2.0, seed=7),
            dict(top_p=3.0, seed=8), dict(min_p=-0.5, seed=9), dict(min_p=7.0, seed=10),
            dict(repetition_penalty=0.0, temperature=0.0), dict(repetition_penalty=float("nan"), temperature=0.0),
            dict(repetition_penalty=-3.0, temperature=0.0)]
    tame = [dict(temperature=0.0), dict(temperature=0.0), dict(top_k=0, top_p=0.7, seed=4), dict(top_k=V, seed=5),
            dict(top_k=1, temperature=1.5, seed=6), dict(top_k=1, seed=7), dict(top_p=1.0, seed=8), dict(min_p=0.0, seed=9),
            dict(min_p=1.0, seed=10), dict(repetition_penalty=1.0, temperature=0.0),
            dict(repetition_penalty=1.0, temperature=0.0), dict(repetition_penalty=1.0, temperature=0.0)]
    bs = len(wild)
    raw = _logits(rng, bs, V, torch.float32)
    hist = np.tile(np.argsort(-raw, axis=1)[:, :4].astype(np.int32), (1, 2))
    hlen = np.full(bs, 8, np.int32)
    logits = _dev(raw)
    a = run(llmie, logits, wild, 21, State(bs, 8, (hist, hlen)))
    b = run(llmie, logits, tame, 21, State(bs, 8, (hist, hlen)))
    assert np.array_equal(a, b)
    assert a[5] == np.argmax(raw[5]) and a[0] == np.argmax(raw[0])


# --------------------------------------------------------------------------- decoder entry
def _decoder(llmie, dtype, V, bs):
    rng = np.random.default_rng(4)
    nh, hs, inter = 4, 32, 344
    H = nh * hs
    f = np.float16 if dtype == torch.float16 else np.float32

    def mk(shape, scale):
        return _dev((rng.uniform(-1, 1, shape) * scale).astype(f))

    layers = [dict(attn_norm=mk((H,), 0.1) + 1, ffn_norm=mk((H,), 0.1) + 1, qkv=mk((3 * H, H), 0.1), o=mk((H, H), 0.1),
                   gate_up=mk((2 * inter, H), 0.1), down=mk((H, inter), 0.1))]
    cfg = dict(head_num=nh, kv_head_num=nh, head_size=hs, inter_size=inter, num_layers=1, vocab_size=V, max_seq_len=16,
               max_batch=bs, rotary_dim=hs, rotary_base=10000.0, rms_eps=1e-5,
               dtype=llmie.F16 if dtype == torch.float16 else llmie.F32,
               wfmt=llmie.W_F16 if dtype == torch.float16 else llmie.W_F32, int4_group=128)
    dec = llmie.Decoder(cfg, layers)
    return dec, mk((bs, H), 1.0), mk((H,), 0.1) + 1, mk((V, H), 0.3), mk((V, H), 1.0)


@pytest.mark.parametrize("dtype,fmt", [(torch.float16, "W_F16"), (torch.float32, "W_F32")])
def test_lm_head_sample_params(llmie, dtype, fmt):
    V, bs, stride = 32000, 4, 8
    dec, x, gam, lm, _ = _decoder(llmie, dtype, V, bs)
    rng = np.random.default_rng(6)
    params = [dict(temperature=0.9, top_p=0.95, seed=3), dict(temperature=0.0, repetition_penalty=1.5),
              dict(top_k=40, min_p=0.05, seed=8), dict(temperature=1.2, presence_penalty=0.5, frequency_penalty=0.2, seed=1)]
    hist = rng.integers(0, V, (bs, stride)).astype(np.int32)
    hlen = np.array([0, 3, 5, 8], np.int32)
    pd = llmie.sampling_params(params)
    logits = torch.empty((bs, V), dtype=dtype, device=DEV)
    st = State(bs, stride, (hist, hlen))
    dec.lm_head_sample_params(x.clone(), gam, lm, getattr(llmie, fmt), logits, pd, st.seq, st.fin, st.out, 41, END,
                              history=st.hist, history_len=st.hlen, append=True, out_logprob=st.lp)
    torch.cuda.synchronize()
    # the sampler on the logits the entry produced (and they are llmie_linear's logits of the normalised rows)
    st2 = State(bs, stride, (hist, hlen))
    llmie.sample_logits(logits, pd, st2.seq, st2.fin, st2.out, 41, END, history=st2.hist, history_len=st2.hlen, append=True,
                        out_logprob=st2.lp)
    xn = x.float()
    xn = (xn * torch.rsqrt(xn.pow(2).mean(-1, keepdim=True) + 1e-5) * gam.float()).to(dtype)
    ref = torch.empty_like(logits)
    llmie.linear(xn, lm, ref)
    torch.cuda.synchronize()
    tol = 2e-2 if dtype == torch.float16 else 1e-3
    assert (logits.float() - ref.float()).abs().max().item() <= tol * max(1.0, ref.float().abs().max().item())
    assert torch.equal(st.out, st2.out) and torch.equal(st.hist, st2.hist) and torch.equal(st.lp, st2.lp)
    assert torch.equal(st.seq, st2.seq) and torch.equal(st.fin, st2.fin)
    dec.close()


def test_lm_head_sample_params_graph(llmie):
    dtype, V, stride, n = torch.float16, 32000, 16, 8
    dec, x, gam, lm, emb = _decoder(llmie, dtype, V, 1)
    H = x.shape[1]
    params = [dict(temperature=0.8, top_p=0.9, repetition_penalty=1.3, seed=12345)]
    pd = llmie.sampling_params(params)
    ws = torch.empty(llmie.sample_logits_workspace_bytes(1, V), dtype=torch.uint8, device=DEV)
    logits = torch.empty((1, V), dtype=dtype, device=DEV)
    hid = torch.empty_like(x)
    nxt = torch.empty_like(x)
    st = State(1, stride, (np.zeros((1, stride), np.int32), np.zeros(1, np.int32)))
    step_dev = torch.zeros(1, dtype=torch.int32, device=DEV)

    def one():
        hid.copy_(x + 0.05 * nxt)   # the next step's input depends on the last pick
        dec.lm_head_sample_params(hid, gam, lm, llmie.W_F16, logits, pd, st.seq, st.fin, st.out, -1, END, history=st.hist,
                                  history_len=st.hlen, append=True, out_logprob=st.lp, step_dev=step_dev, embed=emb,
                                  next_hidden=nxt, advance=True, workspace=ws)

    def reset(step0):
        st.hist.zero_()
        st.hlen.zero_()
        st.seq.zero_()
        st.fin.zero_()
        nxt.zero_()
        step_dev.fill_(step0)

    reset(100)
    eager = []
    for _ in range(n):
        one()
        eager.append((int(st.out.item()), nxt.clone(), float(st.lp.item())))
    assert int(step_dev.item()) == 100 + n
    assert st.hist.cpu().numpy()[0, :n].tolist() == [e[0] for e in eager]

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        reset(100)
        one()   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        one()
    reset(100)
    torch.cuda.synchronize()
    for i in range(n):
        g.replay()
        torch.cuda.synchronize()
        assert int(st.out.item()) == eager[i][0], "replay %d" % i
        assert torch.equal(nxt, eager[i][1]) and float(st.lp.item()) == eager[i][2]
    assert int(step_dev.item()) == 100 + n
    # new device parameters take effect on the next replay: greedy gives the penalised argmax of the logits it computed
    llmie.sampling_params([dict(temperature=0.0)], out=pd)
    g.replay()
    torch.cuda.synchronize()
    assert int(st.out.item()) == int(torch.argmax(logits.float()).item())
    assert torch.equal(nxt[0], emb[int(st.out.item())])
    dec.close()
