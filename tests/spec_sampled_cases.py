"""llmie_spec_verify_sampled restated in numpy and Python integers, one sequence at a time (no GPU, no library).

sampler_row restates the sampler of include/llmie.h on one row and hands out what the verify rule needs: the fixed-point masses
M_v = floor(exp(v - max) * 2^32) of the kept tokens (float64 exp; 0 for a token not kept), their sum S, and the sampler's own
pick (the lane-0 draw).  A greedy row, or one with at most one valid token, is the point mass M_pick = S = 1; a row without a
valid token has M = 0, S = 0 and picks end_id.  verify_sequence walks the positions of one sequence by the header's rule, every
product and comparison in Python integers.

The device forms its masses with fp32 expf, so a decision may differ where it sits on a boundary.  A sequence is reported
FRAGILE when any decision on its walk does, with TIE = 1e-5 (the value tests/test_sampling_params_gpu.py uses): the inner
sampler's own boundaries (the top-p cut, the min-p cut, the draw), |(U1 - 1) / 2^24 - p_d / q_d| < TIE, or a residual cumulative
within TIE * SR of thr."""
import numpy as np

TIE = 1e-5
FLT_MAX = np.float32(np.finfo(np.float32).max)
M32 = 0xffffffff
ONE = 1 << 32


def philox(seed, stream, lane=0):
    """Philox4x32-10 with key (seed, 0x4c4c4d49) on the counter (stream, lane, 0, 0): the 24-bit integer U = (c0 >> 8) + 1 in
    [1, 2^24].  Lane 0 is the sampler's draw (u = U / 2^24), lane 1 the accept draw, lane 2 the residual draw."""
    c0, c1, c2, c3 = stream & M32, lane & M32, 0, 0
    k0, k1 = seed & M32, 0x4c4c4d49
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return (c0 >> 8) + 1


def philox_many(seed, streams, lane=0):
    """philox(seed, s, lane) for an array of streams, in numpy uint64"""
    c0 = np.asarray(streams, np.uint64) & np.uint64(M32)
    c1, c2, c3 = np.full_like(c0, lane), np.zeros_like(c0), np.zeros_like(c0)
    k0, k1 = seed & M32, 0x4c4c4d49
    m = np.uint64(M32)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return (c0 >> np.uint64(8)) + np.uint64(1)


def clamp(p, V):
    p = dict(dict(temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, repetition_penalty=1.0, presence_penalty=0.0,
                  frequency_penalty=0.0, seed=0), **p)
    f32 = lambda v: float(np.float32(v))
    t = f32(p["temperature"])
    t = t if t >= 0 else 0.0
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
                frequency=f32(p["frequency_penalty"]), seed=int(p["seed"]) & M32)


class Row:
    """M: uint64 [V] masses (0: not kept); S: their sum (int); pick: the sampler's own token; valid: any valid token;
    fragile_cut / fragile_draw: the kept set / the lane-0 draw sits on a boundary; lse: raw log-sum-exp (None: no finite logit)"""


def sampler_row(raw, p, hist, step, end_id, ctl=None):
    """raw: the fp32 values the device reads.  ctl: None or dict(mask=bool [V] or None, bias=[(id, val)], stops=[ids],
    min_step=int or None) -- the extension as it applies to this row."""
    V = raw.size
    c = clamp(p, V)
    raw = raw.astype(np.float32)
    l = raw.copy()
    r = Row()
    rv = raw.astype(np.float64)[~np.isnan(raw)]
    with np.errstate(all="ignore"):
        r.lse = float(rv.max() + np.log(np.exp(rv - rv.max()).sum())) if rv.size else None
    if ctl:
        last = {}
        for t, v in ctl.get("bias") or []:
            if 0 <= t < V and not np.isnan(v) and v != np.inf:
                last[t] = np.float32(v)
        for t, v in last.items():
            l[t] = np.nan if v == -np.inf else np.float32(l[t] + v)
        if ctl.get("min_step") is not None and step < ctl["min_step"]:
            for t in list(ctl.get("stops") or []) + [end_id]:
                if 0 <= t < V:
                    l[t] = np.nan
    h = np.asarray(hist, np.int64)
    h = h[(h >= 0) & (h < V)]
    if h.size and (c["rep"] != 1 or c["presence"] != 0 or c["frequency"] != 0):
        ids, cnt = np.unique(h, return_counts=True)
        x = l[ids]
        with np.errstate(all="ignore"):
            x = np.where(x > 0, x / np.float32(c["rep"]), x * np.float32(c["rep"])).astype(np.float32)
            x = (x - np.float32(c["presence"])).astype(np.float32)
            x = (x - cnt.astype(np.float32) * np.float32(c["frequency"])).astype(np.float32)
        l[ids] = x
    if ctl and ctl.get("mask") is not None:
        l[~np.asarray(ctl["mask"], bool)] = np.nan
    valid = ~np.isnan(l)
    r.M = np.zeros(V, np.uint64)
    r.S, r.pick, r.valid, r.fragile_cut, r.fragile_draw = 0, end_id, bool(valid.any()), False, False
    if not r.valid:
        return r
    ids = np.nonzero(valid)[0]
    if c["temperature"] == 0 or ids.size <= 1:
        vals = np.where(valid, l, -np.inf)
        r.pick = int(np.nonzero(valid & (vals == vals.max()))[0][0])
        r.M[r.pick], r.S = 1, 1
        return r
    with np.errstate(all="ignore"):
        v = np.clip((l / np.float32(c["temperature"])).astype(np.float32), -FLT_MAX, FLT_MAX)
    order = ids[np.lexsort((ids, -v[ids]))]
    vo = v[order].astype(np.float64)
    mass = np.exp(vo - vo[0])
    n = order.size
    if 0 < c["top_k"] < n:
        n = c["top_k"]
    if c["top_p"] < 1:
        cum = np.cumsum(mass[:n])
        tgt = c["top_p"] * cum[-1]
        i = min(int(np.searchsorted(cum, tgt, side="left")), n - 1)
        r.fragile_cut |= bool(np.min(np.abs(cum - tgt)) < TIE * cum[-1])
        n = int(np.count_nonzero(vo[:n] >= vo[i]))
    if c["min_p"] > 0:
        r.fragile_cut |= bool(np.min(np.abs(mass[:n] - c["min_p"])) < TIE)
        n = int(np.count_nonzero(mass[:n] >= c["min_p"]))
    fixed = np.floor(mass[:n] * float(ONE)).astype(np.uint64)
    r.M[order[:n]] = fixed
    r.S = int(fixed.astype(object).sum())
    cum = np.cumsum(mass[:n])
    tgt = philox(step, c["seed"], 0) / 16777216.0 * cum[-1]
    j = min(int(np.searchsorted(cum, tgt, side="right")), n - 1)
    r.fragile_draw = bool(np.min(np.abs(cum - tgt)) < TIE * cum[-1])
    r.pick = int(order[j])
    return r


def history_view(hist, hlen0, hstride, append, drafts, i):
    """the penalty history of position i: the stored history, then the drafts in front of i as far as i appends reach"""
    if hstride <= 0:
        return []
    stored = min(max(hlen0, 0), hstride)
    length = min(stored + i, hstride) if (append and hlen0 >= 0) else stored
    return list(hist[:stored]) + list(drafts[:length - stored])


def decide(P, Q, d, step, seed):
    """the rule at one position with a draft: -> (accepted, residual token or None when SR == 0, fragile)"""
    V = P.M.size
    SP, SQ = P.S, Q.S
    fragile = P.fragile_cut or Q.fragile_cut
    acc = False
    if 0 <= d < V:
        Pd, Qd = int(P.M[d]), int(Q.M[d])
        u1 = philox(step, seed, 1) - 1
        acc = u1 * Qd * SP < (1 << 24) * Pd * SQ
        if Pd and Qd and SQ and SP:
            fragile |= abs(u1 / 16777216.0 - (Pd * SQ) / (Qd * SP)) < TIE
    if acc:
        return True, None, fragile
    res, run = None, 0
    idx = np.nonzero(P.M)[0]   # ascending ids; R_v > 0 needs P_v > 0
    R = [max(0, int(P.M[t]) * SQ - int(Q.M[t]) * SP) for t in idx]
    SR = sum(R)
    if SR > 0:
        thr = ((philox(step, seed, 2) - 1) * SR) >> 24
        for t, w in zip(idx, R):
            run += w
            if res is None and run > thr:
                res = int(t)
            if w and run < SR and abs(run - thr) < TIE * SR:   # a boundary between two residual tokens next to thr
                fragile = True
    return False, res, fragile


def verify_sequence(raw_t, raw_d, drafts, m, p, dp, hist, hlen0, hstride, append, step0, end_id, ctl=None, finished=False):
    """raw_t [k + 1, V], raw_d [k, V] (fp32 as read), drafts [k]; ctl: None or dict(masks=[k + 1 rows of bool [V] or None] or
    None, bias, stops, min_step) of this sequence.  -> dict(tokens, logprob, count, accepted, fin, hist, hlen, fragile)"""
    k = len(drafts)
    n = k + 1
    out = dict(tokens=[-1] * n, logprob=[-np.inf] * n, count=0, accepted=0, fin=int(bool(finished)), hist=list(hist), hlen=hlen0,
               fragile=False)
    if finished:
        return out
    m = k if m is None else min(max(int(m), 0), k)
    stops = list((ctl or {}).get("stops") or [])
    seed = clamp(p, raw_t.shape[1])["seed"]
    hl = hlen0 if (append and hstride > 0) else -1
    for i in range(n):
        view = history_view(hist, hlen0, hstride, append, drafts, i)
        rc = None
        if ctl:
            rc = dict(bias=ctl.get("bias"), stops=stops, min_step=ctl.get("min_step"),
                      mask=None if ctl.get("masks") is None else ctl["masks"][i])
        P = sampler_row(raw_t[i], p, view, step0 + i, end_id, rc)
        go_on = False
        if i < m:
            Q = sampler_row(raw_d[i], dp, view, step0 + i, end_id, None)
            acc, res, fr = decide(P, Q, int(drafts[i]), step0 + i, seed)
            out["fragile"] |= bool(fr)
            if acc:
                tok, go_on = int(drafts[i]), True
                out["accepted"] += 1
            elif res is not None:
                tok = res
            else:
                tok = P.pick
                out["fragile"] |= P.fragile_draw
        else:
            tok = P.pick
            out["fragile"] |= P.fragile_cut or P.fragile_draw
        fin = tok == end_id or tok in stops
        out["tokens"][i] = tok
        out["logprob"][i] = float(raw_t[i][tok]) - P.lse if (0 <= tok < raw_t.shape[1] and P.valid and P.lse is not None) else -np.inf
        out["count"] += 1
        out["fin"] = int(fin)
        if 0 <= hl < hstride:
            out["hist"][hl] = tok
            hl += 1
        if fin or not go_on:
            break
    if append and hstride > 0 and hl >= 0:
        out["hlen"] = hl
    return out


def draw_drafts(raw_d, dp, hist, hlen0, hstride, append, step0, end_id):
    """the caller's side of the contract: draft i is the sampler's pick from raw_d[i] with dp at step step0 + i on the history
    view of position i.  -> (drafts, fragile)"""
    k = raw_d.shape[0]
    drafts, fragile = [], False
    for i in range(k):
        q = sampler_row(raw_d[i], dp, history_view(hist, hlen0, hstride, append, drafts, i), step0 + i, end_id)
        drafts.append(q.pick)
        fragile |= q.fragile_cut or q.fragile_draw
    return np.array(drafts, np.int32), fragile


# ------------------------------------------------------------------------------------------------ the cases of the GPU test
# (numpy only: tests/test_spec_sampled_cpu.py checks the restatement's fragile share of every case without a GPU)
END, STRIDE = 2, 24
STEPS = [3, 100, 7, 1 << 20, 55]
# The parameter mixes: the CASES of tests/test_sampling_params_gpu.py that cut the tail off (by index; top_p = 0.99 and the bare
# temperature 1.7 are left out).  With TIE = 1e-5 a draw that lands among thousands of kept tail tokens of mass < 1e-5 each
# is "on a boundary" by definition, whatever the device does, and the fragile share could not stay under the cap.
TRUNC = [0, 1, 3, 4, 5, 7, 8, 9, 10]


def fragile_cap(sequences):
    return max(1, int(0.004 * sequences))


class Case:
    """one call: B sequences of k drafts over V tokens.  raw_t [B, k + 1, V] / raw_d [B, k, V]: fp32 values as the device reads
    them (rounded through fp16 for an fp16 case); ctl: per sequence None or verify_sequence's dict; mask rows / index for ext."""

    def expected(self):
        if getattr(self, "_want", None) is None:
            self._want = [verify_sequence(self.raw_t[b], self.raw_d[b], self.drafts[b], None if self.draft_len is None else self.draft_len[b],
                                          self.params[b], self.dparams[b], self.hist[b], int(self.hlen[b]), STRIDE, self.append,
                                          int(self.steps[b]), END, self.ctl[b] if self.ctl else None, bool(self.fin[b]))
                          for b in range(self.B)]
        return self._want


def sampler_cases():
    from test_sampling_params_gpu import CASES
    return [dict(CASES[i]) for i in TRUNC]


def mixed_params(B, case, kind="mixed"):
    """(target, draft) parameter rows: mixes drawn independently for target and draft, penalties on every other sequence"""
    cs = sampler_cases()
    tp, dp = [], []
    for b in range(B):
        pen = dict(repetition_penalty=1.2, frequency_penalty=0.1, presence_penalty=0.2) if b % 2 else {}
        t = dict(cs[(case + b) % len(cs)], seed=1000 + 17 * b + case, **pen)
        d = dict(cs[(3 * case + 2 * b + 1) % len(cs)], seed=5000 + 31 * b + case, **pen)
        if kind in ("greedy_target", "both_greedy"):
            t = dict(temperature=0.0, **pen)
        if kind in ("greedy_draft", "both_greedy"):
            d = dict(temperature=0.0, **pen)
        tp.append(t)
        dp.append(d)
    return tp, dp


def make_logits(rng, B, k, V, f16):
    """target [B, k + 1, V] and draft [B, k, V] rows.  V >= 1000: a handful of tokens carries almost all the mass (a model that
    knows what comes next), so that the cuts and the draws fall among tokens far wider than TIE; the draft is the target plus
    noise, so that p / q scatters around 1 and both outcomes occur.  The logit of END is -30: no walk is cut short by chance."""
    if V < 100:
        t = (rng.standard_normal((B, k + 1, V)) * 2.0).astype(np.float32)
    else:
        t = rng.standard_normal((B, k + 1, V)).astype(np.float32)
        for b in range(B):
            for i in range(k + 1):
                big = rng.choice(np.arange(3, V), 6, replace=False)
                t[b, i, big] += (16.0 + 1.5 * rng.standard_normal(6)).astype(np.float32)
    d = t[:, :k] + (rng.standard_normal((B, k, V)) * 0.5).astype(np.float32)
    if V > END:
        t[:, :, END] = -30.0
        d[:, :, END] = -30.0
    if f16:
        t, d = t.astype(np.float16).astype(np.float32), d.astype(np.float16).astype(np.float32)
    return t, d


def make_case(seed, V, B, k, f16, kind="mixed", append=True, hlen=None, finalize=True):
    rng = np.random.default_rng(seed)
    c = Case()
    c.V, c.B, c.k, c.f16, c.append = V, B, k, f16, append
    c.raw_t, c.raw_d = make_logits(rng, B, k, V, f16)
    c.params, c.dparams = mixed_params(B, seed, kind)
    hist = rng.integers(0, V, (B, STRIDE)).astype(np.int32)
    hist[:, 1], hist[:, 3] = -1, V + 3          # ids outside [0, V) are ignored
    c.hist = hist
    c.hlen = np.array([5, 0, 11, STRIDE // 2, 9][:B] if hlen is None else hlen, np.int32)
    c.steps = np.array(STEPS[:B], np.int32)
    c.seq = np.array([10, 0, 7, 300, 1][:B], np.int32)
    c.cached = np.array([120, 5, 77, 2000, 128][:B], np.int32)
    c.fin = np.zeros(B, np.uint8)
    c.draft_len, c.ctl, c.masks, c.mask_index, c.top_n = None, None, None, None, 0
    c.shared_step = None
    if finalize:
        draw(c)
    return c


def draw(c):
    """the drafter's side: every draft is the restated sampler's pick from its draft row (the caller contract)"""
    c.drafts = np.zeros((c.B, c.k), np.int32)
    c.draft_fragile = np.zeros(c.B, bool)
    for b in range(c.B):
        c.drafts[b], c.draft_fragile[b] = draw_drafts(c.raw_d[b], c.dparams[b], c.hist[b], int(c.hlen[b]), STRIDE, c.append, int(c.steps[b]), END)
    c._want = None
    return c


SHAPES = [(V, B, k, f16) for V in (7, 1000, 32003) for B in (1, 5) for k in (1, 4, 15) for f16 in (True, False)]
KINDS = ["greedy_target", "greedy_draft", "both_greedy"]


def matrix():
    """(id, builder) of every restated case the GPU test runs"""
    out = []
    for n, (V, B, k, f16) in enumerate(SHAPES):
        out.append(("V%d-B%d-k%d-%s" % (V, B, k, "f16" if f16 else "f32"), lambda n=n, s=(V, B, k, f16): make_case(100 + n, *s)))
    for j, kind in enumerate(KINDS):
        for f16 in (True, False):
            out.append(("%s-%s" % (kind, "f16" if f16 else "f32"), lambda j=j, kind=kind, f16=f16: make_case(300 + 2 * j + f16, 1000, 5, 4, f16, kind)))
    out += [(name, fn) for name, fn in SPECIAL.items()]
    return out


def _draft_len_case():
    c = make_case(400, 1000, 5, 4, True)
    c.draft_len = [0, 1, 4, -3, 13]     # 0, short of k, k, and values the device clamps
    c._want = None
    return c


def _out_of_range_case():
    c = make_case(401, 1000, 5, 4, False)
    c.drafts[0, 0], c.drafts[1, 1], c.drafts[2, 0], c.drafts[3, 3] = -1, c.V, c.V + 7, -(1 << 31)
    c._want = None
    return c


def _stops_case():
    # an accepted draft that is end_id (sequence 0) or a stop id (sequence 1) ends the walk behind it; 500 is no stop of sequence 2
    c = make_case(402, 1000, 3, 4, False, finalize=False)
    for b, i, t in ((0, 1, END), (1, 2, 500), (2, 3, 500)):
        c.raw_t[b, i, t] = c.raw_d[b, i, t] = 60.0
    c.ctl = [dict(stops=[]), dict(stops=[9, 500]), dict(stops=[501])]
    return draw(c)


def _min_step_case():
    c = make_case(403, 1000, 2, 4, True, finalize=False)
    c.raw_t[:, :, END] = 40.0            # end_id wins in the target wherever it is allowed ...
    c.raw_t[1, :, 77] = 41.0             # ... and sequence 1's stop id above it
    c.raw_d[0, 0] = c.raw_t[0, 0]        # (position 0 of sequence 0: P == Q but for the banned end_id -- accepted)
    c.raw_d[0, 0, END] = -30.0
    c.raw_d[0, 1:, END] = 40.0           # the drafter (no extension) names them: one step early (P_d = 0: rejected) or in time
    c.raw_d[1, 3:, 77] = 41.0
    c.steps = np.array([10, 20], np.int32)
    c.ctl = [dict(stops=[], min_step=12), dict(stops=[77], min_step=23)]   # held back at steps 10, 11 / 20, 21, 22: P_d = 0 there
    return draw(c)


def _mask_case():
    # per-position masks: rows 0 .. R - 1 ban the draft of their position (P_d = 0: rejected), row R allows everything
    c = make_case(404, 1000, 2, 4, True)
    R = c.B * (c.k + 1)
    c.masks = np.ones((R + 1, c.V), bool)
    c.mask_index = [R] * R
    for b, i in ((0, 2), (1, 0)):
        r = b * (c.k + 1) + i
        c.masks[r, c.drafts[b, i]] = False
        c.masks[r, ::2] &= (np.arange(0, c.V, 2) % 3 != 0)
        c.mask_index[r] = r
    c.mask_index[3] = -1                                # one position unconstrained
    c.ctl = [dict(masks=[c.masks[c.mask_index[b * (c.k + 1) + i]] if c.mask_index[b * (c.k + 1) + i] >= 0 else None
                         for i in range(c.k + 1)]) for b in range(c.B)]
    c._want = None
    return c


def _bias_case():
    c = make_case(405, 1000, 2, 4, False)
    ban = int(c.drafts[0, 1])
    c.ctl = [dict(bias=[(ban, float("-inf")), (5, 1.5)]), dict(bias=[(7, -2.0), (int(c.drafts[1, 0]), 3.0)])]
    c._want = None
    return c


def _saturate_case(append):
    # histories within the chunk's reach of the stride: the appends saturate inside the chunk, and one is full on entry
    c = make_case(406 + append, 1000, 5, 4, True, append=bool(append), hlen=[STRIDE - 2, STRIDE, STRIDE - 1, STRIDE - 4, 0], finalize=False)
    for b in range(c.B):
        c.params[b].update(repetition_penalty=1.5, presence_penalty=0.4, frequency_penalty=0.3)
        c.dparams[b].update(repetition_penalty=1.5, presence_penalty=0.4, frequency_penalty=0.3)
    return draw(c)


def _finished_case():
    c = make_case(408, 1000, 3, 4, True)
    c.fin[1] = 1
    c._want = None
    return c


def _nan_case():
    c = make_case(409, 1000, 4, 4, True, finalize=False)
    c.raw_t[0, 1, ::3] = np.nan          # a third of a target row
    c.raw_t[1, 2, :] = np.nan            # a whole target row: always rejected, emits end_id and finishes
    c.raw_d[2, 0], c.dparams[2] = c.raw_t[2, 0], dict(c.params[2], seed=777)   # (P == Q: position 0 is accepted)
    c.raw_d[2, 1, :] = np.nan            # a whole draft row: S_Q = 0, the draft (end_id) is rejected, the pick is emitted
    c.raw_d[3, 0, 5:900] = np.nan
    return draw(c)


def _top_n_case():
    c = make_case(410, 1000, 5, 4, True)
    c.fin[4] = 1
    c.top_n = 5
    c._want = None
    return c


def _shared_step_case():
    c = make_case(411, 1000, 5, 4, True, finalize=False)
    c.shared_step = 41
    c.steps = np.full(c.B, 41, np.int32)
    return draw(c)


SPECIAL = {"draft_len": _draft_len_case, "draft_out_of_range": _out_of_range_case, "stops": _stops_case, "min_step": _min_step_case,
           "mask_bans_draft": _mask_case, "bias_ban": _bias_case, "saturate_keep": lambda: _saturate_case(0),
           "saturate_append": lambda: _saturate_case(1), "finished": _finished_case, "nan_rows": _nan_case, "top_n": _top_n_case,
           "shared_step": _shared_step_case}
