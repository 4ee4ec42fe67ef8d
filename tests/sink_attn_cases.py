"""Attention cases with a learned sink logit per query head ("head sink", include/llmie.h): one generator shared by
tests/test_sink_cases_cpu.py (the tests of the tests), tests/test_sink_decode_gpu.py and tests/test_sink_prefill_gpu.py.  Plain
module, no fixtures; builds on tests/attn_cases.py, tests/window_attn_cases.py and tests/prefill_attn_cases.py.

The softmax of query head h runs over the keys the mask exposes (causal; window + sink TOKENS where set) and one extra column with
logit s_h and no value row:

    M = max(max_j l_j, s_h),   out = sum_j exp(l_j - M) v_j / (sum_j exp(l_j - M) + exp(s_h - M) + 1e-6)

As in the modules this builds on, every (sequence, query head) owns one cache position whose K row gives logit 12 over a +-0.5
background and holds >= 0.9 of the mass AMONG THE REAL KEYS; windowed cases keep their dominating rows just outside the mask.  The
query heads' sink logits cycle through five classes, placed relative to that planted logit:

    ninf        -inf: no sink for this head (the bits of the call without a head sink)
    negligible  12 - 8:   share of the total mass <= 1e-3
    half        12:       share in [0.3, 0.7]
    dominant    12 + 2.5: share >= 0.9
    above       12 + 8:   larger than every real logit (M = s), share >= 0.999

The shares are asserted by the generator from the float64 reference wherever a head owns a planted row: conditions on the inputs, not
measurements.  Consecutive heads take consecutive classes (from `shift`), so the heads of one KV group fall into different classes
(ratio 8: no two neighbours alike) and a sink taken from the wrong head of a group is an O(0.1) error.

Reference: float64 restatement of the formula on the inputs as rounded to fp16; for an e4m3 cache on the de-quantised bytes.
"""
import functools

import numpy as np

import attn_cases as ac
import window_attn_cases as wc

F16 = ac.F16
KV_PAGE = ac.KV_PAGE
KVH = wc.KVH
LOGIT = 12.0
CLASSES = ("ninf", "negligible", "half", "dominant", "above")
OFFSET = {"ninf": -np.inf, "negligible": -8.0, "half": 0.0, "dominant": 2.5, "above": 8.0}
SHARE = {"ninf": (0.0, 0.0), "negligible": (0.0, 1e-3), "half": (0.3, 0.7), "dominant": (0.9, 1.0), "above": (0.999, 1.0)}
DEFECTS = ("missing", "per_split", "per_lane", "group_div", "group_mod", "before_mask", "no_max", "as_key")


def sink_classes(nh, shift):
    return [CLASSES[(h + shift) % len(CLASSES)] for h in range(nh)]


def sink_values(nh, shift, logit=LOGIT):
    """float32 [nh]: the sink logit of every query head, and the class names"""
    names = sink_classes(nh, shift)
    return np.array([logit + OFFSET[n] for n in names], np.float32), names


# ------------------------------------------------------------------------------------------------------------------ decode
@functools.lru_cache(maxsize=4)
def _background(hs, bs, max_seq, e4m3, seed):
    rng = np.random.default_rng([seed, hs, bs, max_seq, int(e4m3)])
    shape = (1, bs, KVH, max_seq, hs)
    if e4m3:
        codes = lambda: rng.integers(0, 0x58, shape, dtype=np.uint8) | (rng.integers(0, 2, shape, dtype=np.uint8) << 7)
        return codes(), codes()
    return (ac.rnd_t(rng.standard_normal(shape, dtype=np.float32) * 0.5, F16), ac.rnd_t(rng.standard_normal(shape, dtype=np.float32) * 0.5, F16))


def make_case(hs, ratio, steps, W, S, chunk, max_seq, shift=0, bias=False, scales=None, logit=LOGIT, seed=23, min_mass=0.9):
    """window_attn_cases.make_case at any max_seq_len (one layer, KVH KV heads, RoPE over the whole head, fp16 activations; scales =
    (k_scale, v_scale): e4m3 cache bytes) plus c.sink (float32 [nh]) / c.sink_cls; c.ref is the reference WITH the sink, c.ref_plain
    the one without, c.share[b][h] the sink's share of the total mass"""
    c = ac.Case()
    steps = [int(s) for s in steps]
    nh, kvh, bs, dtype = KVH * ratio, KVH, len(steps), F16
    assert all(1 <= s <= max_seq for s in steps) and W >= 0 and S >= 0 and (W > 0 or S == 0) and max_seq % KV_PAGE == 0
    rng = np.random.default_rng([seed, hs, ratio, W, S, int(bias), int(scales is not None), max_seq] + steps)
    c.dtype, c.hs, c.nh, c.kvh, c.rep, c.bs, c.L, c.layer = dtype, hs, nh, kvh, ratio, bs, 1, 0
    c.steps, c.uniform, c.max_seq, c.chunk, c.rope, c.rot, c.logit = steps, False, max_seq, chunk, True, hs, logit
    c.W, c.S, c.scales = W, S, scales
    qkv = ac.rnd_t(rng.standard_normal((bs, nh + 2 * kvh, hs)), dtype)
    c.bias = ac.rnd_t(rng.standard_normal(((nh + 2 * kvh) * hs,)) * 0.3, dtype) if bias else None
    bias3 = (c.bias if bias else np.zeros((nh + 2 * kvh) * hs, np.float32)).reshape(nh + 2 * kvh, hs).astype(np.float64)
    bq, bk, bv = bias3[:nh], bias3[nh:nh + kvh], bias3[nh + kvh:]
    c.tab = ac.rope_table(max_seq, hs, hs)
    rot_fwd = lambda x, b: ac.rnd_t(ac._rope(x, c.tab[steps[b] - 1]), dtype).astype(np.float64)
    q_eff = np.stack([rot_fwd(qkv[b, :nh].astype(np.float64), b) + bq for b in range(bs)])
    kb, vb = _background(hs, bs, max_seq, scales is not None, seed)
    if scales is None:
        kc, vc = kb.copy(), vb.copy()
        store = lambda x: ac.rnd_t(x, dtype)
    else:
        kc, vc = kb.copy(), vb   # codes
        store = lambda x: ac.to_e4m3(np.asarray(x, np.float64) / scales[0])
    c.pos = [[None] * nh for _ in range(bs)]
    c.cls = [["none"] * nh for _ in range(bs)]
    c.classes, c.outside = [], []
    for b in range(bs):
        items = wc.position_classes(steps[b], W, S, chunk, rng)
        c.classes.append(items)
        used = [set() for _ in range(kvh)]
        for h in range(nh):
            g = h // ratio
            start = (3 * b + h) % len(items)
            for k in range(len(items)):
                name, p = items[(start + k) % len(items)]
                if p not in used[g]:
                    used[g].add(p)
                    c.pos[b][h], c.cls[b][h] = p, name
                    break
        for h in range(nh):
            p, g = c.pos[b][h], h // ratio
            if p is None:
                continue
            target = q_eff[b, h] * (logit * np.sqrt(hs) / np.dot(q_eff[b, h], q_eff[b, h]))
            if p == steps[b] - 1:
                qkv[b, nh + g] = ac.rnd_t(ac._rope(target - bk[g], c.tab[p], inverse=True), dtype)
            else:
                kc[0, b, g, p] = store(target)
        c.outside.append(wc.outside_positions(steps[b], W, S))
        for g in range(kvh):
            qs = q_eff[b, g * ratio:(g + 1) * ratio]
            dots = qs @ qs.sum(axis=0) / np.sqrt(hs)
            for p in c.outside[b]:
                assert dots.min() > 0, "the group's query heads do not share a direction"
                kc[0, b, g, p] = store(qs.sum(axis=0) * (wc.OUT_LOGIT / dots.min()))
    c.qkv, c.q_eff = qkv, q_eff
    kn, vn = qkv[:, nh:nh + kvh].astype(np.float64), qkv[:, nh + kvh:].astype(np.float64)
    k_new = np.stack([ac.rnd_t(rot_fwd(kn[b], b) + bk, dtype) for b in range(bs)]).astype(np.float64)
    v_new = ac.rnd_t(vn + bv, dtype).astype(np.float64)
    if scales is None:
        c.kc, c.vc, c.k_new, c.v_new = kc, vc, k_new, v_new
    else:
        c.kq, c.vq = kc, vc
        c.kc, c.vc = ac._Deq(kc, scales[0]), ac._Deq(vc, scales[1])
        c.k_codes_new, c.v_codes_new = ac.to_e4m3(k_new / scales[0]), ac.to_e4m3(v_new / scales[1])
    c.sink, c.sink_cls = sink_values(nh, shift, logit)
    return finish(c, min_mass=min_mass)


def finish(c, k_codes_new=None, v_codes_new=None, min_mass=0.9):
    """(re)compute the references and assert the generator's conditions; e4m3: with the appended rows as these codes"""
    if c.scales is not None:
        c.k_new = (ac.E4M3[c.k_codes_new if k_codes_new is None else k_codes_new] * np.float32(c.scales[0])).astype(np.float64)
        c.v_new = (ac.E4M3[c.v_codes_new if v_codes_new is None else v_codes_new] * np.float32(c.scales[1])).astype(np.float64)
    c.ref_plain, c.mass, c.out_mass = wc.reference(c, c.W, c.S, with_mass=True)
    c.ref, c.share, c.top = attend(c, c.sink, with_share=True)
    for b in range(c.bs):
        for h in range(c.nh):
            if c.pos[b][h] is None:
                continue
            assert c.mass[b][h] >= min_mass, "planted row holds %.3f of the real keys' mass: %s" % (c.mass[b][h], describe(c, "generator", b, h))
            lo, hi = SHARE[c.sink_cls[h]]
            assert lo <= c.share[b][h] <= hi, "sink class %s holds %.4g of the mass: %s" % (c.sink_cls[h], c.share[b][h], describe(c, "generator", b, h))
            if c.sink_cls[h] == "above":
                assert c.sink[h] > c.top[b][h], describe(c, "generator", b, h)
            for p, m in c.out_mass[b][h].items():
                assert m >= min_mass, "outside row %d would hold only %.3f: %s" % (p, m, describe(c, "generator", b, h))
    return c


def describe(c, form, b=None, h=None):
    s = wc.describe(c, form, b, h)
    return s if h is None else s + " sink=%s (%g)" % (c.sink_cls[h], c.sink[h])


def attend(c, sink, defect=None, with_share=False):
    """float64 attention of the decode case under its mask with the sink logits `sink` ([nh], -inf = none).  defect: one of DEFECTS
    seeded into it -- a deliberately wrong restatement, the mutation check of tests/test_sink_cases_cpu.py"""
    sink = np.asarray(sink, np.float64)
    out = np.zeros((c.bs, c.nh * c.hs))
    share = [[0.0] * c.nh for _ in range(c.bs)]
    top = [[0.0] * c.nh for _ in range(c.bs)]
    for b in range(c.bs):
        s = c.steps[b]
        vis = wc.visible(s, c.W, c.S)
        nsplits = len(wc.live_chunks(s, c.W, c.S, c.chunk))
        for g in range(c.kvh):
            K = np.array(c.kc[c.layer, b, g, :s], np.float64)
            V = np.array(c.vc[c.layer, b, g, :s], np.float64)
            K[s - 1], V[s - 1] = c.k_new[b, g], c.v_new[b, g]
            for h in range(g * c.rep, (g + 1) * c.rep):
                lg = np.where(vis, K @ c.q_eff[b, h] / np.sqrt(c.hs), -np.inf)
                sh = sink[{"group_div": h // c.rep, "group_mod": h % c.rep}.get(defect, h)]
                if defect == "missing" or (defect == "before_mask" and not (c.W > 0 and s >= c.W)):
                    sh = -np.inf
                count = {"per_split": nsplits, "per_lane": 4}.get(defect, 1)
                m = max(lg.max(), sh)
                e = np.exp(lg - m)
                if defect == "no_max":   # the real keys under their own maximum, the sink as exp(s) in fp32
                    e = np.exp(lg - lg.max())
                    with np.errstate(over="ignore"):
                        es = float(np.exp(np.float32(sh)))
                else:
                    es = count * np.exp(sh - m)
                num = e @ V + (es * V[s - 1] if defect == "as_key" else 0.0)
                den = e.sum() + es + 1e-6
                out[b, h * c.hs:(h + 1) * c.hs] = num / den if np.isfinite(den) else 0.0
                share[b][h], top[b][h] = float(es / (e.sum() + es)) if np.isfinite(es) else 1.0, float(lg.max())
    return (out, share, top) if with_share else out


def applies(c, defect):
    """can this defect change the reference of this case?"""
    if defect in ("group_div", "group_mod"):
        return c.rep > 1
    if defect == "per_split":
        return any(len(wc.live_chunks(s, c.W, c.S, c.chunk)) > 1 for s in c.steps)
    if defect == "before_mask":
        return any(not (c.W > 0 and s >= c.W) for s in c.steps)
    return True


def distance(c, wrong, bounds):
    """largest |wrong - ref| / bound over the case"""
    rtol, atol = bounds
    return float((np.abs(np.asarray(wrong) - c.ref) / (atol + rtol * np.abs(c.ref))).max())


check = wc.check


# the decode geometries of tests/test_sink_decode_gpu.py: (id, head_size, ratio, bias, scales or None)
GEOMETRIES = [("f16-hs128-r1", 128, 1, False, None), ("f16-hs128-r8", 128, 8, True, None),
              ("f16-hs64-r1", 64, 1, True, None), ("f16-hs64-r8", 64, 8, False, None),
              ("e4m3-hs128-r4", 128, 4, True, (0.037, 0.021)), ("e4m3-hs64-r4", 64, 4, False, (1.0 / 32, 1.0 / 16))]
CPW_GEOMETRY = ("e4m3-hs128-r1-b64", 128, 1, False, (1.0 / 32, 1.0 / 16))
CPW_BATCH = 64


def max_seq_of(chunk):
    """17 chunks and a few tokens, in whole pages"""
    return -(-(17 * chunk + 5) // KV_PAGE) * KV_PAGE


def step_sets(chunk):
    """two ragged batches of 3 whose splits per sequence (no window) are 1 (the direct store), 2, 16 and 17 (a second merge round)"""
    return [[chunk - 3, chunk + 1, 16 * chunk + 5], [16 * chunk, 15 * chunk + 1, 1]]


def windows(chunk):
    """(W, S): full attention; a window below a chunk with 4 sink tokens; a window spanning three chunks"""
    return [(0, 0), (chunk - 28, 4), (2 * chunk + 37, 0)]


def decode_cases():
    return [("%s-W%d-S%d" % (g[0], W, S), g, W, S) for g in GEOMETRIES for W, S in windows(ac.chunk_len(F16, g[1], e4m3=g[4] is not None))]


def build(geo, W, S, steps, chunk, max_seq, shift=0):
    _, hs, ratio, bias, scales = geo
    return make_case(hs, ratio, steps, W, S, chunk, max_seq, shift=shift, bias=bias, scales=scales)


# ------------------------------------------------------------------------------------------------------------------ prefill
def prefill_reference(c, kfull, vfull, sink, defect=None, with_share=False):
    """window_attn_cases.prefill_reference with the sink column: one [length, nh HS] array per sequence; with_share: also
    {(s, i, h): the sink's share of row i's total mass} for the owners"""
    import prefill_attn_cases as pc
    sink = np.asarray(sink, np.float64)
    outs, share = [], {}
    for s in range(c.bs):
        ln, hist, ctx = c.lens[s], c.hist[s], c.ctx[s]
        n = min(ctx + 1, c.max_seq)
        vis = wc.prefill_visible(hist + np.arange(ln), n, c.W, c.S)
        out = np.zeros((ln, c.nh * pc.HS))
        for g in range(c.kvh):
            K, V = kfull[0, s, g, :n].astype(np.float64), vfull[0, s, g, :n].astype(np.float64)
            for h in range(g * c.rep, (g + 1) * c.rep):
                sc = np.where(vis, c.q_eff[c.cum[s]:c.cum[s] + ln, h] @ K.T / np.sqrt(pc.HS), -np.inf)
                sh = sink[{"group_div": h // c.rep, "group_mod": h % c.rep}.get(defect, h)]
                if defect == "missing":
                    sh = -np.inf
                m = np.maximum(sc.max(axis=1), sh)
                e = np.exp(sc - m[:, None])
                es = (4 if defect == "per_lane" else 1) * np.exp(sh - m)
                den = e.sum(axis=1) + es
                out[:, h * pc.HS:(h + 1) * pc.HS] = (e @ V) / (den + 1e-6)[:, None]
                for i, o in c.by_seq_head.get((s, h), []):
                    share[(s, i, h)] = float(es[i] / den[i])
        outs.append(out)
    return (outs, share) if with_share else outs


def make_prefill_case(cid, nh, kvh, lens, hist, kv, form, W, S, shift=0):
    """window_attn_cases.make_prefill_case (W = 0: full causal attention) plus c.sink / c.sink_cls; c.ref with the sink, c.ref_plain
    without; the classes' shares asserted at every owner row"""
    import prefill_attn_cases as pc
    c = wc.make_prefill_case(cid, nh, kvh, lens, hist, kv, form, W, S)
    c.sink, c.sink_cls = sink_values(nh, shift, pc.LOGIT)
    c.ref_plain = c.ref
    c.ref, c.share = prefill_reference(c, c.deq(c.k_cpu, 0), c.deq(c.v_cpu, 1), c.sink, with_share=True)
    for (s, i, h), sh in c.share.items():
        lo, hi = SHARE[c.sink_cls[h]]
        assert lo <= sh <= hi, "%s W=%d S=%d owner %s: sink class %s holds %.4g of the mass" % (cid, W, S, (s, i, h), c.sink_cls[h], sh)
    return c
