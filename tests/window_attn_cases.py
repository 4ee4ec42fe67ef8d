"""Sliding-window decode-attention cases whose inputs can fail: one generator shared by tests/test_window_cases_cpu.py (the
tests of the tests) and tests/test_window_decode_gpu.py (the kernels).  Plain module, no fixtures; builds on tests/attn_cases.py.

Mask (include/llmie.h): the query at position step - 1 sees key j iff j < step and (j >= step - W or j < S); W = 0 is full
attention.  As in attn_cases every (sequence, query head) owns ONE cache position whose K row is c * q_eff, logit 12 over a +-0.5
background, so that it holds >= 0.9 of the softmax mass AMONG THE KEYS THE MASK EXPOSES; the positions cycle through the places
where the windowed kernel changes behaviour (first / last row of the window, last sink, chunk and page boundaries inside the live
ranges, the appended token).

What a window adds: a kernel that reads one key too many must be wrong by O(0.5), not by noise.  So every case also plants a
dominating row JUST OUTSIDE the mask of every KV head -- at step - 1 - W (the row in front of the window) and at S (the row behind
the sinks) wherever those are dead -- aimed at the sum of the group's query heads with a logit of at least OUT_LOGIT for each:
were it visible it would take >= 0.9 of the mass of every head (asserted by the generator).

Reference (reference()): numpy float64 restatement of the masked softmax on the inputs as rounded to the dtype under test -- for an
e4m3 cache on the de-quantised bytes, i.e. what the cache stores -- with the library's sum + 1e-6 denominator.
"""
import functools

import numpy as np

import attn_cases as ac

F16 = ac.F16
KV_PAGE = ac.KV_PAGE
OUT_LOGIT = 18.0
MAX_SEQ, BATCH, KVH = 2048, 3, 2
NAN_CODE = 0x7F   # e4m3 NaN


# ------------------------------------------------------------------------------------------- the mask and the live-chunk mapping
def visible(step, W, S):
    """bool [step]: which keys the query at step - 1 sees"""
    t = np.arange(step)
    return np.ones(step, bool) if W <= 0 else ((t >= step - W) | (t < S))


def live_chunks(step, W, S, chunk):
    """the chunks (of `chunk` tokens, aligned to token 0) a windowed call walks, in split-index order: restatement of
    attn_live_chunks / attn_live_chunk of csrc/attention_decode.hip"""
    n = -(-step // chunk)
    if W <= 0 or W >= step:
        return list(range(n))
    first = (step - W) // chunk
    ns = -(-min(max(S, 0), step) // chunk)
    if ns >= first:
        return list(range(n))
    return list(range(ns)) + list(range(first, n))


def live_bound(max_seq, W, S, chunk):
    """grid x of a call whose position lives on the device"""
    n = -(-max_seq // chunk)
    return n if W <= 0 else min(n, -(-max(S, 0) // chunk) + -(-W // chunk) + 1)


def ring_pages(W, S, n=1):
    """pool pages a windowed sequence lives in at any context length (llmie_kv_window_advance)"""
    return -(-S // KV_PAGE) + -(-(W + n) // KV_PAGE) + 1


def ring_advance(row, cached, n, W, S):
    """restatement of llmie_kv_window_advance for one table row (list, -1 = unmapped): (new row, status)"""
    row = list(row)
    if n <= 0:
        return row, 0
    if cached < 0 or cached + n > len(row) * KV_PAGE:
        return row, 2
    p0, p1 = cached // KV_PAGE, (cached + n - 1) // KV_PAGE
    lo = min(-(-S // KV_PAGE), len(row))
    dead_end = cached + 1 - W
    hi = min(p0, dead_end // KV_PAGE) if dead_end > 0 else 0
    need = [p for p in range(p0, p1 + 1) if row[p] < 0]
    have = [p for p in range(lo, hi) if row[p] >= 0]
    if len(have) < len(need):
        return row, 1
    for p, d in zip(need, have):
        row[p], row[d] = row[d], -1
    return row, 0


# ---------------------------------------------------------------------------------------------------------------- the generator
def position_classes(step, W, S, chunk, rng, n_random=2):
    """ordered (class, position) pairs among the VISIBLE keys of a context of `step` tokens"""
    vis = visible(step, W, S)
    t_lo = max(0, step - W) if W > 0 else 0
    s_eff = min(S, step) if W > 0 else 0
    items = [("new", step - 1), ("win_first", t_lo), ("prev", step - 2), ("win_second", t_lo + 1), ("sink_last", s_eff - 1), ("first", 0)]
    for unit, name in ((chunk, "chunk"), (KV_PAGE, "page")):
        m = -(-t_lo // unit) * unit                      # first boundary at or behind the window start
        items += [(name + "_lo", m - 1), (name + "_hi", m)]
        m = ((step - 1) // unit) * unit                  # last boundary of the context
        items += [(name + "_last_lo", m - 1), (name + "_last_hi", m)]
        m = ((s_eff - 1) // unit) * unit if s_eff > 0 else -1   # last boundary inside the sinks
        items += [("sink_" + name + "_lo", m - 1), ("sink_" + name + "_hi", m)]
    live = np.flatnonzero(vis)
    items += [("random", int(live[rng.integers(0, len(live))])) for _ in range(n_random)]
    names, out, seen = {}, [], set()
    for name, p in items:
        if 0 <= p < step and vis[p] and name not in names.setdefault(p, []):
            names[p].append(name)
    for name, p in items:
        if 0 <= p < step and vis[p] and p not in seen:
            seen.add(p)
            out.append(("+".join(names[p]), p))
    return out


def outside_positions(step, W, S):
    """the dead rows next to the mask: in front of the window, and behind the sinks"""
    if W <= 0 or W >= step:
        return []
    out = []
    if S < step - W:
        out.append(step - 1 - W)
        if S < step - W - 1:
            out.append(S)
    return out


@functools.lru_cache(maxsize=2)
def _background(hs, seed, bs):
    rng = np.random.default_rng([seed, hs, bs])
    shape = (1, bs, KVH, MAX_SEQ, hs)
    return (ac.rnd_t(rng.standard_normal(shape, dtype=np.float32) * 0.5, F16), ac.rnd_t(rng.standard_normal(shape, dtype=np.float32) * 0.5, F16))


@functools.lru_cache(maxsize=2)
def _background_e4m3(hs, seed, bs):
    rng = np.random.default_rng([seed, hs, 8, bs])
    shape = (1, bs, KVH, MAX_SEQ, hs)
    codes = lambda: rng.integers(0, 0x58, shape, dtype=np.uint8) | (rng.integers(0, 2, shape, dtype=np.uint8) << 7)
    return codes(), codes()


def make_case(hs, ratio, steps, W, S, chunk, bias=False, scales=None, logit=12.0, seed=11, min_mass=0.9):
    """fp16 activations; scales = (k_scale, v_scale): the caches are e4m3 bytes.  One layer, one sequence per entry of `steps`, KVH KV
    heads, max_seq_len MAX_SEQ, RoPE over the whole head.  The result is an attn_cases.Case (attn_cases.reference applies to it)
    with W, S, the outside plants (c.outside[b] = positions) and ref / mass under the mask."""
    c = ac.Case()
    steps = [int(s) for s in steps]
    nh, kvh, bs, dtype = KVH * ratio, KVH, len(steps), F16
    assert all(1 <= s <= MAX_SEQ for s in steps) and W >= 0 and S >= 0 and (W > 0 or S == 0)
    rng = np.random.default_rng([seed, hs, ratio, W, S, int(bias), int(scales is not None)] + steps)
    c.dtype, c.hs, c.nh, c.kvh, c.rep, c.bs, c.L, c.layer = dtype, hs, nh, kvh, ratio, bs, 1, 0
    c.steps, c.uniform, c.max_seq, c.chunk, c.rope, c.rot, c.logit = steps, False, MAX_SEQ, chunk, True, hs, logit
    c.W, c.S, c.scales = W, S, scales
    qkv = ac.rnd_t(rng.standard_normal((bs, nh + 2 * kvh, hs)), dtype)
    c.bias = ac.rnd_t(rng.standard_normal(((nh + 2 * kvh) * hs,)) * 0.3, dtype) if bias else None
    bias3 = (c.bias if bias else np.zeros((nh + 2 * kvh) * hs, np.float32)).reshape(nh + 2 * kvh, hs).astype(np.float64)
    bq, bk, bv = bias3[:nh], bias3[nh:nh + kvh], bias3[nh + kvh:]
    c.tab = ac.rope_table(MAX_SEQ, hs, hs)
    rot_fwd = lambda x, b: ac.rnd_t(ac._rope(x, c.tab[steps[b] - 1]), dtype).astype(np.float64)
    q_eff = np.stack([rot_fwd(qkv[b, :nh].astype(np.float64), b) + bq for b in range(bs)])
    if scales is None:
        kb, vb = _background(hs, seed, bs)
        kc, vc = kb.copy(), vb.copy()
        store = lambda x: ac.rnd_t(x, dtype)
    else:
        ks, vs = scales
        kb, vb = _background_e4m3(hs, seed, bs)
        kc, vc = kb.copy(), vb        # codes
        store = lambda x: ac.to_e4m3(np.asarray(x, np.float64) / ks)
    c.pos = [[None] * nh for _ in range(bs)]
    c.cls = [["none"] * nh for _ in range(bs)]
    c.classes, c.outside = [], []
    for b in range(bs):
        items = position_classes(steps[b], W, S, chunk, rng)
        c.classes.append(items)
        used = [set() for _ in range(kvh)]
        for h in range(nh):
            g = h // ratio
            start = (3 * b + h) % len(items)
            for k in range(len(items)):   # the heads of one KV head get distinct positions, while there are any left
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
            if p == steps[b] - 1:   # the appended token: its pre-image goes into the qkv row
                qkv[b, nh + g] = ac.rnd_t(ac._rope(target - bk[g], c.tab[p], inverse=True), dtype)
            else:
                kc[0, b, g, p] = store(target)
        # the rows just outside the mask: aimed at the sum of the group's heads, at least OUT_LOGIT for each of them
        c.outside.append(outside_positions(steps[b], W, S))
        for g in range(kvh):
            qs = q_eff[b, g * ratio:(g + 1) * ratio]
            dots = qs @ qs.sum(axis=0) / np.sqrt(hs)
            assert dots.min() > 0, "the group's query heads do not share a direction"
            for p in c.outside[b]:
                kc[0, b, g, p] = store(qs.sum(axis=0) * (OUT_LOGIT / dots.min()))
    c.qkv, c.q_eff = qkv, q_eff
    kn, vn = qkv[:, nh:nh + kvh].astype(np.float64), qkv[:, nh + kvh:].astype(np.float64)
    k_new = np.stack([ac.rnd_t(rot_fwd(kn[b], b) + bk, dtype) for b in range(bs)]).astype(np.float64)
    v_new = ac.rnd_t(vn + bv, dtype).astype(np.float64)
    if scales is None:
        c.kc, c.vc, c.k_new, c.v_new = kc, vc, k_new, v_new
    else:   # what the cache stores is what is attended to
        c.kq, c.vq = kc, vc
        c.kc, c.vc = ac._Deq(kc, scales[0]), ac._Deq(vc, scales[1])
        c.k_codes_new, c.v_codes_new = ac.to_e4m3(k_new / scales[0]), ac.to_e4m3(v_new / scales[1])
    finish(c, min_mass=min_mass)
    return c


def finish(c, k_codes_new=None, v_codes_new=None, min_mass=0.9):
    """(re)compute the reference; e4m3: with the appended rows as these codes (default: the CPU's rounding of them)"""
    if c.scales is not None:
        c.k_new = (ac.E4M3[c.k_codes_new if k_codes_new is None else k_codes_new] * np.float32(c.scales[0])).astype(np.float64)
        c.v_new = (ac.E4M3[c.v_codes_new if v_codes_new is None else v_codes_new] * np.float32(c.scales[1])).astype(np.float64)
    c.ref, c.mass, c.out_mass = reference(c, c.W, c.S, with_mass=True)
    for b in range(c.bs):
        for h in range(c.nh):
            if c.pos[b][h] is not None:
                assert c.mass[b][h] >= min_mass, "planted row holds %.3f of the visible mass: %s" % (c.mass[b][h], describe(c, "generator", b, h))
            for p, m in c.out_mass[b][h].items():
                assert m >= min_mass, "outside row %d would hold only %.3f: %s" % (p, m, describe(c, "generator", b, h))
    return c


def describe(c, form, b=None, h=None):
    s = "hs=%d ratio=%d kv=%s W=%d S=%d steps=%s form=%s" % (c.hs, c.rep, "e4m3" if c.scales else "f16", c.W, c.S, c.steps, form)
    if b is not None:
        s += " b=%d h=%d position=%s class=%s outside=%s" % (b, h, c.pos[b][h], c.cls[b][h], c.outside[b])
    return s


def reference(c, W, S, with_mass=False):
    """float64 masked softmax attention of the case under window W / sinks S.  with_mass: also the share of the visible mass each
    owner's row holds, and per head {outside position: the share it WOULD hold if the mask let that one row in}"""
    out = np.zeros((c.bs, c.nh * c.hs))
    mass = [[0.0] * c.nh for _ in range(c.bs)]
    out_mass = [[{} for _ in range(c.nh)] for _ in range(c.bs)]
    for b in range(c.bs):
        s = c.steps[b]
        vis = visible(s, W, S)
        for g in range(c.kvh):
            K = np.array(c.kc[c.layer, b, g, :s], np.float64)
            V = np.array(c.vc[c.layer, b, g, :s], np.float64)
            K[s - 1], V[s - 1] = c.k_new[b, g], c.v_new[b, g]
            for h in range(g * c.rep, (g + 1) * c.rep):
                lg_all = K @ c.q_eff[b, h] / np.sqrt(c.hs)
                lg = np.where(vis, lg_all, -np.inf)
                m = lg.max()
                e = np.exp(lg - m)
                out[b, h * c.hs:(h + 1) * c.hs] = e @ V / (e.sum() + 1e-6)
                if with_mass:
                    if c.pos[b][h] is not None:
                        mass[b][h] = float(e[c.pos[b][h]] / e.sum())
                    for p in getattr(c, "outside", [[]] * c.bs)[b]:
                        if not vis[p]:
                            m2 = max(m, lg_all[p])
                            out_mass[b][h][p] = float(np.exp(lg_all[p] - m2) / (np.exp(lg - m2).sum() + np.exp(lg_all[p] - m2)))
    return (out, mass, out_mass) if with_mass else out


def check(got, c, form, bounds, extra_atol=0.0):
    """attn_cases.check with this module's description of the case"""
    rtol, atol = bounds
    got = np.asarray(got, np.float64).reshape(c.ref.shape)
    ratio = np.abs(got - c.ref) / (atol + rtol * np.abs(c.ref) + extra_atol)
    bad = ~(ratio <= 1.0)
    if bad.any():
        score = np.where(np.isnan(ratio), np.inf, ratio)
        b, k = np.unravel_index(np.argmax(score), score.shape)
        h, d = divmod(int(k), c.hs)
        raise AssertionError("%s dim=%d: got %r expected %r (error / bound %.3g, %d elements out of bound)" % (
            describe(c, form, int(b), h), d, float(got[b, k]), float(c.ref[b, k]), float(score[b, k]), int(bad.sum())))
    return float(ratio.max())


def dead_rows(c):
    """bool [bs, max_seq]: cache rows no query of the case may read (masked, or past the context)"""
    dead = np.ones((c.bs, c.max_seq), bool)
    for b, s in enumerate(c.steps):
        dead[b, :s] = ~visible(s, c.W, c.S)
    return dead


def dead_pages(c):
    """bool [bs, max_pages]: pages without a visible row"""
    return dead_rows(c).reshape(c.bs, -1, KV_PAGE).all(axis=2)


# --------------------------------------------------------------------------------------------------------------- the case table
# (id, head_size, ratio, bias, scales or None); chunk: fp16 hs 128 -> 128 (one page), fp16 hs 64 -> 256 (two pages), e4m3 hs 128 ->
# 256 (two pages), e4m3 hs 64 -> 512 (FOUR pages: the one geometry where a chunk's live page can have dead pages on both sides)
GEOMETRIES = [("f16-hs128-r1", 128, 1, False, None), ("f16-hs128-r4", 128, 4, True, None),
              ("f16-hs64-r1", 64, 1, True, None), ("f16-hs64-r4", 64, 4, False, None),
              ("e4m3-hs128-r1", 128, 1, False, (1.0 / 32, 1.0 / 16)), ("e4m3-hs128-r4", 128, 4, True, (0.037, 0.021)),
              ("e4m3-hs64-r2", 64, 2, False, (1.0 / 32, 1.0 / 16))]


def chunk_of(geo):
    return ac.chunk_len(F16, geo[1], e4m3=geo[4] is not None)


def windows(chunk):
    return [1, 5, chunk - 1, chunk, chunk + 1, 2 * chunk + 37]


def step_sets(W, chunk):
    """three ragged batches: step - W on a chunk start, on a chunk end and on a page boundary; mid-chunk, step <= W and step = 1; the
    longest context, step - W = 1 and a far window"""
    C = chunk
    sets = [[W + 2 * C, W + 3 * C - 1, W + C + KV_PAGE], [W + C + 37, max(1, W - 1), 1], [MAX_SEQ, W + 1, W + 5 * C + 5]]
    return [[min(MAX_SEQ, s) for s in st] for st in sets]   # (512-token chunks under the largest window: the slab ends first)


def sink_sets(W, chunk):
    """(S, steps): the plain sink counts on every step set; S touching and overlapping the window start of the first sequence of
    the first set (step - W = 2 chunks)"""
    sets = step_sets(W, chunk)
    out = [(S, st) for S in (0, 1, 4, chunk + 3) for st in sets]
    out += [(2 * chunk, sets[0]), (2 * chunk + 5, sets[0])]
    return out


def decode_cases():
    """[(id, geometry, W)]; each expands to sink_sets(W, chunk)"""
    return [("%s-W%d" % (g[0], W), g, W) for g in GEOMETRIES for W in windows(chunk_of(g))]


# e4m3 cache, 64 sequences x 2 KV heads: the planner gives such a batch TWO chunks per workgroup (spans of 512 tokens), and the
# windowed workgroup has to start at its span's first live chunk and skip dead ones
CPW_GEOMETRY = ("e4m3-hs128-r1-b64", 128, 1, False, (1.0 / 32, 1.0 / 16))
CPW_BATCH = 64


def cpw_cases():
    """[(W, S, steps)]: the step sets of the small batches, cycled over 64 sequences"""
    C, out = chunk_of(CPW_GEOMETRY), []
    for W, S in ((5, 0), (5, 4), (C + 1, 4), (C + 1, C + 3), (2 * C + 37, 1), (2 * C + 37, 3 * C)):
        pool = sorted({s for st in step_sets(W, C) for s in st} | {W + 2 * C + 1, W + 4 * C, W + 4 * C - 1, 2 * C, 2 * C + 1})
        out.append((W, S, [pool[(7 * b) % len(pool)] for b in range(CPW_BATCH)]))
    return out


def build(geo, W, S, steps):
    _, hs, ratio, bias, scales = geo
    return make_case(hs, ratio, steps, W, S, chunk_of(geo), bias=bias, scales=scales)


# =========================================================================================================== windowed prefill
# The flash prefill kernel under a window, through a one-layer engine as tests/prefill_attn_cases.py reaches it (QKV weight column t
# IS token t's pre-RoPE row, o = identity, gate_up = 0).  That module draws the rows and caches (planted=False); the owners here lie
# INSIDE the mask of their query row -- the diagonal, the first rows of the window, the last sink, tile boundaries inside the window
# -- and every owner also gets, where those slots are dead for its row and free, a dominating row at qpos - W (in front of its
# window), at S (behind the sinks) and at qpos + 1 (its future), each with logit OUT_PREFILL toward the owner's query.
OUT_PREFILL = 16.0
PREFILL_LENS, PREFILL_HIST = [1, 63, 64, 65, 130, 300], [200, 128, 37, 0, 37, 0]
PREFILL_WINDOWS, PREFILL_SINKS = [1, 5, 17, 64, 65, 200, 512], [0, 4, 70]      # (512 >= every context: full attention)
# larger batches that reach the other two flash forms (tests/prefill_attn_cases.TABLE): (nh, kvh, lens, hist, form)
PREFILL_FORMS = [("rt2", 32, 8, [512, 300, 1, 40], [0, 37, 128, 256], "q128w4t2"), ("w8", 32, 8, [640, 128, 1], [37, 0, 128], "q128w8t1")]


def prefill_visible(qpos, n, W, S):
    """bool [len(qpos), n]: key t seen from the query positions qpos"""
    t, q = np.arange(n)[None, :], np.asarray(qpos)[:, None]
    return (t <= q) & ((t > q - W) | (t < S)) if W > 0 else (t <= q)


def _prefill_slots(hist, i, W, S, rng, n_random):
    import prefill_attn_cases as pc
    qpos = hist + i
    lo = max(0, qpos - W + 1) if W > 0 else 0
    items = [("diag", qpos), ("win_first", lo), ("prev", qpos - 1), ("win_second", lo + 1), ("sink_last", min(S, qpos + 1) - 1), ("first", 0),
             ("tile_first", (qpos // pc.BT) * pc.BT), ("prev_tile_last", (qpos // pc.BT) * pc.BT - 1), ("hist_last", hist - 1),
             ("win_tile_hi", -(-lo // pc.BT) * pc.BT), ("win_tile_lo", -(-lo // pc.BT) * pc.BT - 1), ("page_hi", (qpos // 128) * 128),
             ("page_lo", (qpos // 128) * 128 - 1)]
    vis = prefill_visible([qpos], qpos + 1, W, S)[0]
    live = np.flatnonzero(vis)
    items += [("random", int(live[rng.integers(0, len(live))])) for _ in range(n_random)]
    out, seen = [], set()
    for name, p in items:
        if 0 <= p <= qpos and vis[p] and p not in seen:
            seen.add(p)
            out.append((name, p))
    return out


def make_prefill_case(cid, nh, kvh, lens, hist, kv, form, W, S, seed=11, min_mass=0.9):
    """a prefill_attn_cases.PrefillCase (one layer) with owners inside the window / sink mask and dominating rows just outside it;
    c.ref / c.mass under the mask, c.outside = {(sequence, row, head): [slots]}"""
    import prefill_attn_cases as pc
    c = pc.make_case(cid, nh, kvh, 1, lens, hist, kv, form, "separate", planted=False, seed=seed)
    c.W, c.S = W, S
    rng = np.random.default_rng([seed, 77, W, S, nh, kvh] + c.lens + c.hist)
    sq, rep = float(np.sqrt(c.H)), c.rep

    def plant(s, g, slot, q, logit):   # (as prefill_attn_cases.make_case)
        target = q * (logit * np.sqrt(pc.HS) / np.dot(q, q))
        if slot < c.hist[s] or slot >= c.ctx[s]:
            c.k0[0, s, g, slot] = c.store(target, 0)
        else:
            t = c.cum[s] + slot - c.hist[s]
            c.w[0, t, nh + g] = ac.rnd_t(ac._rope(target, c.tab[slot], inverse=True) / sq, F16)
            c.rows[0, t, nh + g] = c.w[0, t, nh + g] * np.float32(sq)

    c.owners, c.outside, taken, k = {}, {}, set(), 0
    for s in range(c.bs):
        for i in pc.owner_rows(c.lens[s], c.bq, rng):
            items = _prefill_slots(c.hist[s], i, W, S, rng, 2 + 2 * rep)
            for h in range(nh):
                for j in range(len(items)):
                    name, p = items[(k + j) % len(items)]
                    if (s, h // rep, p) not in taken:
                        taken.add((s, h // rep, p))
                        c.owners[(s, i, h)] = pc.Owner(p, name, pc.row_class(c.lens[s], c.bq, i))
                        break
                k += 1
    for (s, i, h), o in c.owners.items():
        plant(s, h // rep, o.slot, c.q_eff[c.cum[s] + i, h], pc.LOGIT)
    for n, ((s, i, h), o) in enumerate(c.owners.items()):
        qpos, outs = c.hist[s] + i, []
        cand = [qpos + 1] if n % 2 == 0 else []
        if W > 0:
            cand += [p for p in (qpos - W, S) if 0 <= p <= qpos - W and p >= S]
        for p in dict.fromkeys(cand):
            if p < c.max_seq and (s, h // rep, p) not in taken:
                taken.add((s, h // rep, p))
                plant(s, h // rep, p, c.q_eff[c.cum[s] + i, h], OUT_PREFILL)
                outs.append(p)
        c.outside[(s, i, h)] = outs
    c.by_seq_head = {}
    for (s, i, h), o in c.owners.items():
        c.by_seq_head.setdefault((s, h), []).append((i, o))
    kn, vn = c.rows[0, :, nh:nh + kvh].astype(np.float64), c.rows[0, :, nh + kvh:]
    c.k_new, c.v_new = [c.store(ac.rnd_t(pc.rope_rows(kn, c.tab, c.pos_of), F16), 0)], [c.store(vn, 1)]
    c.k_tol = [2 * ac.EPS[F16] * (np.abs(kn) + np.abs(np.concatenate([kn[..., pc.HS // 2:], kn[..., :pc.HS // 2]], axis=-1)))]
    c.k_cpu, c.v_cpu = pc.after_pass(c, c.k0, c.k_new), pc.after_pass(c, c.v0, c.v_new)
    c.ref, c.mass, c.out_mass = prefill_reference(c, c.deq(c.k_cpu, 0), c.deq(c.v_cpu, 1), W, S, with_mass=True)
    for key, m in c.mass.items():
        assert m >= min_mass, "planted row holds %.3f of the visible mass: %s W=%d S=%d owner %s" % (m, cid, W, S, key)
    for key, m in c.out_mass.items():
        assert m >= min_mass, "outside row would hold only %.3f: %s W=%d S=%d %s" % (m, cid, W, S, key)
    return c


def prefill_reference(c, kfull, vfull, W, S, with_mass=False):
    """float64 masked attention of the case on the caches AFTER the pass -> one [length, nh HS] array per sequence.  with_mass: the
    share of each owner's slot among the keys its row sees, and {(s, i, h, slot): share an outside row would take if let in}"""
    import prefill_attn_cases as pc
    outs, mass, out_mass = [], {}, {}
    for s in range(c.bs):
        ln, hist, ctx = c.lens[s], c.hist[s], c.ctx[s]
        n = min(ctx + 1, c.max_seq)
        vis = prefill_visible(hist + np.arange(ln), n, W, S)
        out = np.zeros((ln, c.nh * pc.HS))
        for g in range(c.kvh):
            K, V = kfull[0, s, g, :n].astype(np.float64), vfull[0, s, g, :n].astype(np.float64)
            for h in range(g * c.rep, (g + 1) * c.rep):
                raw = c.q_eff[c.cum[s]:c.cum[s] + ln, h] @ K.T / np.sqrt(pc.HS)
                sc = np.where(vis, raw, -np.inf)
                m = sc.max(axis=1)
                e = np.exp(sc - m[:, None])
                den = e.sum(axis=1)
                out[:, h * pc.HS:(h + 1) * pc.HS] = (e @ V) / (den + 1e-6)[:, None]
                if with_mass:
                    for i, o in c.by_seq_head.get((s, h), []):
                        mass[(s, i, h)] = float(e[i, o.slot] / den[i])
                        for p in c.outside.get((s, i, h), []):
                            if p < n and not vis[i, p]:
                                x = np.exp(raw[i, p] - m[i])
                                out_mass[(s, i, h, p)] = float(x / (den[i] + x))
        outs.append(out)
    return (outs, mass, out_mass) if with_mass else outs


def prefill_dead_rows(c):
    """bool [bs, max_seq]: history rows that no query of the pass sees"""
    dead = np.zeros((c.bs, c.max_seq), bool)
    if c.W > 0:
        for s in range(c.bs):
            t = np.arange(c.hist[s])
            dead[s, :c.hist[s]] = (t >= c.S) & (t < c.hist[s] - c.W + 1)
    return dead


# ======================================================================================================== a windowed engine
def window_layer_restatement(cfg, layers, x, k_cache, v_cache, lens, hist, layer_window, sinks, store=None, stored=None):
    """model_param_cases.layer_restatement with the attention of layer l masked by layer_window[l] (0 = full) and `sinks`: float64
    numpy, caches [L, bs, kvh, max_seq, hs] updated in place.  store(rows, which): what the cache keeps of a new K (0) / V (1) row
    (an e4m3 cache rounds it; default: the row itself).  stored = (K, V) values [L, bs, kvh, max_seq, hs] the DEVICE stored for the
    new rows (e4m3 cache): the layer attends to those -- an fp16 value that falls on the other side of an e4m3 rounding boundary on
    the device moves a stored element by a whole e4m3 step, which is the append's business (checked here to within one step), not the
    attention's."""
    import model_param_cases as mpc
    nh, kvh, hs, inter = cfg["head_num"], cfg["kv_head_num"], cfg["head_size"], cfg["inter_size"]
    eps, rot, base = cfg["rms_eps"], cfg["rotary_dim"], cfg["rotary_base"]
    rep, H, T = nh // kvh, nh * hs, int(sum(lens))
    starts = np.concatenate([[0], np.cumsum(lens)]).astype(int)
    pos = np.concatenate([hist[b] + np.arange(lens[b]) for b in range(len(lens))])
    h = np.asarray(x, np.float64).copy()
    f = lambda a: None if a is None else np.asarray(a, np.float64)
    store = store or (lambda rows, which: rows)
    for l, w in enumerate(layers):
        resid = h
        hn = mpc._norm(h, f(w["attn_norm"]), eps, "attn", l, frozenset())
        qkv = (hn @ f(w["qkv"]).T).reshape(T, nh + 2 * kvh, hs)
        q = mpc._rope(qkv[:, :nh], pos, hs, rot, base, "q", frozenset())
        k = mpc._rope(qkv[:, nh:nh + kvh], pos, hs, rot, base, "k", frozenset())
        v = qkv[:, nh + kvh:]
        att = np.empty((T, nh, hs))
        for b in range(len(lens)):
            s0, s1, h0 = starts[b], starts[b + 1], hist[b]
            k_cache[l, b, :, h0:h0 + lens[b]] = store(k[s0:s1].transpose(1, 0, 2), 0)
            v_cache[l, b, :, h0:h0 + lens[b]] = store(v[s0:s1].transpose(1, 0, 2), 1)
            if stored is not None:
                for cache, dev in ((k_cache, stored[0]), (v_cache, stored[1])):
                    mine, theirs = cache[l, b, :, h0:h0 + lens[b]], np.asarray(dev[l, b, :, h0:h0 + lens[b]], np.float64)
                    tol = 0.126 * np.abs(theirs) + 2.0 ** -6 * np.abs(theirs).max(axis=-1, keepdims=True)
                    assert (np.abs(mine - theirs) <= tol).all(), "layer %d sequence %d: stored rows off by %.3g" % (l, b, (np.abs(mine - theirs) - tol).max())
                    cache[l, b, :, h0:h0 + lens[b]] = theirs
            ctx = h0 + lens[b]
            K, V = k_cache[l, b, np.arange(nh) // rep, :ctx], v_cache[l, b, np.arange(nh) // rep, :ctx]
            sc = np.einsum("qhd,htd->hqt", q[s0:s1], K) / np.sqrt(hs)
            vis = prefill_visible(h0 + np.arange(lens[b]), ctx, layer_window[l], sinks)
            sc = np.where(vis[None], sc, -np.inf)
            p = np.exp(sc - sc.max(axis=2, keepdims=True))
            p = p / (p.sum(axis=2, keepdims=True) + 1e-6)
            att[s0:s1] = np.einsum("hqt,htd->qhd", p, V)
        resid = resid + att.reshape(T, H) @ f(w["o"]).T
        hn2 = mpc._norm(resid, f(w["ffn_norm"]), eps, "ffn", l, frozenset())
        gu = hn2 @ f(w["gate_up"]).T
        g, u = gu[:, :inter], gu[:, inter:]
        h = resid + ((g * 0.5 * (1.0 + np.tanh(0.5 * g))) * u) @ f(w["down"]).T
    return h
