"""Prefill-attention cases whose inputs can fail: one generator shared by tests/test_prefill_attn_cases_cpu.py (the tests of the
tests) and tests/test_prefill_attn_gpu.py (prefill_flash_kernel and the three producers of the K / V rows it reads).  Plain
module, no fixtures; the helpers are those of tests/attn_cases.py.

Reaching the kernel.  Prefill attention has no entry of its own, so the case is a Decoder whose weights let the test dictate every
token's q, k and v row: attn_norm = 1, o = identity, gate_up = 0 (the FFN adds exactly 0) and a one-hot hidden state, packed token
t = 64 e_t.  RMSNorm maps that row to sqrt(H) e_t (eps 1e-5: exactly 32 or 64 in fp16 for H = 1024 or 4096), so the QKV projection
returns sqrt(H) W_qkv[:, t] from a single non-zero product per output: COLUMN t OF THE QKV WEIGHT IS TOKEN t's PRE-RoPE ROW on every
GEMM route (total tokens <= H).  The fp16 column is drawn first and the row is sqrt(H) times it, so nothing is rounded.  hidden_out -
hidden_in is the attention output, rounded once more where x != 0 (one element per row: one fp16 ulp of |x| is allowed there).
History rows are written straight into the cache.  Cases with two layers give layer 0 o = 0: it is the identity, the measured layer
is layer 1, and layer 0's cache rows must still be written.

Why planted rows: a softmax over n near-equal logits is a mean of n V rows; a mask off by one, a key of a tile missing, two V rows
exchanged or a page from the wrong table entry move an element by O(0.5 / n), under every bound.  Here a (query row, head) pair that
is an OWNER gets one key slot p <= qpos whose K row is c q_eff with c chosen for a scaled logit of 12: that slot holds >= 0.9 of the
softmax mass (asserted by the generator), the output is essentially V[p], and reading another row is an O(0.5) error.  Some owners
also get a DECOY at slot qpos + 1 carrying logit 16 toward the same query (the next token's K row; for the last row of a sequence
the cache slot just past the context): a mask that lets it through moves the output to the decoy's V row.

Reference (reference()): numpy float64 on the values as the cache stores them, q_eff = round16(RoPE(q)), mask t <= history + i,
out = sum_t e_t V_t / (sum_t e_t + 1e-6).
"""
import numpy as np

from attn_cases import BOUNDS, E4M3, E4M3_SCALES, EPS, F16, _rope, check, rnd_t, rope_table, to_e4m3

HS, BT, PAGE = 128, 64, 128           # head size, keys per tile of the flash kernel, tokens per page
LOGIT, DECOY_LOGIT = 12.0, 16.0
X_ONE_HOT = 64.0
BOUND = BOUNDS["rope"][F16]            # (3e-3, 2e-3): what this project holds fp16 attention to
FORM_BQ = {"q64w4t1": 64, "q128w4t2": 128, "q128w8t1": 128}   # query rows per workgroup of the three shapes
PRODUCER_PLAN = {"splitk": "qkv=splitk_rope", "separate": "rope_append=1", "fused": "qkv=rope_f16"}
INTER = 512

# (id, head_num, kv_head_num, layers, lengths, histories, cache, flash form, producer of the new K / V rows).  Ragged batches chosen so
# that each form is reached at the smallest token count (the form is a function of heads x sequences x 128-row tiles and of the
# longest sequence); total tokens <= H = 128 head_num.  The CPU test asserts form and producer from the plan text.
TABLE = [
    ("f16-8x8-splitk", 8, 8, 1, [64, 1, 45], [0, 128, 37], "f16", "q64w4t1", "splitk"),
    ("f16-8x2-separate-l2", 8, 2, 2, [150, 30], [100, 0], "f16", "q64w4t1", "separate"),
    ("f16-32x32-fused", 32, 32, 1, [300], [37], "f16", "q64w4t1", "fused"),
    ("f16-32x8-rt2-fused", 32, 8, 1, [512, 300, 1, 40], [0, 37, 128, 256], "f16", "q128w4t2", "fused"),
    ("f16-8x8-rt2-separate", 8, 8, 1, [512, 300, 100, 50, 30, 20, 1, 11], [0, 64, 29, 128, 0, 200, 5, 256], "f16", "q128w4t2", "separate"),
    ("f16-32x8-w8-fused-l2", 32, 8, 2, [640, 128, 1], [37, 0, 128], "f16", "q128w8t1", "fused"),
    ("f16-8x8-w8-separate", 8, 8, 1, [520, 128, 100, 64, 1, 40, 30], [100, 0, 128, 7, 0, 64, 256], "f16", "q128w8t1", "separate"),
    ("e4m3-pow2-8x2-splitk", 8, 2, 1, [64, 1, 45], [0, 128, 37], "pow2", "q64w4t1", "splitk"),
    ("e4m3-np2-8x2-separate-l2", 8, 2, 2, [150, 30], [100, 0], "np2", "q64w4t1", "separate"),
    ("e4m3-np2-32x32-fused", 32, 32, 1, [300], [37], "np2", "q64w4t1", "fused"),
    ("e4m3-np2-8x8-rt2-separate", 8, 8, 1, [512, 300, 100, 50, 30, 20, 1, 11], [0, 64, 29, 128, 0, 200, 5, 256], "np2", "q128w4t2", "separate"),
    ("e4m3-pow2-32x8-rt2-fused", 32, 8, 1, [512, 300, 1, 40], [0, 37, 128, 256], "pow2", "q128w4t2", "fused"),
    ("e4m3-pow2-32x8-w8-fused", 32, 8, 1, [640, 128, 1], [37, 0, 128], "pow2", "q128w8t1", "fused"),
    ("e4m3-np2-8x8-w8-separate", 8, 8, 1, [520, 128, 100, 64, 1, 40, 30], [100, 0, 128, 7, 0, 64, 256], "np2", "q128w8t1", "separate"),
]
IDS = [t[0] for t in TABLE]

ROW_CLASSES = ("row0", "r15", "r16", "r31", "r32", "bq_last", "bq_first", "last", "tail")
SEQ_CLASSES = ("hist0", "hist_not64", "hist_128k", "len1", "len_multiple_bq", "short")
POS_CLASSES = ("diag", "prev", "first", "tile_first", "prev_tile_last", "hist_last", "hist_first", "page_lo", "page_hi", "wg_last_tile",
               "random")


def rope_rows(x, tab, pos, inverse=False):
    """_rope for many rows at once: x [T, heads, HS] float64, row t rotated by the table row pos[t]"""
    half = x.shape[-1] // 2
    c, s = tab[pos, :, 0].astype(np.float64)[:, None, :], tab[pos, :, 1].astype(np.float64)[:, None, :]
    if inverse:
        s = -s
    a, b = x[..., :half], x[..., half:]
    return np.concatenate([a * c - b * s, b * c + a * s], axis=-1)


def owner_rows(ln, bq, rng):
    """query rows of a sequence that get owners: the rows at which the kernel's row tiles, waves and workgroups begin and end"""
    rows = {0, 15, 16, 31, 32, 63, 64, bq - 1, bq, ln - 2, ln - 1}
    if ln % bq:   # a partial tail tile: its first row and one in its middle
        tail0 = (ln // bq) * bq
        rows |= {tail0, (tail0 + ln) // 2}
    rows |= {int(r) for r in rng.integers(0, ln, 2)}
    return sorted(r for r in rows if 0 <= r < ln)


def row_class(ln, bq, i):
    names = [n for n, r in (("row0", 0), ("r15", 15), ("r16", 16), ("r31", 31), ("r32", 32), ("bq_last", bq - 1), ("bq_first", bq),
                            ("last", ln - 1)) if r == i]
    if ln % bq and i >= (ln // bq) * bq:
        names.append("tail")
    return "+".join(names) or "other"


def seq_class(ln, hist, bq, max_q_len):
    names = ["hist0" if hist == 0 else ("hist_128k" if hist % 128 == 0 else ("hist_not64" if hist % 64 else "hist_64k"))]
    names += ["len1"] if ln == 1 else []
    names += ["len_multiple_bq"] if ln % bq == 0 else []
    names += ["short"] if ln <= max_q_len - bq else []   # whole workgroups of the grid (sized for max_q_len) return at once
    return names


def position_classes(hist, ln, i, bq, rng, n_random=2):
    """ordered (class, slot) list for the owner at query row i: the places where the kernel changes behaviour first, random fillers
    last; a slot that belongs to several classes appears once, under the joined name"""
    qpos = hist + i
    q0 = (i // bq) * bq
    t_hi = hist + min(q0 + bq, ln)            # keys the workgroup of row i loads
    last0 = ((t_hi - 1) // BT) * BT           # its last key tile
    pb = (qpos // PAGE) * PAGE
    items = [("diag", qpos), ("prev", qpos - 1), ("first", 0), ("tile_first", (qpos // BT) * BT), ("prev_tile_last", (qpos // BT) * BT - 1),
             ("hist_last", hist - 1), ("hist_first", hist), ("page_lo", pb - 1), ("page_hi", pb if pb else -1), ("page_lo", PAGE - 1),
             ("page_hi", PAGE)]
    if last0 > hist + q0 and qpos >= last0:   # keys that only the later rows of the query tile see
        items.append(("wg_last_tile", last0 + (qpos - last0) // 2))
    items += [("random", int(rng.integers(0, qpos + 1))) for _ in range(n_random)]
    names = {}
    for name, p in items:
        if 0 <= p <= qpos and name not in names.setdefault(p, []):
            names[p].append(name)
    out, seen = [], set()
    for name, p in items:
        if 0 <= p <= qpos and p not in seen:
            seen.add(p)
            out.append(("+".join(names[p]), p))
    return out


class Owner:
    def __init__(self, slot, cls, rowcls):
        self.slot, self.cls, self.rowcls, self.decoy = slot, cls, rowcls, None


class _Seq:
    """what attn_cases.check needs of one sequence of a case: the head size and the words of a failure"""

    def __init__(self, c, s, rows=None):
        self.c, self.s, self.hs, self.rows = c, s, HS, rows

    def describe(self, form, b=None, h=None):
        c, s = self.c, self.s
        text = "case=%s form=%s" % (c.cid, form)
        if b is not None:
            i = int(b if self.rows is None else self.rows[b])
            o = c.owners.get((s, i, h))
            text += " sequence=%d (length %d, history %d) row=%d head=%d class=%s position=%s row_class=%s" % (
                s, c.lens[s], c.hist[s], i, h, o.cls if o else "none", o.slot if o else None, row_class(c.lens[s], c.bq, i))
        return text


class PrefillCase:
    def deq(self, stored, which):
        """a cache as the values the device attends to (fp16 values as they are; e4m3 codes x the scale)"""
        if self.scales is None:
            return np.asarray(stored, np.float32)
        return E4M3[stored] * np.float32(self.scales[which])

    def store(self, values, which):
        return rnd_t(values, F16) if self.scales is None else to_e4m3(np.asarray(values, np.float64) / np.float32(self.scales[which]))

    def extra_atol(self, s):
        """one fp16 ulp of |x| where x != 0: the residual add rounds attention + x once more (element t of packed token t)"""
        a = np.zeros((self.lens[s], self.nh * HS))
        t = np.arange(self.cum[s], self.cum[s + 1])
        a[t - self.cum[s], t] = float(np.spacing(np.float16(X_ONE_HOT)))
        return a

    def plan_words(self):
        return ["attn=" + self.form, "kv=" + ("f16" if self.scales is None else "e4m3"), PRODUCER_PLAN[self.producer]]

    def config(self, llmie):
        ks, vs = self.scales or (0.0, 0.0)
        return dict(head_num=self.nh, kv_head_num=self.kvh, head_size=HS, inter_size=INTER, num_layers=self.L, vocab_size=100,
                    max_seq_len=self.max_seq, max_batch=self.bs, rotary_dim=HS, rotary_base=10000.0, rms_eps=1e-5, dtype=llmie.F16,
                    wfmt=llmie.W_F16, int4_group=128, kv_fmt=llmie.KV_NATIVE if self.scales is None else llmie.KV_FP8, k_scale=ks,
                    v_scale=vs)


def make_case(cid, nh, kvh, L, lens, hist, kv, form, producer, planted=True, rows=None, min_mass=0.9, seed=11):
    """planted=False keeps plain random rows (owners are still chosen, nothing is written for them); rows: the pre-RoPE q/k/v rows
    [L, T, heads, HS] to use instead of drawn ones (today's inputs: what a random model projects)."""
    c = PrefillCase()
    rep, H, heads, bs, T = nh // kvh, nh * HS, nh + 2 * kvh, len(lens), int(sum(lens))
    assert nh % kvh == 0 and len(hist) == bs and all(l >= 1 for l in lens)
    assert rows is not None or (H in (1024, 4096) and T <= H), "one-hot rows need sqrt(H) exact in fp16 and a weight column per token"
    sq = float(np.sqrt(H))
    c.cid, c.nh, c.kvh, c.rep, c.L, c.layer, c.bs, c.T, c.H = cid, nh, kvh, rep, L, L - 1, bs, T, H
    c.lens, c.hist, c.ctx = [int(l) for l in lens], [int(h) for h in hist], [int(l + h) for l, h in zip(lens, hist)]
    c.cum = np.concatenate([[0], np.cumsum(c.lens)]).astype(np.int64)
    c.max_q_len, c.form, c.bq, c.producer, c.kv = max(c.lens), form, FORM_BQ[form], producer, kv
    c.scales = None if kv == "f16" else E4M3_SCALES[kv]
    c.max_seq = -(-(max(c.ctx) + 1) // PAGE) * PAGE      # every context ends before the slab does: room for the decoy past it
    c.seq_classes = [seq_class(l, h, c.bq, c.max_q_len) for l, h in zip(c.lens, c.hist)]
    rng = np.random.default_rng([seed, nh, kvh, L] + c.lens + c.hist)
    c.tab = rope_table(c.max_seq, HS, HS)
    c.seq_of = np.repeat(np.arange(bs), c.lens)
    c.pos_of = np.concatenate([h + np.arange(l) for l, h in zip(c.lens, c.hist)])    # cache slot of every packed token
    # weight columns first (fp16), rows = sqrt(H) x them: q ~ N(0, 1), k, v ~ 0.5 N(0, 1)
    if rows is None:
        sd = np.concatenate([np.ones(nh), np.full(2 * kvh, 0.5)]).astype(np.float32)[None, None, :, None]
        c.w = rnd_t(rng.standard_normal((L, T, heads, HS), dtype=np.float32) * (sd / np.float32(sq)), F16)
        c.rows = c.w * np.float32(sq)
    else:
        c.w, c.rows = None, np.array(rows, np.float32)
    shape = (L, bs, kvh, c.max_seq, HS)
    if c.scales is None:
        c.k0, c.v0 = (rnd_t(rng.standard_normal(shape, dtype=np.float32) * 0.5, F16) for _ in range(2))
    else:   # random codes up to 15 x the scale, either sign (as the e4m3 decode cases)
        c.k0, c.v0 = (rng.integers(0, 0x58, shape, dtype=np.uint8) | (rng.integers(0, 2, shape, dtype=np.uint8) << 7) for _ in range(2))
    c.q_eff = rnd_t(rope_rows(c.rows[c.layer, :, :nh].astype(np.float64), c.tab, c.pos_of), F16).astype(np.float64)

    # ---- owners: every head of the chosen rows, classes cycling; the heads of one KV group own distinct slots
    c.owners, taken, k = {}, set(), 0
    for s in range(bs):
        if c.lens[s] >= 2:   # kept free in KV group 0 for the decoy of row len - 2: the row that clamped keys read (defect "clamp")
            taken.add((s, 0, c.ctx[s] - 1))
        for i in owner_rows(c.lens[s], c.bq, rng):
            items = position_classes(c.hist[s], c.lens[s], i, c.bq, rng, n_random=2 + 2 * rep)
            for h in range(nh):
                for j in range(len(items)):
                    name, p = items[(k + j) % len(items)]
                    if (s, h // rep, p) not in taken:
                        taken.add((s, h // rep, p))
                        c.owners[(s, i, h)] = Owner(p, name, row_class(c.lens[s], c.bq, i))
                        break
                k += 1
    c.by_seq_head = {}
    for (s, i, h), o in c.owners.items():
        c.by_seq_head.setdefault((s, h), []).append((i, o))

    def plant(s, g, slot, q, logit):
        target = q * (logit * np.sqrt(HS) / np.dot(q, q))
        if slot < c.hist[s] or slot >= c.ctx[s]:       # a cache row (history, or the slot just past the context)
            c.k0[c.layer, s, g, slot] = c.store(target, 0)
        else:                                           # a new token: the pre-image goes into its weight column
            t = c.cum[s] + slot - c.hist[s]
            c.w[c.layer, t, nh + g] = rnd_t(_rope(target, c.tab[slot], inverse=True) / sq, F16)
            c.rows[c.layer, t, nh + g] = c.w[c.layer, t, nh + g] * np.float32(sq)

    if planted:
        for (s, i, h), o in c.owners.items():
            plant(s, h // rep, o.slot, c.q_eff[c.cum[s] + i, h], LOGIT)
        # decoys at qpos + 1 on slots no owner uses: every other owner, and the last two rows of every sequence
        for n, ((s, i, h), o) in enumerate(c.owners.items()):
            d = c.hist[s] + i + 1
            kept = h == 0 and i == c.lens[s] - 2
            if kept or ((n % 2 == 0 or i >= c.lens[s] - 2) and (s, h // rep, d) not in taken):
                taken.add((s, h // rep, d))
                o.decoy = d
                plant(s, h // rep, d, c.q_eff[c.cum[s] + i, h], DECOY_LOGIT)

    # ---- the appended rows as the pass stores them, per layer, with the tolerance their arithmetic allows (attn_cases.make_case:
    # RoPE is two roundings of a sum of two products computed in fp32 -> 2 eps (|x| + |partner|); v is copied: exact)
    c.k_new, c.v_new, c.k_tol = [], [], []
    for l in range(L):
        kn, vn = c.rows[l, :, nh:nh + kvh].astype(np.float64), c.rows[l, :, nh + kvh:]
        c.k_new.append(c.store(rnd_t(rope_rows(kn, c.tab, c.pos_of), F16), 0))
        c.v_new.append(c.store(vn, 1))
        c.k_tol.append(2 * EPS[F16] * (np.abs(kn) + np.abs(np.concatenate([kn[..., HS // 2:], kn[..., :HS // 2]], axis=-1))))
    c.k_cpu, c.v_cpu = after_pass(c, c.k0, c.k_new), after_pass(c, c.v0, c.v_new)
    c.ref, c.mass = reference(c, c.deq(c.k_cpu, 0), c.deq(c.v_cpu, 1), with_mass=True)
    if planted:   # a condition on the INPUTS (not a tolerance on the kernel); for e4m3 on the de-quantised values
        assert_mass(c, c.mass, min_mass)
    return c


def assert_mass(c, mass, min_mass=0.9):
    for (s, i, h), m in mass.items():
        assert m >= min_mass, "planted row holds %.3f of the mass: %s" % (m, _Seq(c, s).describe("generator", i, h))


def after_pass(c, cache0, new):
    """the cache after the pass: new[l][t] at [l, sequence of t, :, slot of t], every other slot as before"""
    out = cache0.copy()
    for l in range(c.L):
        out[l, c.seq_of, :, c.pos_of] = new[l]
    return out


DEFECTS = ("mask_plus1", "mask_minus1", "no_history", "drop", "v_next", "v_prev", "clamp", "page_prev", "stale", "layer0")


def _clamp_mult(c, s, i):
    """keys the workgroup of row i reads through the min(t0 + row, ctx - 1) clamp: from t_hi to the end of its last 64-key tile"""
    q0 = (i // c.bq) * c.bq
    return (-(c.hist[s] + np.minimum(q0 + c.bq, c.lens[s]))) % BT


def _v_other(c, s, i, o, defect):
    p = o.slot + (1 if defect == "v_next" else -1)
    p = p if 0 <= p <= c.hist[s] + i else 2 * o.slot - p
    return p if 0 <= p <= c.hist[s] + i else None


def expressible(c, defect, cls=None):
    """can this seeded defect move the reference of this case at an element some owner holds?"""
    own = c.owners.items()
    if defect == "mask_plus1":
        return any(o.decoy is not None for _, o in own)
    if defect == "mask_minus1":
        return any(o.slot == c.hist[s] + i for (s, i, h), o in own)
    if defect == "no_history":
        return any(o.slot > i for (s, i, h), o in own)
    if defect == "drop":
        return any(o.cls == cls for _, o in own)
    if defect in ("v_next", "v_prev"):
        return any(_v_other(c, s, i, o, defect) is not None for (s, i, h), o in own)
    if defect == "clamp":   # the decoy of row len - 2 sits in slot ctx - 1: counted again for every clamped key
        return any(o.decoy == c.ctx[s] - 1 and _clamp_mult(c, s, i) > 0 for (s, i, h), o in own)
    if defect == "page_prev":
        return any(o.slot >= PAGE for _, o in own)
    if defect == "stale":
        return any(o.slot >= c.hist[s] for (s, i, h), o in own)
    if defect == "layer0":
        return c.L > 1
    raise ValueError(defect)


def reference(c, kfull, vfull, defect=None, cls=None, with_mass=False, rows=None):
    """float64 attention of the case on the caches AFTER the pass (values, [L, bs, kvh, max_seq, HS]) -> one [length, nh HS] array per
    sequence (rows: {sequence: row indices} to evaluate a subset).  `defect` seeds one of DEFECTS into it (a deliberately wrong
    reference: the mutation check):
      mask_plus1 / mask_minus1  the mask t <= qpos + 1 / t < qpos;   no_history  the mask t <= i
      drop         the slot of every owner of class `cls` left out;   v_next / v_prev  V of an owner's slot from the slot after / before
      clamp        the keys from t_hi to the end of the workgroup's last tile read as row ctx - 1 and counted
      page_prev    keys from 128 on read one page (128 slots) earlier;   stale  the cache rows from before the pass at the new tokens' slots
      layer0       layer 0's caches instead of the measured layer's"""
    layer = 0 if defect == "layer0" else c.layer
    outs, mass = [], {}
    for s in range(c.bs):
        ln, hist, ctx = c.lens[s], c.hist[s], c.ctx[s]
        sel = np.arange(ln) if rows is None else np.asarray(rows[s], np.int64)
        n = min(ctx + 1, c.max_seq)   # one slot past the context: what a mask that is off by one lets in
        t, qpos = np.arange(n)[None, :], (hist + sel)[:, None]
        vis = {"mask_plus1": t <= qpos + 1, "mask_minus1": t < qpos, "no_history": t <= qpos - hist}.get(defect, t <= qpos)
        local = {int(i): j for j, i in enumerate(sel)}
        out = np.zeros((len(sel), c.nh * HS))
        for g in range(c.kvh):
            K, V = kfull[layer, s, g, :n].astype(np.float64), vfull[layer, s, g, :n].astype(np.float64)
            if defect == "stale":
                K[hist:ctx], V[hist:ctx] = c.deq(c.k0[layer, s, g, hist:ctx], 0), c.deq(c.v0[layer, s, g, hist:ctx], 1)
            if defect == "page_prev":
                src = np.where(t[0] >= PAGE, t[0] - PAGE, t[0])
                K, V = K[src], V[src]
            for h in range(g * c.rep, (g + 1) * c.rep):
                own = [(local[i], i, o) for i, o in c.by_seq_head.get((s, h), []) if i in local]
                S = c.q_eff[c.cum[s] + sel, h] @ K.T / np.sqrt(HS)
                S[~vis] = -np.inf
                if defect == "drop":
                    for j, i, o in own:
                        if o.cls == cls:
                            S[j, o.slot] = -np.inf
                m = S.max(axis=1)
                if defect == "clamp":
                    mult = _clamp_mult(c, s, sel).astype(np.float64)
                    sc = c.q_eff[c.cum[s] + sel, h] @ K[ctx - 1] / np.sqrt(HS)
                    m = np.maximum(m, np.where(mult > 0, sc, -np.inf))
                m = np.where(np.isfinite(m), m, 0.0)
                e = np.exp(S - m[:, None])
                den, num = e.sum(axis=1), e @ V
                if defect == "clamp":
                    ec = mult * np.exp(sc - m)
                    den, num = den + ec, num + ec[:, None] * V[ctx - 1]
                if defect in ("v_next", "v_prev"):
                    for j, i, o in own:
                        p = _v_other(c, s, i, o, defect)
                        if p is not None:
                            num[j] += e[j, o.slot] * (V[p] - V[o.slot])
                out[:, h * HS:(h + 1) * HS] = num / (den + 1e-6)[:, None]
                for j, i, o in own:
                    mass[(s, i, h)] = float(e[j, o.slot] / den[j]) if den[j] > 0 else 0.0
        outs.append(out)
    return (outs, mass) if with_mass else outs


def check_case(got, c, form, exp=None, rows=None, residual=True):
    """attn_cases.check per sequence (got, exp: one array per sequence) against the fp16 attention bound, plus one fp16 ulp of |x| on
    the element the residual add rounds again; the message names case, form, sequence, row, head, class and position.  Returns the
    largest error / bound."""
    exp = c.ref if exp is None else exp
    worst = 0.0
    for s in range(c.bs):
        extra = c.extra_atol(s) if residual else 0.0
        if residual and rows is not None:
            extra = extra[rows[s]]
        worst = max(worst, check(got[s], _Seq(c, s, None if rows is None else rows[s]), form, BOUND, exp=exp[s], extra_atol=extra))
    return worst


def attention_ratio(got, c, exp=None):
    """largest error / bound away from the one element per row that the residual add rounds again (there the fp16 rounding of
    64 + attention alone is up to 0.48 of the bound, which hides the figure that tells how close the kernel is)"""
    exp = c.ref if exp is None else exp
    worst = 0.0
    for s in range(c.bs):
        r = np.abs(np.asarray(got[s], np.float64) - exp[s]) / (BOUND[1] + BOUND[0] * np.abs(exp[s]))
        worst = max(worst, float(r[c.extra_atol(s) == 0].max()))
    return worst


def build(entry, **kw):
    return make_case(*entry, **kw)


# ------------------------------------------------------------------------- the oracle's composition of the same attention
def oracle_rows(c, n_random=8, seed=3):
    """{sequence: rows} the CPU composition evaluates: every owner row and a few others (the whole K / V context for each)"""
    rng = np.random.default_rng(seed)
    return {s: np.array(sorted({i for (s_, i, h) in c.owners if s_ == s} | {int(r) for r in rng.integers(0, c.lens[s], n_random)}))
            for s in range(c.bs)}


def oracle_composition(c, rows):
    """the attention of the measured layer as the oracle's kernels compose it (qkv_bias_transpose_rope -> concat_kv -> repeat_kv ->
    batched_gemm -> scale_mask_softmax -> batched_gemm), one sequence at a time, for the query rows `rows`; fp16 (e4m3 for the
    cache) roundings where the device rounds: q and the rows it stores, and the output"""
    import oracle as orc
    h16 = lambda a: rnd_t(a, F16)
    outs = []
    for s in range(c.bs):
        ln, hist, ctx = c.lens[s], c.hist[s], c.ctx[s]
        sl = slice(c.cum[s], c.cum[s + 1])
        q, k, v = orc.qkv_bias_transpose_rope(c.rows[c.layer, sl], None, np.zeros(ln, np.int32), [hist], 1, ln, c.nh, c.kvh, HS, HS, 10000.0)
        q, k, v = h16(q), c.deq(c.store(h16(k), 0), 0), c.deq(c.store(h16(v), 1), 1)
        kc = np.array(c.deq(c.k0[c.layer:c.layer + 1, s:s + 1], 0), np.float32, order="C")   # (copies: concat_kv writes in place)
        vc = np.array(c.deq(c.v0[c.layer:c.layer + 1, s:s + 1], 1), np.float32, order="C")
        orc.concat_kv(k, kc, [ln], [hist], 0)
        orc.concat_kv(v, vc, [ln], [hist], 0)
        kr, vr = orc.repeat_kv(kc, [ctx], 0, c.nh, ctx), orc.repeat_kv(vc, [ctx], 0, c.nh, ctx)
        sel = rows[s]
        mask = (np.arange(ctx)[None, None, :] <= (hist + sel)[None, :, None]).astype(np.float32)
        p = orc.scale_mask_softmax(orc.batched_gemm(np.ascontiguousarray(q[:, :, sel]), kr, True), mask, 1.0 / np.sqrt(HS))
        av = h16(orc.batched_gemm(p, vr, False))[0]            # [nh, rows, HS]
        outs.append(av.transpose(1, 0, 2).reshape(len(sel), c.nh * HS))
    return outs
