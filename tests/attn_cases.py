"""Decode-attention cases whose inputs can fail: one generator shared by tests/test_decode_attn_cases_cpu.py (the tests of
the tests) and tests/test_decode_attn_gpu.py (the kernels).  Plain module, no fixtures.

Why: with q ~ N(0,1) and k, v ~ 0.5 N(0,1) the softmax over a long context is nearly uniform and the output is a mean of
`step` random rows; one missing row or two exchanged V rows move it by less than the fp16 bound.  Here every (sequence, query
head) owns ONE cache position p whose K row is c * q_eff, with c chosen so that the scaled logit is `logit` (12) over a
background of +-0.5: that row holds >= 0.9 of the softmax mass, the output is essentially V[p], and reading any other row, or
not reading this one, is an O(0.5) error.  The positions are not random: they cycle through the places where the split-KV
kernel changes behaviour (see position_classes).

Reference (reference()): numpy float64 on the inputs as rounded to the dtype under test,
    q_eff = [round_T(RoPE(q, step - 1))] + bias_q,   row step-1 = the appended token (round_T(round_T(RoPE(k)) + bias_k), round_T(v +
    bias_v): what is stored is what is attended to),   out = sum_t e_t V_t / (sum_t e_t + 1e-6),  e_t = exp(l_t - max l).
The 1e-6 in the denominator is the library's (and the project it was modelled on); sum e_t >= 1, so it is a relative 1e-6 at
most: below every bound used here.
"""
import functools

import numpy as np

F16, F32 = "f16", "f32"
NP_T = {F16: np.float16, F32: np.float32}
# (rtol, atol) the project already holds these entries to (tests/test_kernels_gpu.py); "rope" also covers the ragged entry
BOUNDS = {"plain": {F32: (1e-4, 1e-5), F16: (3e-3, 2e-3)}, "rope": {F32: (2e-4, 2e-5), F16: (3e-3, 2e-3)}}
EPS = {F16: 2.0 ** -10, F32: 2.0 ** -23}   # largest relative spacing of the format
KV_PAGE = 128


def rnd_t(a, dtype):
    """values rounded to the dtype under test, as float32"""
    return np.asarray(a, np.float32).astype(NP_T[dtype]).astype(np.float32)


def chunk_len(dtype, hs, e4m3=False):
    """tokens per chunk of the split kernel: 4 waves x 8 loads x (64 lanes / lanes per token row)"""
    per16 = 16 if e4m3 else (8 if dtype == F16 else 4)
    return 4 * 8 * (64 // (hs // per16))


def rope_table(max_pos, hs, rot, base=10000.0):
    """[max_pos, hs/2, 2] fp32 (cos, sin); dims >= rot/2 are the identity"""
    j = np.arange(hs // 2, dtype=np.float32)
    inv = np.power(np.float32(base), (2 * j) / np.float32(rot)).astype(np.float32)
    ang = (np.arange(max_pos, dtype=np.float32)[:, None] / inv[None, :]).astype(np.float32)
    tab = np.stack([np.cos(ang), np.sin(ang)], axis=-1).astype(np.float32)
    tab[:, rot // 2:, 0], tab[:, rot // 2:, 1] = 1.0, 0.0
    return tab


def _rope(x, cs, inverse=False):
    """rotate-half pairs (d, d + hs/2) of the last axis of x (float64) by the table row cs [hs/2, 2]"""
    half = x.shape[-1] // 2
    c, s = cs[:, 0].astype(np.float64), cs[:, 1].astype(np.float64)
    if inverse:
        s = -s
    a, b = x[..., :half], x[..., half:]
    return np.concatenate([a * c - b * s, b * c + a * s], axis=-1)


def position_classes(step, chunk, rng, extra=(), n_random=3):
    """Ordered list of (class name, position) for a context of `step` tokens (the appended one included) cut into chunks of
    `chunk` tokens: the places where the kernel changes behaviour first, random fillers last.  A position that belongs to
    several classes appears once, under the joined name."""
    s, C = step, chunk
    last0 = ((s - 1) // C) * C
    items = [("first", 0), ("new", s - 1), ("prev", s - 2), ("last_chunk_first", last0), ("last_chunk_last", s - 1),
             ("chunk0_last", C - 1), ("chunk1_first", C), ("split16_first", 16 * C)]
    if C > KV_PAGE:   # both sides of every page boundary inside the first, a middle and the last chunk
        for base in sorted({0, (last0 // C // 2) * C, last0}):
            for t in range(base + KV_PAGE, base + C, KV_PAGE):
                items += [("page_lo", t - 1), ("page_hi", t)]
    items += list(extra)
    items += [("random", int(rng.integers(0, s))) for _ in range(n_random)]
    names = {}
    for name, p in items:
        if 0 <= p < s:
            if name not in names.setdefault(p, []):
                names[p].append(name)
    out, seen = [], set()
    for name, p in items:
        if 0 <= p < s and p not in seen:
            seen.add(p)
            out.append(("+".join(names[p]), p))
    return out


def _ragged_order(items, b):
    new = [i for i in items if "new" in i[0]]
    lo = [i for i in items if "page_lo" in i[0] and "new" not in i[0]]
    hi = [i for i in items if "page_hi" in i[0] and "new" not in i[0]]
    head = new + ([lo[b % len(lo)]] if lo else []) + ([hi[b % len(hi)]] if hi else [])
    rest = [i for i in items if i not in head]
    k = (5 * b) % len(rest) if rest else 0
    return head + rest[k:] + rest[:k]


@functools.lru_cache(maxsize=1)
def _background(dtype, L, bs, kvh, max_seq, hs, seed):
    rng = np.random.default_rng(seed)
    shape = (L, bs, kvh, max_seq, hs)
    return (rnd_t(rng.standard_normal(shape, dtype=np.float32) * 0.5, dtype),
            rnd_t(rng.standard_normal(shape, dtype=np.float32) * 0.5, dtype))


class Case:
    """inputs (float32 arrays holding values of the dtype under test), owners and the float64 reference of one call"""

    def describe(self, form, b=None, h=None):
        s = "dtype=%s head_size=%d ratio=%d step=%s form=%s" % (self.dtype, self.hs, self.rep,
                                                                 self.steps[0] if self.uniform else self.steps, form)
        if b is not None:
            s += " b=%d h=%d step[b]=%d position=%s class=%s" % (b, h, self.steps[b], self.pos[b][h], self.cls[b][h])
        return s


def make_case(dtype, hs, nh, kvh, bs, steps, max_seq, chunk, L=1, layer=0, bias=False, rope=False, rot=None, logit=12.0,
              seed=0, planted=True, extra=None, min_mass=0.9):
    """steps: one int (the whole batch at one position) or one per sequence.  chunk: chunk length of the kernel that will run
    (drives the position classes only).  extra(step) -> more (class, position) pairs.  planted=False keeps today's plain random
    caches (positions are still chosen, nothing is written there): used to show what such inputs cannot detect."""
    c = Case()
    uniform = isinstance(steps, (int, np.integer))
    steps = [int(steps)] * bs if uniform else [int(s) for s in steps]
    assert len(steps) == bs and all(1 <= s <= max_seq for s in steps) and nh % kvh == 0 and 0 <= layer < L
    rep = nh // kvh
    rot = hs if rot is None else rot
    rng = np.random.default_rng([seed, hs, nh, kvh, bs, max_seq, int(rope), int(bias)] + steps)
    c.dtype, c.hs, c.nh, c.kvh, c.rep, c.bs, c.L, c.layer = dtype, hs, nh, kvh, rep, bs, L, layer
    c.steps, c.uniform, c.max_seq, c.chunk, c.rope, c.rot, c.logit = steps, uniform, max_seq, chunk, rope, rot, logit
    qkv = rnd_t(rng.standard_normal((bs, nh + 2 * kvh, hs)), dtype)
    c.bias = rnd_t(rng.standard_normal(((nh + 2 * kvh) * hs,)) * 0.3, dtype) if bias else None
    bias3 = (c.bias if bias else np.zeros((nh + 2 * kvh) * hs, np.float32)).reshape(nh + 2 * kvh, hs).astype(np.float64)
    bq, bk, bv = bias3[:nh], bias3[nh:nh + kvh], bias3[nh + kvh:]
    kb, vb = _background(dtype, L, bs, kvh, max_seq, hs, seed)
    kc, vc = kb.copy(), vb.copy()   # slot step - 1 keeps its random row: the decoy behind the appended token
    c.tab = rope_table(max_seq, hs, rot) if rope else None

    def rot_fwd(x, b):   # as the unfused RoPE kernel stores it: rotated, rounded to T
        return rnd_t(_rope(x, c.tab[steps[b] - 1]), dtype).astype(np.float64) if rope else x

    # what the kernel dots with K
    q_eff = np.stack([rot_fwd(qkv[b, :nh].astype(np.float64), b) + bq for b in range(bs)])
    c.pos = [[None] * nh for _ in range(bs)]
    c.cls = [["none"] * nh for _ in range(bs)]
    c.classes = []
    for b in range(bs):
        items = position_classes(steps[b], chunk, rng, extra(steps[b]) if extra else ())
        c.classes.append(items)
        if not uniform:   # 8 owners per sequence: the appended token and one page boundary always, the rest rotated by sequence
            items = _ragged_order(items, b)
        used = [set() for _ in range(kvh)]
        for h in range(nh):
            g = h // rep
            start = ((b * nh if uniform else 0) + h) % len(items)
            for k in range(len(items)):   # the REP heads of one KV head get distinct positions (while there are any left)
                name, p = items[(start + k) % len(items)]
                if p not in used[g]:
                    used[g].add(p)
                    c.pos[b][h], c.cls[b][h] = p, name
                    break
        if not uniform:
            owned = "+".join(c.cls[b])
            assert "new" in owned and (("page_lo" in owned and "page_hi" in owned) or not any("page_hi" in n for n, _ in items))
    if uniform and bs * nh >= sum(n != "random" for n, _ in c.classes[0]):   # every class of the case has an owner
        owned = {c.pos[b][h] for b in range(bs) for h in range(nh)}
        assert owned >= {p for name, p in c.classes[0] if name != "random"}, (steps[0], c.classes[0], c.pos)
    if planted:
        for b in range(bs):
            for h in range(nh):
                p, g = c.pos[b][h], h // rep
                if p is None:
                    continue
                target = q_eff[b, h] * (logit * np.sqrt(hs) / np.dot(q_eff[b, h], q_eff[b, h]))
                if p == steps[b] - 1:   # the appended token: its pre-image goes into the qkv row, the cache slot keeps the decoy
                    pre = target - bk[g]
                    qkv[b, nh + g] = rnd_t(_rope(pre, c.tab[p], inverse=True) if rope else pre, dtype)
                else:
                    kc[layer, b, g, p] = rnd_t(target, dtype)
    c.qkv, c.kc, c.vc = qkv, kc, vc
    # the appended rows, as stored (and attended to), with the tolerance their arithmetic allows: exact without bias / RoPE; one
    # rounding of an exactly representable sum with bias (1 ulp covers a double rounding); with RoPE two roundings of a sum of
    # three products / terms computed in fp32: 2 eps (|x| + |partner| + |bias|)
    kn, vn = qkv[:, nh:nh + kvh].astype(np.float64), qkv[:, nh + kvh:].astype(np.float64)
    c.k_new = np.stack([rnd_t(rot_fwd(kn[b], b) + bk, dtype) for b in range(bs)]).astype(np.float64)
    c.v_new = rnd_t(vn + bv, dtype).astype(np.float64)
    half = hs // 2
    partner = np.concatenate([kn[..., half:], kn[..., :half]], axis=-1)
    c.k_tol = 2 * EPS[dtype] * (np.abs(kn) + np.abs(partner) + np.abs(bk)) if rope else \
        (EPS[dtype] * np.abs(c.k_new) if bias else np.zeros_like(c.k_new))
    c.v_tol = EPS[dtype] * np.abs(c.v_new) if bias else np.zeros_like(c.v_new)
    c.q_eff = q_eff
    c.ref, mass = reference(c, with_mass=True)
    c.mass = mass
    if planted:   # a condition on the INPUTS (not a tolerance on the kernel): the planted row owns the softmax in every head
        for b in range(bs):
            for h in range(nh):
                if c.pos[b][h] is not None:
                    assert mass[b][h] >= min_mass, "planted row holds %.3f of the mass: %s" % (mass[b][h], c.describe("generator", b, h))
    return c


DEFECTS = ("drop", "v_next", "v_prev", "trunc_last", "stale_new", "ignore_split16", "page0")


def expressible(c, defect, cls=None):
    """can this seeded defect change the reference of this case at a row some head owns?"""
    owners = [(b, h) for b in range(c.bs) for h in range(c.nh) if c.pos[b][h] is not None]
    if defect == "drop":
        return any(c.cls[b][h] == cls for b, h in owners)
    if defect in ("v_next", "v_prev"):
        return any(c.steps[b] >= 2 for b, h in owners)
    if defect in ("trunc_last", "stale_new"):
        return any(c.pos[b][h] == c.steps[b] - 1 for b, h in owners)
    if defect == "ignore_split16":
        return any(c.pos[b][h] >= 16 * c.chunk for b, h in owners)
    if defect == "page0":
        return c.chunk > KV_PAGE and any((c.pos[b][h] % c.chunk) >= KV_PAGE for b, h in owners)
    raise ValueError(defect)


def reference(c, defect=None, cls=None, with_mass=False):
    """float64 attention of the case; `defect` seeds one of DEFECTS into it (a deliberately wrong reference: the mutation check)"""
    out = np.zeros((c.bs, c.nh * c.hs))
    mass = [[0.0] * c.nh for _ in range(c.bs)]
    for b in range(c.bs):
        s = c.steps[b]
        for g in range(c.kvh):
            K = c.kc[c.layer, b, g, :s].astype(np.float64)
            V = c.vc[c.layer, b, g, :s].astype(np.float64)
            if defect != "stale_new":
                K[s - 1], V[s - 1] = c.k_new[b, g], c.v_new[b, g]
            if defect == "page0":   # rows of page j > 0 of a chunk read from the chunk's first page
                t = np.arange(s)
                src = np.where((t % c.chunk) >= KV_PAGE, (t // c.chunk) * c.chunk + t % KV_PAGE, t)
                K, V = K[src], V[src]
            for h in range(g * c.rep, (g + 1) * c.rep):
                p = c.pos[b][h]
                lg = K @ c.q_eff[b, h] / np.sqrt(c.hs)
                Vh = V
                if defect == "drop" and c.cls[b][h] == cls:
                    lg[p] = -np.inf
                if defect == "trunc_last":
                    lg[s - 1] = -np.inf
                if defect == "ignore_split16":
                    lg[16 * c.chunk:] = -np.inf
                if defect in ("v_next", "v_prev") and s >= 2 and p is not None:
                    o = p + (1 if defect == "v_next" else -1)
                    o = o if 0 <= o < s else 2 * p - o
                    Vh = V.copy()
                    Vh[p] = V[o]
                m = lg.max()
                e = np.exp(lg - m) if np.isfinite(m) else np.zeros_like(lg)
                out[b, h * c.hs:(h + 1) * c.hs] = e @ Vh / (e.sum() + 1e-6)
                if p is not None and e.sum() > 0:
                    mass[b][h] = float(e[p] / e.sum())
    return (out, mass) if with_mass else out


def check(got, c, form, bounds, exp=None, extra_atol=0.0):
    """the comparison of every test here: |got - ref| <= atol + rtol |ref| element-wise (NaN fails); the message names the case
    and the owner of the worst element.  Returns the largest error / bound."""
    rtol, atol = bounds
    exp = c.ref if exp is None else exp
    got = np.asarray(got, np.float64).reshape(exp.shape)
    err = np.abs(got - exp)
    ratio = err / (atol + rtol * np.abs(exp) + extra_atol)
    bad = ~(ratio <= 1.0)
    if bad.any():
        score = np.where(np.isnan(ratio), np.inf, ratio)
        b, k = np.unravel_index(np.argmax(score), score.shape)
        h, d = divmod(int(k), c.hs)
        raise AssertionError("%s dim=%d: got %r expected %r (error / bound %.3g, %d elements out of bound)" % (
            c.describe(form, int(b), h), d, float(got[b, k]), float(exp[b, k]), float(score[b, k]), int(bad.sum())))
    return float(ratio.max())


# --------------------------------------------------------------------------------------------------------------- the case table
NH = 8
# (head_size, head_num / kv_head_num, batch, L, layer, bias, max_seq a multiple of 128).  Every head size with ratio 1 and one GQA
# ratio, every ratio at 128; batch 3 where a chunk spans several pages (more owners for the page-boundary classes)
GEOMETRIES = [(32, 1, 3, 1, 0, False, False), (32, 4, 3, 1, 0, True, True),
              (64, 1, 3, 1, 0, True, False), (64, 2, 3, 1, 0, False, True),
              (128, 1, 2, 2, 1, False, False), (128, 2, 2, 1, 0, True, True), (128, 4, 3, 1, 0, False, False),
              (128, 8, 2, 1, 0, True, True),
              (256, 1, 2, 1, 0, True, False), (256, 2, 2, 2, 1, False, True)]
GEOMETRIES_F32_ONLY = [(256, 8, 2, 1, 0, True, False)]   # 8 query heads x a whole wave per row: register pressure


def geometries(dtype):
    return GEOMETRIES + (GEOMETRIES_F32_ONLY if dtype == F32 else [])


def max_seq_of(dtype, hs, round128):
    m = 17 * chunk_len(dtype, hs) + 37
    return -(-m // 128) * 128 if round128 else m


def sweep(dtype, hs, round128):
    C, m = chunk_len(dtype, hs), max_seq_of(dtype, hs, round128)
    return sorted({1, 2, C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1, 127, 128, 129, 16 * C - 1, 16 * C, 16 * C + 1, 17 * C + 1, m})


def geo_id(dtype, geo):
    return "%s-hs%d-r%d" % (dtype, geo[0], geo[1])


def uniform_cases():
    """[(id, dtype, geometry, step, logit)]"""
    out = []
    for dtype in (F16, F32):
        for geo in geometries(dtype):
            for step in sweep(dtype, geo[0], geo[6]):
                out.append(("%s-step%d" % (geo_id(dtype, geo), step), dtype, geo, step, 12.0))
    # logit 40: the partials of every other split are rescaled by exp(-40)
    for dtype, geo in ((F16, GEOMETRIES[4]), (F32, GEOMETRIES[3]), (F16, GEOMETRIES[1])):
        step = 17 * chunk_len(dtype, geo[0]) + 1
        out.append(("%s-step%d-logit40" % (geo_id(dtype, geo), step), dtype, geo, step, 40.0))
    return out


def ragged_cases():
    """[(id, dtype, geometry, steps)]: the sequences of a batch at DIFFERENT steps of the sweep (strided, so that short and long
    contexts share a launch)"""
    out = []
    for dtype in (F16, F32):
        for geo in geometries(dtype):
            sw, bs = sweep(dtype, geo[0], geo[6]), geo[2]
            nb = -(-len(sw) // bs)
            for i in range(nb):
                steps = [sw[(i + j * nb) % len(sw)] for j in range(bs)]
                out.append(("%s-steps%s" % (geo_id(dtype, geo), "_".join(map(str, steps))), dtype, geo, steps))
    return out


# the generic kernel (any head size / ratio): ratio 3, and hs = 4 from the unit test of the project this one was modelled on.
# (head_size, head_num, kv_head_num, batch, bias); it strides the context by its 256 threads
GENERIC = [(64, 6, 2, 2, True), (4, 2, 2, 2, False)]
GENERIC_STEPS = [1, 2, 255, 256, 257, 1000]
GENERIC_MAX_SEQ = 1000


def generic_cases():
    return [("%s-hs%d-nh%d-kvh%d-step%d" % (dtype, g[0], g[1], g[2], step), dtype, g, step)
            for dtype in (F16, F32) for g in GENERIC for step in GENERIC_STEPS]


def build_uniform(dtype, geo, step, logit=12.0, rope=False, planted=True):
    hs, ratio, bs, L, layer, bias, r128 = geo
    return make_case(dtype, hs, NH, NH // ratio, bs, step, max_seq_of(dtype, hs, r128), chunk_len(dtype, hs), L=L, layer=layer,
                     bias=bias, rope=rope, rot=hs if ratio != 2 else hs // 2, logit=logit, seed=7, planted=planted)


def build_ragged(dtype, geo, steps):
    hs, ratio, bs, L, layer, bias, r128 = geo
    return make_case(dtype, hs, NH, NH // ratio, bs, steps, max_seq_of(dtype, hs, r128), chunk_len(dtype, hs), L=L, layer=layer,
                     bias=bias, rope=True, rot=hs if ratio != 2 else hs // 2, seed=7)


def build_generic(dtype, g, step):
    hs, nh, kvh, bs, bias = g
    return make_case(dtype, hs, nh, kvh, bs, step, GENERIC_MAX_SEQ, 256, bias=bias, seed=9)


# ------------------------------------------------------------------------------------- fp16 activations over an e4m3 KV cache
# Only reachable through the engine: a one-layer Decoder with o = identity and gate_up = 0 (the FFN then adds exactly 0 and
# hidden_out - x is the attention output, rounded once more with the residual).  Cache bytes = e4m3(x / scale).
def _e4m3_table():
    vals = []
    for b in range(256):
        s, e, m = b >> 7, (b >> 3) & 0xF, b & 7
        v = np.nan if (e == 15 and m == 7) else ((m / 8.0) * 2.0 ** -6 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7))
        vals.append(-v if s else v)
    return np.array(vals, np.float32)


E4M3 = _e4m3_table()


def to_e4m3(x):
    """round to nearest even, saturating at 448"""
    pos = E4M3[:127]
    x = np.asarray(x, np.float64)
    a = np.minimum(np.abs(x), 448.0)
    idx = np.clip(np.searchsorted(pos, a), 1, 126)
    lo, hi = pos[idx - 1].astype(np.float64), pos[idx].astype(np.float64)
    pick_hi = (a - lo > hi - a) | ((a - lo == hi - a) & (idx % 2 == 0))
    code = np.where(pick_hi, idx, idx - 1).astype(np.uint8)
    code = np.where(a == 0, 0, code).astype(np.uint8)
    return code | (np.signbit(x).astype(np.uint8) << 7)


class _Deq:
    """a byte cache seen as the values the device attends to (de-quantised on access: the whole cache never exists in fp32)"""

    def __init__(self, codes, scale):
        self.codes, self.scale = codes, np.float32(scale)

    def __getitem__(self, idx):
        return E4M3[self.codes[idx]] * self.scale


E4M3_SCALES = {"pow2": (1.0 / 32, 1.0 / 16), "np2": (0.037, 0.021)}
E4M3_KVH = 8
E4M3_NEW_GROUPS = (0, 3)   # KV heads whose K weight rows are c0 x the Q rows of the group's first head
# aimed at for the appended token.  |q|^2 varies by sequence (+-18 % at hs 64), so the logit does: 24 keeps the lowest above the 10.5
# that 0.9 of the mass needs at 4097 tokens.  The other heads of such a group see that row at c0 q.q' / sqrt(hs), up to ~10: their
# planted rows get 18 instead of 12.
E4M3_NEW_LOGIT = 24.0
E4M3_SHARED_GROUP_LOGIT = 18.0


def e4m3_cpw(bs):
    """chunks one workgroup walks through (launch_split): a function of batch x kv heads"""
    cpw = 1
    while cpw < 8 and bs * E4M3_KVH >= 128 * cpw:
        cpw *= 2
    return cpw


def e4m3_cases():
    """[(id, head_size, ratio, batch, scale pair, step)]: batches 2 / 16 / 64 = 1 / 2 / 8 chunks per workgroup; steps around 1, 2 and
    8 chunk lengths and around cpw * C (the large batches run a subset: their float64 reference is seconds per case)"""
    out = []
    for hs in (128, 64):
        C = chunk_len(F16, hs, e4m3=True)
        for ratio in (1, 4):
            for bs in (2, 16, 64):
                S = e4m3_cpw(bs) * C
                steps = {2: {1, 2, C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1, 8 * C - 1, 8 * C, 8 * C + 1, 8 * C + 37},
                         16: {2, C, C + 1, S - 1, S, S + 1, 8 * C + 1}, 64: {1, C + 1, 2 * C, S - 1, S, S + 1}}[bs]
                for sc in E4M3_SCALES:
                    for step in sorted(steps):
                        out.append(("e4m3-hs%d-r%d-b%d-%s-step%d" % (hs, ratio, bs, sc, step), hs, ratio, bs, sc, step))
    return out


def e4m3_max_seq(hs):
    return 8 * chunk_len(F16, hs, e4m3=True) + 37


@functools.lru_cache(maxsize=1)
def e4m3_model(hs, ratio, bs):
    """weights (fp16 values), x and the pre-RoPE qkv of the CPU composition for one configuration"""
    import oracle as orc
    nh, kvh = E4M3_KVH * ratio, E4M3_KVH
    H, QKV, I = nh * hs, (nh + 2 * kvh) * hs, 256   # (half of the down matrix; the engine's batch paths need I >= 512)
    rng = np.random.default_rng([31, hs, ratio, bs])
    u = lambda shape, s: rnd_t(rng.uniform(-1, 1, shape) * s, F16)
    w = dict(attn_norm=rnd_t(u((H,), 0.2) + 1, F16), qkv=u((QKV, H), 2 / np.sqrt(H)), ffn_norm=rnd_t(u((H,), 0.2) + 1, F16),
             down=u((H, I), 2 / np.sqrt(I)), I=I)
    x = rnd_t(rng.standard_normal((bs, H)) / 16, F16)
    w["down"], w["I"] = np.concatenate([w["down"], u((H, I), 2 / np.sqrt(I))], axis=1), 2 * I
    hn = rnd_t(orc.rmsnorm(x, w["attn_norm"], 1e-5)[0], F16)
    q = orc.linear(hn, w["qkv"][:nh * hs]).reshape(bs, nh, hs)
    c0 = E4M3_NEW_LOGIT * np.sqrt(hs) / float(np.mean(np.sum(q.astype(np.float64) ** 2, axis=-1)))
    for g in E4M3_NEW_GROUPS:   # k_new = c0 q before RoPE, so the logit is the same after it
        w["qkv"][(nh + g) * hs:(nh + g + 1) * hs] = rnd_t(c0 * w["qkv"][g * ratio * hs:(g * ratio + 1) * hs], F16)
    pre = rnd_t(orc.linear(hn, w["qkv"]), F16).reshape(bs, nh + 2 * kvh, hs)
    return w, x, pre


@functools.lru_cache(maxsize=1)
def _e4m3_background(hs, bs):
    rng = np.random.default_rng([32, hs, bs])
    shape = (1, bs, E4M3_KVH, e4m3_max_seq(hs), hs)
    codes = lambda: rng.integers(0, 0x58, shape, dtype=np.uint8) | (rng.integers(0, 2, shape, dtype=np.uint8) << 7)
    return codes(), codes()


def make_case_e4m3(hs, ratio, bs, sc, step, logit=12.0):
    """The case of one engine step.  q_eff and the appended rows come from the CPU composition (oracle kernels, fp16 roundings
    where the device rounds); planted rows are e4m3(c q_eff / k_scale) bytes.  Call finish_e4m3 to get the reference."""
    import oracle as orc
    ks, vs = E4M3_SCALES[sc]
    nh, kvh = E4M3_KVH * ratio, E4M3_KVH
    C = chunk_len(F16, hs, e4m3=True)
    S = e4m3_cpw(bs) * C
    w, x, pre = e4m3_model(hs, ratio, bs)
    qkv = rnd_t(orc.rope_decode(pre, nh, kvh, hs, step, hs, 10000.0), F16)
    c = Case()
    c.dtype, c.hs, c.nh, c.kvh, c.rep, c.bs, c.L, c.layer = F16, hs, nh, kvh, ratio, bs, 1, 0
    c.steps, c.uniform, c.max_seq, c.chunk, c.rope, c.logit = [step] * bs, True, e4m3_max_seq(hs), C, True, logit
    c.weights, c.x, c.scales, c.cpw = w, x, (ks, vs), S // C
    c.q_eff = qkv[:, :nh].astype(np.float64)
    c.k_codes_new, c.v_codes_new = to_e4m3(qkv[:, nh:nh + kvh] / np.float32(ks)), to_e4m3(qkv[:, nh + kvh:] / np.float32(vs))
    kb, vb = _e4m3_background(hs, bs)
    kq = kb.copy()
    rng = np.random.default_rng([33, hs, ratio, bs, step])
    c.pos = [[None] * nh for _ in range(bs)]
    c.cls = [["none"] * nh for _ in range(bs)]
    k = 0
    for b in range(bs):
        items = position_classes(step, C, rng, [("span0_last", S - 1), ("span1_first", S)])
        new_name = [n for n, p in items if p == step - 1][0]
        rest = [i for i in items if i[1] != step - 1]
        used = [set() for _ in range(kvh)]
        for h in range(nh):
            g = h // ratio
            if g in E4M3_NEW_GROUPS and h % ratio == 0:   # this head's appended token carries its logit through the weights
                c.pos[b][h], c.cls[b][h] = step - 1, new_name
                continue
            for j in range(len(rest)):
                name, p = rest[(k + j) % len(rest)]
                if p not in used[g]:
                    used[g].add(p)
                    c.pos[b][h], c.cls[b][h] = p, name
                    lg = max(logit, E4M3_SHARED_GROUP_LOGIT) if g in E4M3_NEW_GROUPS else logit
                    target = c.q_eff[b, h] * (lg * np.sqrt(hs) / np.dot(c.q_eff[b, h], c.q_eff[b, h]))
                    kq[0, b, g, p] = to_e4m3(target / ks)
                    break
            k += 1
    c.kq, c.vq = kq, vb
    c.kc, c.vc = _Deq(kq, ks), _Deq(vb, vs)
    return c


def finish_e4m3(c, k_codes_new=None, v_codes_new=None, min_mass=0.9):
    """float64 reference on the de-quantised cache, with the appended rows given as codes (default: the CPU composition's)"""
    ks, vs = c.scales
    c.k_new = (E4M3[c.k_codes_new if k_codes_new is None else k_codes_new] * np.float32(ks)).astype(np.float64)
    c.v_new = (E4M3[c.v_codes_new if v_codes_new is None else v_codes_new] * np.float32(vs)).astype(np.float64)
    c.ref, c.mass = reference(c, with_mass=True)
    for b in range(c.bs):
        for h in range(c.nh):
            if c.pos[b][h] is not None:
                assert c.mass[b][h] >= min_mass, "planted row holds %.3f of the mass: %s" % (c.mass[b][h], c.describe("generator", b, h))
    return c


def e4m3_extra_atol(c):
    """one fp16 ulp of |x| per element: the residual add rounds attention + x once more"""
    return np.spacing(np.abs(c.x).astype(np.float16)).astype(np.float64)


def e4m3_cpu_composition(c):
    """hidden_out - x of the one-layer engine as the oracle's kernels compose it, fp16 roundings where the device applies them"""
    import oracle as orc
    ks, vs = c.scales
    h = lambda a: rnd_t(a, F16)
    out = np.empty((c.bs, c.nh * c.hs), np.float32)
    for b in range(c.bs):   # one sequence at a time: the de-quantised cache of a whole batch would be 0.5 GB
        qkv = np.concatenate([c.q_eff[b].astype(np.float32), E4M3[c.k_codes_new[b]] * np.float32(ks),
                              E4M3[c.v_codes_new[b]] * np.float32(vs)])[None]
        kc, vc = np.ascontiguousarray(c.kc[:, b:b + 1]), np.ascontiguousarray(c.vc[:, b:b + 1])
        mha = h(orc.decoder_mha(qkv, None, kc, vc, 0, c.nh, c.kvh, c.hs, c.steps[b]))
        out[b] = h(mha + c.x[b:b + 1]) - c.x[b]   # o = identity is exact; the FFN adds exactly 0
    return out
