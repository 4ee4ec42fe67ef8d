"""Tree-attention cases whose inputs can fail: one generator shared by tests/test_spec_tree_cpu.py (the tests of the tests) and
tests/test_spec_tree_attn_gpu.py (the TREE instantiations of prefill_rope_append_kernel and prefill_flash_kernel).  Plain module,
no fixtures; the planted-row method and the helpers are those of tests/prefill_attn_cases.py.

The case is a Decoder whose QKV weight columns dictate every token's q / k / v row (attn_norm = 1, o = identity in the measured
layer and 0 in front of it, gate_up = 0, one-hot hidden rows), with a draft tree set: position i of a sequence is node i, rotated
at history + depth_i, stored at slot history + i, and it sees the history and its own ancestors.  Every sequence of a case carries
the same tree on another history (0, 37, 128: history + n crosses a 64-key tile and a 128-token page).

Owners and decoys.  A (node, head) pair that is an OWNER gets one visible key slot -- its parent's, the root's, the last history
row, history row 0 or its own, cycling -- whose K row is aligned with its query at a scaled logit of 12: that slot holds >= 0.9 of
the softmax mass (asserted here, in float64).  Where the tree has one, the owner also gets a DECOY at logit 16 in the slot of a
sibling or of another earlier node that is NOT an ancestor: a mask that admits it moves the output by O(0.5).

With QK-norm the norm fixes the length of every new q and k row, so an aligned pair has the logit sqrt(128) g_q g_k whatever the
weight column's scale: the gammas are chosen for 12, and a decoy among the new tokens carries 12 as well (admitting it halves the
owner's mass: still O(0.25)).

Reference: numpy float64 on the values as the cache stores them; q_eff = round16(RoPE(q, history + depth)); query i sees key t iff
t < history or t = history + j with bit j of (anc_i & ((2 << i) - 1)) | (1 << i); out = sum e_t V_t / (sum e_t + 1e-6).
"""
import numpy as np

from attn_cases import BOUNDS, E4M3, E4M3_SCALES, EPS, F16, _rope, rnd_t, rope_table, to_e4m3
from prefill_attn_cases import rope_rows

HS, PAGE, NH, KVH, H, INTER = 128, 128, 8, 8, 1024, 512
LOGIT, DECOY_LOGIT = 12.0, 16.0
X_ONE_HOT = 64.0
BOUND = BOUNDS["rope"][F16]
HISTS = (0, 37, 128)
QK_EPS = 1e-6
QK_GAMMA = float(np.float16(np.sqrt(LOGIT / np.sqrt(HS))))   # aligned normalised rows: logit sqrt(HS) g^2 = 12
MASK64 = (1 << 64) - 1


def _comb(n):
    """a spine 0, 1, 3, 5, ... with one leaf on every spine node: node 32 hangs on node 31 (bits 31 and 32 of one mask)"""
    return [-1] + [(max(i - 2, 0) if i % 2 else i - 1) for i in range(1, n)]


# name -> (parent, node_count or None).  "dead": node 5 names a later node and node 7 hangs on it (both dead), node_count 10 < n = 12
TREES = {
    "n1": ([-1], None),
    "chain2": ([-1, 0], None),
    "star17": ([-1] + [0] * 16, None),
    "comb33": (_comb(33), None),
    "heap64": ([-1] + [(i - 1) // 2 for i in range(1, 64)], None),   # node 63 has depth 6 and bit 63
    "dead12": ([-1, 0, 0, 1, 1, 9, 2, 5, 3, 3, 4, 4], 10),
}


def prepare_ref(parent, count=None):
    """llmie_spec_tree_prepare's rule for one sequence: (depth list, anc list of python ints)"""
    n = len(parent)
    cnt = n if count is None else min(max(int(count), 1), n)
    depth, anc = [0] * n, [1] + [0] * (n - 1)
    for i in range(1, n):
        p = int(parent[i])
        live = i < cnt and 0 <= p < i and (anc[p] & 1)
        depth[i] = depth[p] + 1 if live else 0
        anc[i] = (anc[p] | (1 << i)) if live else (1 << i)
    return depth, anc


def chain_ref(n):
    return list(range(n)), [(2 << i) - 1 for i in range(n)]


def anc_i64(anc):
    """ancestor masks as the int64 tensor holds them (the bits of the uint64)"""
    return np.array([a & MASK64 for a in anc], dtype=np.uint64).view(np.int64)


DEFECTS = ("sibling", "rope_index", "shift32_wrap", "shift32_zero", "no_self")


def visibility(anc, n, defect=None):
    """vis[i, j]: node i sees chunk position j"""
    vis = np.zeros((n, n), bool)
    for i in range(n):
        a = (anc[i] & ((2 << i) - 1)) | (1 << i)
        if defect == "no_self":
            a &= ~(1 << i)
        for j in range(n):
            if defect == "sibling":
                vis[i, j] = j <= i
            elif defect == "shift32_wrap":   # a 32-bit shift whose count wraps: the mask's low word shifted by j mod 32
                vis[i, j] = ((a & 0xffffffff) >> (j % 32)) & 1
            elif defect == "shift32_zero":   # a 32-bit shift that gives 0 from 32 on: bits 32 .. 63 (the self bit included) are lost
                vis[i, j] = j < 32 and (a >> j) & 1
            else:
                vis[i, j] = (a >> j) & 1
    return vis


class Owner:
    def __init__(self, slot, cls):
        self.slot, self.cls, self.decoy = slot, cls, None


class TreeCase:
    def deq(self, stored, which):
        if self.scales is None:
            return np.asarray(stored, np.float32)
        return E4M3[stored] * np.float32(self.scales[which])

    def store(self, values, which):
        return rnd_t(values, F16) if self.scales is None else to_e4m3(np.asarray(values, np.float64) / np.float32(self.scales[which]))

    def config(self, llmie):
        ks, vs = self.scales or (0.0, 0.0)
        return dict(head_num=NH, kv_head_num=KVH, head_size=HS, inter_size=INTER, num_layers=self.L, vocab_size=100,
                    max_seq_len=self.max_seq, max_batch=self.bs, rotary_dim=HS, rotary_base=10000.0, rms_eps=1e-5, dtype=llmie.F16,
                    wfmt=llmie.W_F16, int4_group=128, kv_fmt=llmie.KV_NATIVE if self.scales is None else llmie.KV_FP8, k_scale=ks,
                    v_scale=vs)

    def describe(self, s, i, h):
        o = self.owners.get((s, i, h))
        return "case=%s sequence=%d (history %d) node=%d (depth %d, parent %d) head=%d class=%s slot=%s decoy=%s" % (
            self.cid, s, self.hist[s], i, self.depth[i], self.parent[i], h, o.cls if o else "none", o.slot if o else None,
            o.decoy if o else None)


def qk_norm_rows(x, gamma):
    """the per-head RMSNorm of rows x [..., HS] as the device stores it: one fp16 rounding"""
    x = np.asarray(x, np.float64)
    return rnd_t(x / np.sqrt((x * x).mean(axis=-1, keepdims=True) + QK_EPS) * gamma, F16).astype(np.float64)


def make_case(tree, kv="f16", qkn=False, L=2, hists=HISTS, seed=23):
    c = TreeCase()
    parent, count = TREES[tree]
    n, bs = len(parent), len(hists)
    c.cid = "%s-%s%s" % (tree, kv, "-qkn" if qkn else "")
    c.tree, c.kv, c.qkn, c.L, c.layer, c.bs, c.n, c.T = tree, kv, qkn, L, L - 1, bs, n, bs * n
    c.parent, c.count = list(parent), count
    c.depth, c.anc = prepare_ref(parent, count)
    c.hist, c.lens = [int(h) for h in hists], [n] * bs
    c.scales = None if kv == "f16" else E4M3_SCALES[kv]
    c.max_seq = -(-(max(c.hist) + n + 1) // PAGE) * PAGE
    c.gamma = np.full((L, HS), QK_GAMMA, np.float32) if qkn else None
    heads, sq = NH + 2 * KVH, float(np.sqrt(H))
    rng = np.random.default_rng([seed, n, len(tree)] + c.hist)
    c.tab = rope_table(c.max_seq, HS, HS)
    c.seq_of = np.repeat(np.arange(bs), n)
    node_of = np.tile(np.arange(n), bs)
    c.slot_of = np.asarray(c.hist)[c.seq_of] + node_of                       # where the row is stored
    c.rpos_of = np.asarray(c.hist)[c.seq_of] + np.asarray(c.depth)[node_of]  # the table row it is rotated by
    c.ipos_of = c.slot_of                                                    # (defect rope_index: rotated by its index)
    sd = np.concatenate([np.ones(NH), np.full(2 * KVH, 0.5)]).astype(np.float32)[None, None, :, None]
    c.w = rnd_t(rng.standard_normal((L, c.T, heads, HS), dtype=np.float32) * (sd / np.float32(sq)), F16)
    shape = (L, bs, KVH, c.max_seq, HS)
    if c.scales is None:
        c.k0, c.v0 = (rnd_t(rng.standard_normal(shape, dtype=np.float32) * 0.5, F16) for _ in range(2))
    else:
        c.k0, c.v0 = (rng.integers(0, 0x58, shape, dtype=np.uint8) | (rng.integers(0, 2, shape, dtype=np.uint8) << 7) for _ in range(2))

    def q_rows(pos):
        q = (c.w[c.layer, :, :NH] * np.float32(sq)).astype(np.float64)
        if qkn:
            q = qk_norm_rows(q, QK_GAMMA)
        return rnd_t(rope_rows(q, c.tab, pos), F16).astype(np.float64)

    c.q_eff = q_rows(c.rpos_of)
    vis = visibility(c.anc, n)

    # ---- owners: every (node, head), classes cycling; a slot of a head serves one owner or one decoy
    c.owners, taken, k = {}, set(), 0
    for s in range(bs):
        hist = c.hist[s]
        for i in range(n):
            live = bool(c.anc[i] & 1)
            items = ([("parent", hist + c.parent[i]), ("root", hist)] if live and i > 0 else []) + \
                    [("hist_last", hist - 1), ("hist_first", 0 if hist > 1 else -1), ("self", hist + i)]
            items = [(name, p) for name, p in items if p >= 0]
            for h in range(NH):
                for j in range(len(items)):
                    name, p = items[(k + j) % len(items)]
                    if (s, h, p) not in taken:
                        taken.add((s, h, p))
                        c.owners[(s, i, h)] = Owner(p, name)
                        break
                k += 1

    def plant(s, h, slot, q, logit):
        target = q * (logit * np.sqrt(HS) / np.dot(q, q))
        if slot < c.hist[s]:
            c.k0[c.layer, s, h, slot] = c.store(target, 0)
        else:   # a node: the pre-image goes into its weight column (QK-norm: the norm sets its length, the direction is what counts)
            j = slot - c.hist[s]
            t = s * n + j
            c.w[c.layer, t, NH + h] = rnd_t(_rope(target, c.tab[c.hist[s] + c.depth[j]], inverse=True) / sq, F16)

    for (s, i, h), o in c.owners.items():
        plant(s, h, o.slot, c.q_eff[s * n + i, h], LOGIT)
        # decoy: a sibling first, then an earlier node whose bit aliases an ancestor's under a 32-bit shift (j - 32 is an ancestor, j is
        # not), else any other earlier node that is no ancestor
        cands = [j for j in range(1, i) if not vis[i, j] and c.parent[j] == c.parent[i]] + \
                [j for j in range(32, i) if not vis[i, j] and vis[i, j - 32]] + [j for j in range(i) if not vis[i, j]]
        for j in cands:
            if (s, h, c.hist[s] + j) not in taken:
                taken.add((s, h, c.hist[s] + j))
                o.decoy = c.hist[s] + j
                plant(s, h, o.decoy, c.q_eff[s * n + i, h], DECOY_LOGIT)
                break
    c.rows = c.w * np.float32(sq)

    # ---- the appended rows as the pass stores them, per layer, rotated by `pos` (k_tol: 2 eps (|x| + |partner|) for the rotation's two
    # roundings; QK-norm: the normalised fp16 value may sit one ulp away -- another eps on either operand of the rotation: 4 eps)
    def new_rows(pos):
        kn_all, tol_all, vn_all = [], [], []
        for l in range(L):
            kn, vn = c.rows[l, :, NH:NH + KVH].astype(np.float64), c.rows[l, :, NH + KVH:]
            if qkn:
                kn = qk_norm_rows(kn, QK_GAMMA)
            kn_all.append(c.store(rnd_t(rope_rows(kn, c.tab, pos), F16), 0))
            vn_all.append(c.store(vn, 1))
            tol_all.append((4 if qkn else 2) * EPS[F16] * (np.abs(kn) + np.abs(np.concatenate([kn[..., HS // 2:], kn[..., :HS // 2]], axis=-1))))
        return kn_all, vn_all, tol_all

    c.k_new, c.v_new, c.k_tol = new_rows(c.rpos_of)
    c.k_cpu, c.v_cpu = after_pass(c, c.k0, c.k_new), after_pass(c, c.v0, c.v_new)
    # what the defect rope_index would compute: q and k rotated by history + index
    c.q_eff_index = q_rows(c.ipos_of)
    c.k_new_index = new_rows(c.ipos_of)[0]
    c.k_cpu_index = after_pass(c, c.k0, c.k_new_index)
    c.ref, c.mass = reference(c, c.deq(c.k_cpu, 0), c.deq(c.v_cpu, 1), with_mass=True)
    assert_mass(c, c.mass)
    return c


def assert_mass(c, mass, min_mass=0.9):
    for (s, i, h), m in mass.items():
        assert m >= min_mass, "planted row holds %.3f of the mass: %s" % (m, c.describe(s, i, h))


def after_pass(c, cache0, new):
    out = cache0.copy()
    for l in range(c.L):
        out[l, c.seq_of, :, c.slot_of] = new[l]
    return out


def reference(c, kfull, vfull, defect=None, with_mass=False):
    """float64 tree attention of the measured layer on the caches AFTER the pass (values [L, bs, kvh, max_seq, HS]) -> one
    [n, NH HS] array per sequence.  `defect` seeds one of DEFECTS (a deliberately wrong reference: the mutation check):
      sibling     the causal mask j <= i instead of the ancestors;   no_self   the self bit dropped
      shift32_wrap / shift32_zero  the mask read with a 32-bit shift (count mod 32 / zero from 32 on)
      rope_index  q and k rotated by history + index (kfull is replaced by the CPU rows rotated that way)"""
    n = c.n
    vis_c = visibility(c.anc, n, defect)
    q_all = c.q_eff_index if defect == "rope_index" else c.q_eff
    if defect == "rope_index":
        kfull = c.deq(c.k_cpu_index, 0)
    outs, mass = [], {}
    for s in range(c.bs):
        hist = c.hist[s]
        vis = np.concatenate([np.ones((n, hist), bool), vis_c], axis=1)
        out = np.zeros((n, NH * HS))
        for h in range(NH):
            K, V = kfull[c.layer, s, h, :hist + n].astype(np.float64), vfull[c.layer, s, h, :hist + n].astype(np.float64)
            S = q_all[s * n:(s + 1) * n, h] @ K.T / np.sqrt(HS)
            S[~vis] = -np.inf
            m = S.max(axis=1)
            m = np.where(np.isfinite(m), m, 0.0)
            e = np.exp(S - m[:, None])
            den = e.sum(axis=1)
            out[:, h * HS:(h + 1) * HS] = (e @ V) / (den + 1e-6)[:, None]
            for i in range(n):
                o = c.owners.get((s, i, h))
                if o is not None:
                    mass[(s, i, h)] = float(e[i, o.slot] / den[i]) if den[i] > 0 else 0.0
        outs.append(out)
    return (outs, mass) if with_mass else outs


def extra_atol(c, s):
    """one fp16 ulp of |x| where x != 0: the residual add rounds attention + x once more (element t of packed token t)"""
    a = np.zeros((c.n, NH * HS))
    t = np.arange(s * c.n, (s + 1) * c.n)
    a[t - s * c.n, t] = float(np.spacing(np.float16(X_ONE_HOT)))
    return a


def bound(c, s, exp):
    return BOUND[1] + BOUND[0] * np.abs(exp) + extra_atol(c, s)


def check_case(got, c, form, exp=None):
    """got, exp: one [n, NH HS] array per sequence -> the largest error / bound; raises with the words of the worst element"""
    exp = c.ref if exp is None else exp
    worst = 0.0
    for s in range(c.bs):
        r = np.abs(np.asarray(got[s], np.float64) - exp[s]) / bound(c, s, exp[s])
        if not (r <= 1.0).all():
            i, e = np.unravel_index(np.argmax(r), r.shape)
            raise AssertionError("%s: %s dim=%d is %r, expected %r (error / bound %.2f)" % (
                form, c.describe(s, int(i), int(e) // HS), int(e) % HS, float(got[s][i, e]), float(exp[s][i, e]), float(r[i, e])))
        worst = max(worst, float(r.max()))
    return worst


def k_row_tolerance(c, l):
    """what the GPU test allows an appended K row of layer l: k_tol on fp16 values; on e4m3 values the neighbouring code (one e4m3 step
    = 2^-3 relative, + two fp16 ulps at the row's magnitude: tests/test_prefill_attn_gpu.py)"""
    if c.scales is None:
        return c.k_tol[l]
    b = E4M3[c.k_new[l]].astype(np.float64) * c.scales[0]
    return 0.126 * np.abs(b) + c.scales[0] * 2.0 ** -9 + 2.0 ** -9 * np.abs(b).max(axis=-1, keepdims=True)


def defect_ratio(c, defect):
    """the largest (defective reference - reference) / bound over the elements owners hold.  rope_index also moves the appended K
    rows, which the GPU test checks first: there the ratio is taken over them as well (a rotation that is a few positions off
    leaves an owner at logit 12 most of its mass, so the attention output alone is a weak witness of it)."""
    bad = reference(c, c.deq(c.k_cpu, 0), c.deq(c.v_cpu, 1), defect=defect)
    worst = 0.0
    if defect == "rope_index":
        for l in range(c.L):
            err = np.abs(c.deq(c.k_new_index[l], 0).astype(np.float64) - c.deq(c.k_new[l], 0))
            worst = max(worst, float((err / np.maximum(k_row_tolerance(c, l), float(np.spacing(np.float16(1e-3))))).max()))
    for (s, i, h), o in c.owners.items():
        sl = slice(h * HS, (h + 1) * HS)
        worst = max(worst, float((np.abs(bad[s][i, sl] - c.ref[s][i, sl]) / bound(c, s, c.ref[s])[i, sl]).max()))
    return worst


def expressible(tree, defect):
    """can the defect move an owner's element of this tree at all?"""
    parent, count = TREES[tree]
    n = len(parent)
    depth, anc = prepare_ref(parent, count)
    if defect == "sibling":      # some node has an earlier non-ancestor
        return not np.array_equal(visibility(anc, n), visibility(anc, n, "sibling"))
    if defect == "rope_index":   # some node's depth differs from its index
        return any(depth[i] != i for i in range(n))
    if defect in ("shift32_wrap", "shift32_zero"):   # some node's view of itself or of an earlier node changes
        return bool((np.tril(visibility(anc, n)) != np.tril(visibility(anc, n, defect))).any())
    return True


CASES = [(t, kv, qkn) for t in TREES for kv, qkn in (("f16", False), ("np2", False), ("f16", True), ("pow2", True))]
CASE_IDS = ["%s-%s%s" % (t, kv, "-qkn" if qkn else "") for t, kv, qkn in CASES]
