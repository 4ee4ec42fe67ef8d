"""Tests of the prefill-attention tests (no GPU): tests/prefill_attn_cases.py builds the inputs and the float64 reference that
tests/test_prefill_attn_gpu.py holds prefill_flash_kernel to.  Here, on the CPU:

1. the table reaches, by the plan text of llmie_decoder_prefill_layer_plan, all six flash instantiations on dense and on paged caches,
   the three producers of the new K / V rows, GQA ratios 1 and 4 and both e4m3 scale pairs, and every row, sequence and position class
   has an owner in some case;
2. the oracle's composition of the same attention (fp16 roundings where the device rounds) meets the GPU test's bound against the
   float64 reference on every case, so the bound is met by a correct implementation before any kernel is involved;
3. defects seeded into the float64 reference (the mask off by one either way, the history left out of the mask, an owner's class
   dropped, V from the neighbouring slot, clamped keys counted, a page from the previous table entry, the stale cache row, layer 0
   instead of layer 1) are rejected by the very comparison the GPU test uses, in every case in which they can be expressed;
4. the same defects on today's inputs (what a random model projects from N(0, 1) hidden states, random caches, a few hundred tokens)
   seen through the whole layer and the bounds of test_prefill_matches_oracle: the reason for this file, kept executable.
"""
import functools
import re

import numpy as np
import pytest

import prefill_attn_cases as pc
from conftest import systematic_error

FRO_F16, PROJ_F16 = 3e-3, 2e-4   # tests/test_prefill_gpu.py
PAGED, RAGGED = 1, 2   # call flags of llmie_decoder_prefill_layer_plan (include/llmie.h)


@pytest.fixture(scope="module")
def built(llmie):
    llmie.build()
    return llmie


@functools.lru_cache(maxsize=None)
def case(cid):
    return pc.build(pc.TABLE[pc.IDS.index(cid)])


def test_the_table_reaches_every_form_producer_and_class(built):
    reached, producers, ratios, scales = set(), set(), set(), set()
    rows, seqs, poss, decoys, rows_of_form = set(), set(), set(), set(), {}
    for cid in pc.IDS:
        c = case(cid)
        for paged in (0, PAGED):
            text, status = built.decoder_prefill_layer_plan(c.config(built), c.T, c.bs, c.max_q_len, call_flags=paged | (RAGGED if c.bs > 1 else 0))
            assert text is not None, (c.cid, status)
            for word in c.plan_words():
                assert word in text.split(" "), (c.cid, word, text)
            reached.add((c.form, "f16" if c.scales is None else "e4m3", "paged" if paged else "dense"))
        producers.add(c.producer)
        ratios.add(c.rep)
        scales.add(c.scales)
        for (s, i, h), o in c.owners.items():
            rows.update(o.rowcls.split("+"))
            rows_of_form.setdefault(c.form, set()).update(o.rowcls.split("+"))
            poss.update(o.cls.split("+"))
            if o.decoy is not None:
                decoys.add("cache" if o.decoy >= c.ctx[s] else "next_token")
        for s in range(c.bs):   # every sequence has owners in its first and in its last row
            seqs.update(c.seq_classes[s])
            assert {0, c.lens[s] - 1} <= {i for (s_, i, h) in c.owners if s_ == s}, c.cid
    assert reached == {(f, kv, lay) for f in pc.FORM_BQ for kv in ("f16", "e4m3") for lay in ("dense", "paged")}
    assert producers == set(pc.PRODUCER_PLAN) and ratios >= {1, 4}
    assert scales == {None, (1.0 / 32, 1.0 / 16), (0.037, 0.021)}
    assert rows >= set(pc.ROW_CLASSES), set(pc.ROW_CLASSES) - rows
    for form in pc.FORM_BQ:   # the rows around the workgroup height, and a partial tail tile, at the height of every form
        assert rows_of_form[form] >= {"row0", "bq_last", "bq_first", "last", "tail"}, (form, rows_of_form[form])
    assert seqs >= set(pc.SEQ_CLASSES), set(pc.SEQ_CLASSES) - seqs
    assert poss >= set(pc.POS_CLASSES), set(pc.POS_CLASSES) - poss
    assert decoys == {"cache", "next_token"}


@pytest.mark.parametrize("cid", pc.IDS)
def test_oracle_composition_meets_the_gpu_bound_and_seeded_defects_are_rejected(cid):
    """measured worst error / bound of the composition over the table: 0.119 (f16-32x32-fused; the e4m3 cases 0.114), least mass of a
    planted row 0.9941"""
    c = case(cid)
    print("%s: least mass of a planted row %.4f, %d owners" % (c.cid, min(c.mass.values()), len(c.owners)))
    # 2. the composition, at every owner row and a few others
    rows = pc.oracle_rows(c)
    ref = [r[rows[s]] for s, r in enumerate(c.ref)]
    r = pc.check_case(pc.oracle_composition(c, rows), c, "oracle composition", exp=ref, rows=rows, residual=False)
    print("%s: oracle composition error / bound %.3f" % (c.cid, r))
    assert r < 0.25 and min(c.mass.values()) > 0.99
    # 3. seeded defects, through the comparison of the GPU test (the residual's ulp included), at the same rows
    kf, vf = c.deq(c.k_cpu, 0), c.deq(c.v_cpu, 1)
    assert pc.check_case(ref, c, "reference", exp=ref, rows=rows) == 0.0
    classes = sorted({o.cls for o in c.owners.values()})
    todo = [("drop", k) for k in classes] + [(d, None) for d in pc.DEFECTS if d != "drop" and pc.expressible(c, d)]
    names = {d for d, _ in todo}
    assert names >= {"mask_plus1", "mask_minus1", "drop", "v_next", "v_prev", "clamp", "stale"}, names
    assert ("no_history" in names) == any(h > 0 for h in c.hist) and ("layer0" in names) == (c.L == 2)
    assert ("page_prev" in names) == (max(c.ctx) > pc.PAGE)
    for defect, cls in todo:
        bad = pc.reference(c, kf, vf, defect, cls, rows=rows)
        with pytest.raises(AssertionError, match=r"class=%s " % re.escape(cls) if cls else r"class=(?!none)"):
            pc.check_case(bad, c, "seeded:%s:%s" % (defect, cls), exp=ref, rows=rows)


def _layer(x, w, att):
    """float64 hidden state behind one decoder layer whose attention output is `att`"""
    h = x + att @ w["o"].T
    hn = h / np.sqrt((h * h).mean(axis=1, keepdims=True) + 1e-5) * w["ffn_norm"]
    gu = hn @ w["gate_up"].T
    gate, up = gu[:, :gu.shape[1] // 2], gu[:, gu.shape[1] // 2:]
    return h + (gate / (1 + np.exp(-gate)) * up) @ w["down"].T


def _through_todays_bounds(plain, x, w):
    """{defect: (element-wise, Frobenius, projection) error / bound} of the layer's output behind the seeded attention"""
    kf, vf = plain.deq(plain.k_cpu, 0), plain.deq(plain.v_cpu, 1)
    exp = _layer(x, w, np.concatenate(plain.ref))
    out = {}
    for defect in pc.DEFECTS:
        cls = sorted({o.cls for o in plain.owners.values()})[0] if defect == "drop" else None
        got = _layer(x, w, np.concatenate(pc.reference(plain, kf, vf, defect, cls)))
        fro, proj = systematic_error(got, exp)
        out[defect] = (float((np.abs(got - exp) / (3e-2 + 3e-2 * np.abs(exp))).max()), fro / FRO_F16, proj / PROJ_F16)
        print("%s: %s, error / bound element-wise %.3f, Frobenius %.3f, projection %.3f" % ((defect, plain.cid) + out[defect]))
    return out


def test_todays_inputs_cannot_see_these_defects():
    """Plain random rows (q ~ N(0, 1), k, v ~ 0.5 N(0, 1): the generator's background with nothing planted), 300 and 77 tokens behind
    640 and 900 of history, seen as the existing prefill tests see attention: through a random output projection and FFN (the uniform
    weights of test_prefill_gpu._model, x ~ N(0, 1)) and the bounds of test_prefill_matches_oracle on the layer's output (3e-2 + 3e-2
    |exp| element-wise, 3e-3 relative Frobenius error, 2e-4 projection on the signal).  Measured, error / bound (element-wise,
    Frobenius, projection): mask t <= qpos + 1 0.29 / 0.34 / 0.003, mask t < qpos 0.23 / 0.33 / 0.001, an owner's key dropped 0.12 /
    0.02 / 0.001, V from the next / previous slot 0.26 / 0.12 / 0.007: each moves one key in n and passes unnoticed.  The other five
    are seeded wholesale -- the history out of the mask, up to 63 clamped copies of a row, every page but the first, every new row
    stale, a whole layer's caches: they replace a constant share of the keys and any inputs see them (printed, not asserted); a
    kernel commits them one tile, one page or one row at a time, which is again one key in n.  On the planted rows every one of the
    ten is at more than 100 times the attention bound.  (With 64 and 100 tokens of history instead, the first rows of a sequence
    attend to fewer than 100 keys and the mask defects reach 2 - 3 times the bounds: today's tests do see those rows.)"""
    rng = np.random.default_rng(41)
    nh, kvh, I, lens, hist = 8, 8, 1376, [300, 77], [640, 900]
    H, T = nh * pc.HS, sum(lens)
    u = lambda shape, s: pc.rnd_t(rng.uniform(-1, 1, shape) * s, pc.F16).astype(np.float64)
    w = dict(o=u((H, H), 2 / np.sqrt(H)), ffn_norm=u((H,), 0.2) + 1, gate_up=u((2 * I, H), 2 / np.sqrt(H)), down=u((H, I), 2 / np.sqrt(I)))
    x = pc.rnd_t(rng.standard_normal((T, H)), pc.F16).astype(np.float64)
    plain = pc.make_case("plain-random-rows", nh, kvh, 2, lens, hist, "f16", "q64w4t1", "separate", planted=False)
    seen = _through_todays_bounds(plain, x, w)
    for defect in ("mask_plus1", "mask_minus1", "drop", "v_next", "v_prev"):
        assert max(seen[defect]) < 0.5, (defect, seen[defect])
    planted = case(pc.IDS[1])
    pk, pv = planted.deq(planted.k_cpu, 0), planted.deq(planted.v_cpu, 1)
    for defect in pc.DEFECTS:
        cls = sorted({o.cls for o in planted.owners.values()})[0] if defect == "drop" else None
        if pc.expressible(planted, defect, cls):
            bad = pc.reference(planted, pk, pv, defect, cls)
            worst = max(float((np.abs(b - r) / (pc.BOUND[1] + pc.BOUND[0] * np.abs(r) + planted.extra_atol(s))).max())
                        for s, (b, r) in enumerate(zip(bad, planted.ref)))
            print("%s: planted rows, error / bound %.0f" % (defect, worst))
            assert worst > 100
