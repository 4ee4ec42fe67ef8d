"""Tests of the decode-attention tests (no GPU): tests/attn_cases.py builds the inputs and the float64 reference that
tests/test_decode_attn_gpu.py holds the HIP kernels to.  Here, on the CPU:

1. the project's C oracle (fp32, oracle/llmie_oracle.c) meets the GPU tests' bounds on every case of their table, so the bounds
   are met by a correct implementation before any kernel is involved;
2. defects seeded into the float64 reference (a row left out, V from the neighbouring slot, a chunk tail cut by one, the stale
   slot instead of the appended token, splits >= 16 ignored, a page of a multi-page chunk read from the chunk's first page) are
   rejected by the very comparison the GPU tests use, in every case in which they can be expressed;
3. the same defects on the inputs the older attention tests draw (plain random caches, step 2048, fp16 bound) pass unnoticed:
   the reason for this file, kept executable.
"""
import numpy as np
import pytest

import attn_cases as ac
import oracle as orc

UNIFORM, RAGGED, GENERIC = ac.uniform_cases(), ac.ragged_cases(), ac.generic_cases()
E4M3 = ac.e4m3_cases()


def _oracle(c, b=None):
    """the oracle's decode attention on the case (sequence b alone, or the whole uniform batch) -> out"""
    sl = slice(None) if b is None else slice(b, b + 1)
    step = c.steps[0 if b is None else b]
    qkv = c.qkv[sl].copy()
    if c.rope:
        qkv = ac.rnd_t(orc.rope_decode(qkv, c.nh, c.kvh, c.hs, step, c.rot, 10000.0), c.dtype)  # stored in T by the unfused path
    kc, vc = np.ascontiguousarray(c.kc[:, sl]), np.ascontiguousarray(c.vc[:, sl])
    return orc.decoder_mha(qkv, c.bias, kc, vc, c.layer, c.nh, c.kvh, c.hs, step)


@pytest.mark.parametrize("cid,dtype,geo,step,logit", UNIFORM, ids=[u[0] for u in UNIFORM])
def test_oracle_meets_the_gpu_bounds_uniform(cid, dtype, geo, step, logit):
    for rope in (False, True):
        c = ac.build_uniform(dtype, geo, step, logit, rope=rope)
        form = "oracle-rope" if rope else "oracle-plain"
        r = ac.check(_oracle(c), c, form, ac.BOUNDS["rope" if rope else "plain"][dtype])
        print("%s %s: error / bound %.3g" % (cid, form, r))


@pytest.mark.parametrize("cid,dtype,geo,steps", RAGGED, ids=[r[0] for r in RAGGED])
def test_oracle_meets_the_gpu_bounds_ragged(cid, dtype, geo, steps):
    c = ac.build_ragged(dtype, geo, steps)
    out = np.concatenate([_oracle(c, b) for b in range(c.bs)])
    print("%s: error / bound %.3g" % (cid, ac.check(out, c, "oracle-ragged", ac.BOUNDS["rope"][dtype])))


@pytest.mark.parametrize("cid,dtype,g,step", GENERIC, ids=[g[0] for g in GENERIC])
def test_oracle_meets_the_gpu_bounds_generic(cid, dtype, g, step):
    c = ac.build_generic(dtype, g, step)
    print("%s: error / bound %.3g" % (cid, ac.check(_oracle(c), c, "oracle-plain", ac.BOUNDS["plain"][dtype])))


def _seeded(c):
    """[(defect, class)] expressible in this case"""
    classes = sorted({c.cls[b][h] for b in range(c.bs) for h in range(c.nh) if c.pos[b][h] is not None})
    todo = [("drop", k) for k in classes] + [(d, None) for d in ac.DEFECTS if d != "drop"]
    return [(d, k) for d, k in todo if ac.expressible(c, d, k)]


def _all_rejected(c, bounds):
    ac.check(c.ref, c, "reference", bounds)
    todo = _seeded(c)
    assert ("drop", c.cls[0][0]) in todo and len(todo) >= 2
    for defect, cls in todo:
        bad = ac.reference(c, defect, cls)
        with pytest.raises(AssertionError, match="class="):
            ac.check(bad, c, "seeded:%s:%s" % (defect, cls), bounds)
    return todo


@pytest.mark.parametrize("cid,dtype,geo,step,logit", UNIFORM, ids=[u[0] for u in UNIFORM])
def test_seeded_defects_are_rejected_uniform(cid, dtype, geo, step, logit):
    c = ac.build_uniform(dtype, geo, step, logit)
    todo = [d for d, _ in _all_rejected(c, ac.BOUNDS["plain"][dtype])]
    # the defects the geometry allows are all there (every class has an owner in a uniform case)
    C = c.chunk
    assert ("trunc_last" in todo) and ("stale_new" in todo)
    assert ("v_next" in todo) == (step >= 2)
    assert ("ignore_split16" in todo) == (step > 16 * C)
    assert ("page0" in todo) == (C > ac.KV_PAGE and step > ac.KV_PAGE)


@pytest.mark.parametrize("cid,dtype,geo,steps", RAGGED, ids=[r[0] for r in RAGGED])
def test_seeded_defects_are_rejected_ragged(cid, dtype, geo, steps):
    _all_rejected(ac.build_ragged(dtype, geo, steps), ac.BOUNDS["rope"][dtype])


@pytest.mark.parametrize("cid,dtype,g,step", GENERIC, ids=[g[0] for g in GENERIC])
def test_seeded_defects_are_rejected_generic(cid, dtype, g, step):
    _all_rejected(ac.build_generic(dtype, g, step), ac.BOUNDS["plain"][dtype])


def test_ragged_cases_own_every_class_of_their_geometry():
    """a sequence of a ragged batch has 8 owners for up to 30 classes: the appended token and one page boundary are owned in every
    sequence (asserted by the generator), every class by some sequence of the geometry"""
    owned, exist = {}, {}
    for cid, dtype, geo, steps in RAGGED:
        c = ac.build_ragged(dtype, geo, steps)
        key = ac.geo_id(dtype, geo)
        for b in range(c.bs):
            owned.setdefault(key, set()).update(n for k in c.cls[b] for n in k.split("+"))
            exist.setdefault(key, set()).update(n for k, _ in c.classes[b] for n in k.split("+"))
    for key in exist:
        assert owned[key] >= exist[key], (key, exist[key] - owned[key])


@pytest.mark.parametrize("cid,hs,ratio,bs,sc,step", E4M3, ids=[e[0] for e in E4M3])
def test_e4m3_cpu_composition_meets_the_engine_bound_and_defects_are_rejected(cid, hs, ratio, bs, sc, step):
    """the bound of the e4m3 engine cases (fp16 attention bound + one fp16 ulp of |x|) against the CPU composition of the same
    step: measured worst error / bound 0.23, so the bound is not widened"""
    c = ac.finish_e4m3(ac.make_case_e4m3(hs, ratio, bs, sc, step))
    bounds, extra = ac.BOUNDS["rope"][ac.F16], ac.e4m3_extra_atol(c)
    if bs < 64 or sc == "np2":   # (batch 64: 64 oracle calls per case)
        r = ac.check(ac.e4m3_cpu_composition(c), c, "cpu composition", bounds, extra_atol=extra)
        print("%s: error / bound %.3f" % (cid, r))
        assert r < 0.5
    todo = _seeded(c) if bs < 64 else [(d, None) for d in ("trunc_last", "v_next") if ac.expressible(c, d)]
    assert todo
    for defect, cls in todo:
        with pytest.raises(AssertionError, match="class="):
            ac.check(ac.reference(c, defect, cls), c, "seeded:%s:%s" % (defect, cls), bounds, extra_atol=extra)


def test_every_geometry_is_in_the_table():
    ids = [u[0] for u in UNIFORM]
    for dtype in (ac.F16, ac.F32):
        for hs in (32, 64, 128, 256):
            C = ac.chunk_len(dtype, hs)
            assert any(i.startswith("%s-hs%d-" % (dtype, hs)) and i.endswith("-step%d" % (17 * C + 1)) for i in ids)
            seqs = {ac.max_seq_of(dtype, g[0], g[6]) % 128 == 0 for g in ac.geometries(dtype) if g[0] == hs}
            assert seqs == {True, False}   # a slab end on and off a page boundary
    assert {g[1] for g in ac.GEOMETRIES if g[0] == 128} == {1, 2, 4, 8}
    assert [ac.chunk_len(ac.F16, h) for h in (32, 64, 128, 256)] == [512, 256, 128, 64]
    assert [ac.chunk_len(ac.F32, h) for h in (32, 64, 128, 256)] == [256, 128, 64, 32]
    assert [ac.chunk_len(ac.F16, h, e4m3=True) for h in (64, 128)] == [512, 256]
    assert {(e[1], e[2], ac.e4m3_cpw(e[3])) for e in E4M3} == {(h, r, k) for h in (64, 128) for r in (1, 4) for k in (1, 2, 8)}


def _head_ratios(c, bad, bounds):
    """largest error / bound per (sequence, head)"""
    rtol, atol = bounds
    r = np.abs(bad - c.ref) / (atol + rtol * np.abs(c.ref))
    return r.reshape(c.bs, c.nh, c.hs).max(axis=-1)


def test_plain_random_caches_cannot_see_these_defects():
    """The inputs of test_decoder_mha at its longest context (q ~ N(0,1), caches 0.5 N(0,1), step 2048, hs 128, 32 heads, fp16
    bound): with a cached key/value row left out, or V taken from the neighbouring slot, the worst of the 4096 output elements
    sits at 0.4 - 1.0 of its bound (measured here: at most 1.02, one element), so such a defect passes or fails by the draw.
    With the planted rows of this file the same defects put EVERY affected head at more than 100 times the bound."""
    kw = dict(dtype=ac.F16, hs=128, nh=32, kvh=32, bs=1, steps=2048, max_seq=2048, chunk=128, seed=13)
    bounds = ac.BOUNDS["plain"][ac.F16]
    plain = ac.make_case(planted=False, **kw)
    planted = ac.make_case(planted=True, **kw)
    # (cache rows only: the appended token's k and v come from the qkv row, N(0,1), and carry twice a cache row's weight)
    keep = np.array([["new" not in k for k in plain.cls[0]]])
    classes = sorted({k for k in plain.cls[0] if "new" not in k})
    for defect, cls in [("drop", k) for k in classes] + [("v_next", None), ("v_prev", None)]:
        hit = keep & (np.array([plain.cls[0]]) == cls if cls else True)
        weak = _head_ratios(plain, ac.reference(plain, defect, cls), bounds)[hit]
        strong = _head_ratios(planted, ac.reference(planted, defect, cls), bounds)[hit]
        print("%s %s: error / bound, plain random caches max %.2f (heads over 1: %d of %d), planted rows min %.0f" % (
            defect, cls, weak.max(), (weak > 1).sum(), weak.size, strong.min()))
        assert weak.max() < 1.5 and (weak > 1).sum() <= 1
        assert strong.min() > 100
        with pytest.raises(AssertionError):
            ac.check(ac.reference(planted, defect, cls), planted, "seeded:%s" % defect, bounds)
