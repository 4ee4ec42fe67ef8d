"""QK-norm on an engine (llmie_decoder_set_qk_norm), in the pattern of tests/test_sink_engine_gpu.py: held to the float64 layer
restatement of tests/qknorm_cases.py (head_norm on q and k in front of the rotation) at model_param_cases.bounds() unchanged -- the
project's engine bounds; QK-norm adds one fp16 rounding of q and k, the kind they already cover.  eps = 1e-6 throughout.

Engine A (head size 128, 4 heads over 2, inter 512, 2 layers): prefill [150, 70, 129] dense and paged, then three decode steps at
batch 1, ragged and paged-ragged; a short prefill [70, 30] (`short_splitk`, qkv=splitk asserted from the plan queries); decode at
batches taken from llmie_decoder_plan_name so that the gemv, packed and splitk sequences each run.  Engine B (head size 64, 4 over 2,
4 layers): decode on a ragged batch, native and e4m3 cache.  An int8 and an MXFP4 engine of geometry A: one prefill and one decode
step.  In every check the restatements that normalise behind RoPE, swap the gammas, leave k un-normalised, or do not normalise at
all miss 10 x bounds["fro"] (asserted), so an engine that did any of these would fail.  set_qk_norm(None, None) restores the bits
recorded before it was set.  The Qwen3-MoE layer: the smallest ragged decode case of moe_engine_ref with LLMIE_MOE_SOFTMAX_ALL and
QK-norm against the oracle composition with head_norm in its attention, at 2e-2 per stable row.  Refusals.
"""
import numpy as np
import pytest
import torch

import model_param_cases as mpc
import qknorm_cases as qc
from conftest import systematic_error

pytestmark = pytest.mark.gpu
DEV, F16 = "cuda", torch.float16
INTER, MAX_SEQ = 512, 1024
GEOMETRY = {128: (4, 2, 2), 64: (4, 2, 4)}   # head size -> (heads, KV heads, layers)
OTHERS = ("after_rope", "gammas_swapped", "k_raw")

KINDS = {
    # kind: head size, weight format, sequence lengths, prefill first, decode steps, entry, e4m3 cache
    "A_dense_ragged": (128, "f16", [150, 70, 129], True, 3, "ragged", False),
    "A_paged_ragged": (128, "f16", [150, 70, 129], True, 3, "paged", False),
    "A_batch1": (128, "f16", [150], True, 3, "batch1", False),
    "A_short_prefill": (128, "f16", [70, 30], True, 0, "ragged", False),
    "B_ragged": (64, "f16", [150, 70, 129], False, 2, "ragged", False),
    "B_e4m3": (64, "f16", [150, 70], False, 2, "ragged", True),
    "A_int8": (128, "int8", [150, 70, 129], True, 1, "ragged", False),
    "A_mxfp4": (128, "mxfp4", [150, 70, 129], True, 1, "ragged", False),
}


def _cfg(llmie, hs, max_batch, wfmt="f16", e4m3=False):
    nh, kvh, L = GEOMETRY[hs]
    code = llmie.W_MXFP4 if wfmt == "mxfp4" else mpc.wfmt_code(llmie, wfmt)
    cfg = dict(head_num=nh, kv_head_num=kvh, head_size=hs, inter_size=INTER, num_layers=L, vocab_size=100, max_seq_len=MAX_SEQ,
               max_batch=max_batch, rotary_dim=hs, rotary_base=10000.0, rms_eps=1e-5, dtype=llmie.F16, wfmt=code,
               int4_group=0 if wfmt == "mxfp4" else 128)
    if e4m3:
        cfg.update(kv_fmt=llmie.KV_FP8, k_scale=mpc.KS, v_scale=mpc.VS)
    return cfg


def _engine_layers(llmie, layers, wfmt):
    if wfmt != "mxfp4":
        return mpc.engine_layers(llmie, layers, wfmt)
    import mxfp4_cases as MX
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    eng, ref = [], []
    for w in layers:
        e, o = dict(attn_norm=d(w["attn_norm"]).to(F16), ffn_norm=d(w["ffn_norm"]).to(F16)), dict(w)
        for m in mpc.MATS:
            wq, sc = MX.quantize(w[m].astype(np.float16))
            e[m], o[m] = dict(data=d(wq), scale=d(sc)), MX.dequantize(wq, sc).astype(np.float32)
        eng.append(e)
        ref.append(o)
    return eng, ref


def _check(got, exp, others, bounds, what):
    rtol, atol = bounds["elem"]
    got = got.double().cpu().numpy()
    err = np.abs(got - exp)
    assert (err <= atol + rtol * np.abs(exp)).all(), "%s: worst error / bound %.3g" % (what, (err / (atol + rtol * np.abs(exp))).max())
    fro, proj = systematic_error(got, exp)
    print("%s: fro %.2e proj %.2e; others %s" % (what, fro, proj, {k: round(float(systematic_error(v, exp)[0]), 3) for k, v in others.items()}))
    assert fro <= bounds["fro"] and proj <= bounds["proj"], (what, fro, proj)
    for name, other in others.items():
        assert systematic_error(other, exp)[0] > 10 * bounds["fro"], "%s: %s does not matter to this case" % (what, name)


class _Refs:
    """the engine's restatement and the ones an engine with a defect would follow, each on its own caches"""

    def __init__(self, cfg, ref_layers, k0, v0, tab, qg, kg, store):
        self.cfg, self.layers, self.tab, self.qg, self.kg, self.store = cfg, ref_layers, tab, qg, kg, store
        self.caches = {n: (k0.astype(np.float64).copy(), v0.astype(np.float64).copy()) for n in ("exp", "no norm") + OTHERS}

    def step(self, x, lens, hist, stored):
        out = {}
        for name, (kc, vc) in self.caches.items():
            gam = (None, None) if name == "no norm" else (self.qg, self.kg)
            out[name] = qc.layer_restatement(self.cfg, self.layers, x, kc, vc, lens, hist, self.tab, gam[0], gam[1], qc.EPS,
                                             name if name in OTHERS else "none", self.store, stored if name == "exp" else None)
        return out.pop("exp"), out


@pytest.mark.parametrize("kind", list(KINDS))
def test_engine_with_qk_norm(llmie, kind):
    hs, wfmt, lens, prefill, steps, entry, e4m3 = KINDS[kind]
    nh, kvh, L = GEOMETRY[hs]
    H, bs, paged = nh * hs, len(lens), entry == "paged"
    rng = np.random.default_rng(7)
    layers = mpc.draw_layers(rng, nh, kvh, hs, INTER, L)
    eng, ref_layers = _engine_layers(llmie, layers, wfmt)
    cfg = _cfg(llmie, hs, bs, wfmt, e4m3)
    dec = llmie.Decoder(cfg, eng)
    bounds = mpc.bounds(wfmt, "paged_e4m3" if e4m3 else "dense")
    ks, vs = (cfg["k_scale"], cfg["v_scale"]) if e4m3 else (1.0, 1.0)
    store = (lambda rows, which: mpc.e4m3_cache_rounding(rows, (ks, vs)[which])) if e4m3 else (lambda rows, which: mpc.h16(rows))
    qg, kg = qc.gammas(L, hs, 13, *qc.GAMMA_RANGE["prefill" if prefill else "decode_only"])
    qgd, kgd = torch.from_numpy(qg).to(DEV), torch.from_numpy(kg).to(DEV)
    tab = llmie.rope_table(MAX_SEQ, hs, hs, cfg["rotary_base"])
    shape = (L, bs, kvh, MAX_SEQ, hs)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    mp = MAX_SEQ // 128
    table = i32(np.random.default_rng(5).permutation(bs * mp + 2)[:bs * mp].reshape(bs, mp)) if paged else None
    cshape = (L, bs * mp + 2, kvh, 128, hs) if paged else shape
    k0, v0, kq, vq = mpc.draw_caches(rng, shape, "f16", "paged_e4m3" if e4m3 else "dense")
    if prefill:
        k0, v0 = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    new_cache = lambda a, q: torch.zeros(cshape, dtype=F16, device=DEV) if prefill else torch.from_numpy(q if e4m3 else a).to(DEV).to(torch.uint8 if e4m3 else F16)
    refs = _Refs(cfg, ref_layers, k0, v0, tab, qg, kg, store)
    T = sum(lens)
    x = mpc.h16(rng.standard_normal((T, H)).astype(np.float32))
    xd = torch.from_numpy(x).to(DEV).to(F16)

    def run_prefill(kd, vd):
        out = torch.full_like(xd, 9.0)
        if paged:
            dec.prefill_paged(xd, out, kd, vd, table, i32(lens), i32([0] * bs), max(lens))
        else:
            dec.prefill(xd, out, kd, vd, i32(lens), i32([0] * bs), max(lens))
        return out

    def run_decode(xsd, kd, vd, new_ctx):
        od = torch.full((bs, H), 9.0, dtype=F16, device=DEV)
        if paged:
            dec.forward_paged_ragged(xsd, od, kd, vd, table, i32(new_ctx))
        elif entry == "batch1":
            dec.forward(xsd, od, kd, vd, new_ctx[0])
        else:
            dec.forward_ragged(xsd, od, kd, vd, i32(new_ctx))
        return od

    if kind == "A_short_prefill":   # the short split-K sequence, its QKV slabs finalised without the RoPE epilogue
        assert llmie.decoder_plan_name(cfg, True, T, call_flags=llmie.PLAN_QK_NORM) == "short_splitk"
        text, _ = llmie.decoder_prefill_layer_plan(cfg, T, bs, max(lens), call_flags=llmie.PLAN_QK_NORM)
        assert " qkv=splitk " in text and " rope_append=1 " in text and text.endswith(" qk_norm=1"), text
    xs0 = torch.from_numpy(mpc.h16(rng.standard_normal((bs, H)).astype(np.float32))).to(DEV).to(F16)
    first = lambda: run_prefill(new_cache(k0, kq), new_cache(v0, vq)) if prefill else run_decode(xs0, new_cache(k0, kq), new_cache(v0, vq), [c + 1 for c in lens])
    try:
        plain = first()   # before anything is set
        dec.set_qk_norm(qgd, kgd, qc.EPS)
        kd, vd = new_cache(k0, kq), new_cache(v0, vq)
        dev = lambda: (mpc.TAB[kd.cpu().numpy()] * np.float32(ks), mpc.TAB[vd.cpu().numpy()] * np.float32(vs)) if e4m3 else None
        ctx = list(lens)
        if prefill:
            out = run_prefill(kd, vd)
            torch.cuda.synchronize()
            exp, others = refs.step(x, lens, [0] * bs, dev())
            _check(out, exp, others, bounds, "%s prefill" % kind)
        for step in range(steps):
            xs = mpc.h16(rng.standard_normal((bs, H)).astype(np.float32))
            new_ctx = [c + 1 for c in ctx]
            od = run_decode(torch.from_numpy(xs).to(DEV).to(F16), kd, vd, new_ctx)
            torch.cuda.synchronize()
            exp, others = refs.step(xs, [1] * bs, ctx, dev())
            _check(od, exp, others, bounds, "%s decode step %d" % (kind, step))
            ctx = new_ctx
        assert not torch.equal(first(), plain), "QK-norm changes nothing"
        dec.set_qk_norm(None, None)
        assert torch.equal(first(), plain), "set_qk_norm(None, None) did not restore the pass"
        torch.cuda.synchronize()
    finally:
        dec.close()


def test_decode_sequences_gemv_packed_splitk(llmie):
    """engine A, one ragged decode step at the first batch that llmie_decoder_plan_name sends down each of the three fused sequences"""
    hs, max_batch = 128, 40
    nh, kvh, L = GEOMETRY[hs]
    H = nh * hs
    rng = np.random.default_rng(17)
    layers = mpc.draw_layers(rng, nh, kvh, hs, INTER, L)
    eng, ref_layers = mpc.engine_layers(llmie, layers, "f16")
    cfg = _cfg(llmie, hs, max_batch)
    flags = llmie.PLAN_RAGGED | llmie.PLAN_QK_NORM
    batch_of = {}
    for rows in range(1, max_batch + 1):
        batch_of.setdefault(llmie.decoder_plan_name(cfg, False, rows, call_flags=flags), rows)
    assert {"gemv", "packed", "splitk"} <= set(batch_of), batch_of
    qg, kg = qc.gammas(L, hs, 13, *qc.GAMMA_RANGE["decode_only"])
    qgd, kgd = torch.from_numpy(qg).to(DEV), torch.from_numpy(kg).to(DEV)
    tab = llmie.rope_table(MAX_SEQ, hs, hs, cfg["rotary_base"])
    bounds = mpc.bounds("f16")
    dec = llmie.Decoder(cfg, eng)
    try:
        dec.set_qk_norm(qgd, kgd, qc.EPS)
        for name in ("gemv", "packed", "splitk"):
            bs = batch_of[name]
            assert llmie.decoder_plan_name(cfg, False, bs, call_flags=flags) == name
            lens = [150 - 11 * (b % 7) for b in range(bs)]
            shape = (L, bs, kvh, MAX_SEQ, hs)
            k0, v0, _, _ = mpc.draw_caches(rng, shape, "f16")
            refs = _Refs(cfg, ref_layers, k0, v0, tab, qg, kg, lambda rows, which: mpc.h16(rows))
            xs = mpc.h16(rng.standard_normal((bs, H)).astype(np.float32))
            kd, vd = torch.from_numpy(k0).to(DEV).to(F16), torch.from_numpy(v0).to(DEV).to(F16)
            od = torch.full((bs, H), 9.0, dtype=F16, device=DEV)
            dec.forward_ragged(torch.from_numpy(xs).to(DEV).to(F16), od, kd, vd, torch.tensor([c + 1 for c in lens], dtype=torch.int32, device=DEV))
            torch.cuda.synchronize()
            exp, others = refs.step(xs, [1] * bs, lens, None)
            _check(od, exp, others, bounds, "%s at batch %d" % (name, bs))
    finally:
        dec.close()


def test_the_qwen3_moe_layer(llmie):
    """the smallest ragged decode case of moe_engine_ref (3 rows, 4 heads over 2 of 64, two sparse layers of 8 experts, top-2) with
    LLMIE_MOE_SOFTMAX_ALL (norm_topk_prob = false) and QK-norm"""
    import moe_cases as mc
    import moe_engine_cases as me
    import moe_engine_ref as er
    case = dict(er.BY_ID["decode_ragged_e8_r3"], id="qwen3_moe_qknorm_r3")
    b = er.build(case)
    hs, L = case["hs"], len(case["sparse"])
    qg, kg = qc.gammas(L, hs, 19, *qc.GAMMA_RANGE["decode_only"])
    tab = llmie.rope_table(me.MAX_SEQ, hs, hs, 10000.0)
    y64, la = qc.moe_decode(b, False, qg, kg, qc.EPS, mc.SOFTMAX_ALL, tab)
    y16, lb = qc.moe_decode(b, True, qg, kg, qc.EPS, mc.SOFTMAX_ALL, tab)
    stable = er.stable_rows(la, lb, case["k"])
    plain16, _ = qc.moe_decode(b, True, None, None, qc.EPS, mc.SOFTMAX_ALL, tab)
    dec = me.moe_engine(llmie, b["weights"], case["sparse"], hs, case["k"], me.MAX_BATCH, flags=llmie.MOE_SOFTMAX_ALL)
    qgd, kgd = torch.from_numpy(qg).to(DEV), torch.from_numpy(kg).to(DEV)
    try:
        dec.set_qk_norm(qgd, kgd, qc.EPS)
        got = me.run_case(llmie, dec, b)
    finally:
        dec.close()
    assert np.isfinite(got).all() and stable.any()
    worst = max(systematic_error(got[m], y16[m])[0] for m in np.nonzero(stable)[0])
    print("Qwen3-MoE layer: worst stable row %.4f (bar 2e-2), %d of %d rows stable" % (worst, stable.sum(), len(stable)))
    assert worst <= 2e-2, worst
    assert min(systematic_error(plain16[m], y16[m])[0] for m in np.nonzero(stable)[0]) > 0.05, "QK-norm does not matter to this case"


def test_refusals(llmie):
    rng = np.random.default_rng(3)
    hs = 128
    nh, kvh, L = GEOMETRY[hs]
    g = lambda dtype=F16, layers=L, width=hs: torch.ones((layers, width), dtype=dtype, device=DEV)
    # an fp32 engine has no QKN instantiation
    cfg32 = dict(_cfg(llmie, hs, 2), dtype=llmie.F32, wfmt=llmie.W_F32)
    e32, _ = mpc.engine_layers(llmie, mpc.draw_layers(rng, nh, kvh, hs, INTER, L, f16=False), "f32")
    dec = llmie.Decoder(cfg32, e32)
    try:
        with pytest.raises(llmie.LlmieError, match=r"\(-2\).*QK-norm needs"):
            dec.set_qk_norm(g(), g())
        dec.set_qk_norm(None, None)
    finally:
        dec.close()
    # a layer with a QKV bias
    eb, _ = mpc.engine_layers(llmie, mpc.draw_layers(rng, nh, kvh, hs, INTER, L, qkv_bias=True), "f16")
    dec = llmie.Decoder(_cfg(llmie, hs, 2), eb)
    try:
        with pytest.raises(llmie.LlmieError, match=r"\(-2\).*QKV bias"):
            dec.set_qk_norm(g(), g())
    finally:
        dec.close()
    cfg = _cfg(llmie, hs, 2)
    eng, _ = mpc.engine_layers(llmie, mpc.draw_layers(rng, nh, kvh, hs, INTER, L), "f16")
    dec = llmie.Decoder(cfg, eng)
    try:
        # fp16 gammas of the engine's shape, both or none
        with pytest.raises(llmie.LlmieError, match="float16"):
            dec.set_qk_norm(g(torch.float32), g())
        with pytest.raises(llmie.LlmieError, match="float16"):
            dec.set_qk_norm(g(), g(width=64))
        with pytest.raises(llmie.LlmieError, match=r"\(-1\).*go together"):
            dec.set_qk_norm(g(), None)
        with pytest.raises(llmie.LlmieError, match=r"\(-1\).*eps"):
            dec.set_qk_norm(g(), g(), eps=-1.0)
        buf = torch.ones(L * hs + 8, dtype=F16, device=DEV)
        with pytest.raises(llmie.LlmieError, match=r"\(-1\).*16-byte aligned"):
            dec.set_qk_norm(buf[4:4 + L * hs].view(L, hs), g())
        # a window or head sinks first, then QK-norm ...
        dec.set_window([64, 0], 4)
        with pytest.raises(llmie.LlmieError, match=r"\(-2\).*QK-norm needs"):
            dec.set_qk_norm(g(), g())
        dec.set_window(None)
        sinks = torch.zeros((L, nh), device=DEV)
        dec.set_head_sinks(sinks)
        with pytest.raises(llmie.LlmieError, match=r"\(-2\).*QK-norm needs"):
            dec.set_qk_norm(g(), g())
        dec.set_head_sinks(None)
        # ... and QK-norm first, then a window or head sinks
        qgd, kgd = g(), g()
        dec.set_qk_norm(qgd, kgd)
        with pytest.raises(llmie.LlmieError, match=r"\(-2\).*QK-norm needs"):
            dec.set_window([64, 0], 4)
        with pytest.raises(llmie.LlmieError, match=r"\(-2\).*QK-norm needs"):
            dec.set_head_sinks(sinks)
        dec.set_window(None)
        dec.set_head_sinks(None)
        # QK-norm set, and a call whose caches are not 16-byte aligned (the generic kernel's operands): refused, nothing written
        n = L * 2 * kvh * MAX_SEQ * hs
        buf = torch.zeros(n + 8, dtype=F16, device=DEV)
        kd, vd = buf[4:4 + n].view(L, 2, kvh, MAX_SEQ, hs), torch.zeros((L, 2, kvh, MAX_SEQ, hs), dtype=F16, device=DEV)
        x = torch.randn((2, nh * hs), device=DEV).to(F16)
        with pytest.raises(llmie.LlmieError, match=r"\(-2\).*QK-norm"):
            dec.forward(x, torch.empty_like(x), kd, vd, 50)
        torch.cuda.synchronize()
        assert not bool(buf.any()) and not bool(vd.any())
    finally:
        dec.close()
