"""Head sinks and RoPE scaling on an engine (llmie_decoder_set_head_sinks, llmie_decoder_set_rope_scaling).

An fp16 engine of 2 query heads over 1 KV head of 128 (2 layers, windows [W, 0]) runs a prefill and then three decode steps -- batch
1 (the fused GEMV sequence) and the paged-ragged entry -- and one of 4 heads over 2 of 64 (4 layers, windows [W, 0, W, 0]) runs decode
steps alone on a ragged batch, native and e4m3 cache; every layer has its own sink row and the table is the gpt-oss YaRN table set
through set_rope_scaling.  Held to the float64 layer restatement of tests/sink_engine_cases.py (the window-aware restatement with
the rotation taken from the table and one sink column per head) at model_param_cases.bounds().  The restatement without sinks, and
the one with the unscaled table, miss the same bounds by far (asserted), so an engine that ignored either would fail.

set_head_sinks(None) and set_rope_scaling(None) restore the bits recorded before they were set.  The gpt-oss layer -- MXFP4 experts
with the full epilogue attached through the _ex descriptor, a window, head sinks and YaRN on one engine -- runs the smallest case of
tests/moe_mxfp4_engine_ref.py against the oracle composition with the same attention, at its 2e-2 per stable row.  Refusals: an fp32
engine, a call whose attention would run on the generic kernel while sinks are set, RoPE scaling on a geometry whose decode
attention does not read the table.
"""
import numpy as np
import pytest
import torch

import model_param_cases as mpc
import sink_engine_cases as se
from conftest import systematic_error

pytestmark = pytest.mark.gpu
DEV, F16 = "cuda", torch.float16
INTER, MAX_SEQ = 512, 1024
W, S = 37, 4
GEOMETRY = {128: (2, 1, 2), 64: (4, 2, 4)}   # head size -> (heads, KV heads, layers)


def _cfg(llmie, hs, max_batch, e4m3=False, base=se.GPT_OSS_BASE):
    nh, kvh, L = GEOMETRY[hs]
    cfg = dict(head_num=nh, kv_head_num=kvh, head_size=hs, inter_size=INTER, num_layers=L, vocab_size=100, max_seq_len=MAX_SEQ,
               max_batch=max_batch, rotary_dim=hs, rotary_base=base, rms_eps=1e-5, dtype=llmie.F16, wfmt=llmie.W_F16, int4_group=128)
    if e4m3:
        cfg.update(kv_fmt=llmie.KV_FP8, k_scale=mpc.KS, v_scale=mpc.VS)
    return cfg


def _sinks(rng, L, nh):
    """one row per layer: logits around the typical maximum of a row's real logits, one head per layer without a sink"""
    s = rng.uniform(3.0, 7.0, (L, nh)).astype(np.float32)
    s[np.arange(L), np.arange(L) % nh] = -np.inf
    return s


def _check(got, exp, others, bounds, what):
    rtol, atol = bounds["elem"]
    got = got.double().cpu().numpy()
    err = np.abs(got - exp)
    assert (err <= atol + rtol * np.abs(exp)).all(), "%s: worst error / bound %.3g" % (what, (err / (atol + rtol * np.abs(exp))).max())
    fro, proj = systematic_error(got, exp)
    assert fro <= bounds["fro"] and proj <= bounds["proj"], (what, fro, proj)
    for name, other in others.items():
        assert systematic_error(other, exp)[0] > 10 * bounds["fro"], "%s: %s does not matter to this case" % (what, name)
    return fro


@pytest.mark.parametrize("kind", ["hs128_batch1", "hs128_paged_ragged", "hs64_ragged", "hs64_e4m3"])
def test_engine_with_head_sinks_windows_and_yarn(llmie, kind):
    hs = 128 if kind.startswith("hs128") else 64
    nh, kvh, L = GEOMETRY[hs]
    H = nh * hs
    prefill = hs == 128
    lens = {"hs128_batch1": [150], "hs128_paged_ragged": [150, 70, 129], "hs64_ragged": [150, 70, 129], "hs64_e4m3": [150, 70]}[kind]
    bs, e4m3, paged = len(lens), kind == "hs64_e4m3", kind == "hs128_paged_ragged"
    windows = [W, 0] * (L // 2)
    rng = np.random.default_rng(7)
    layers = mpc.draw_layers(rng, nh, kvh, hs, INTER, L)
    eng, ref_layers = mpc.engine_layers(llmie, layers, "f16")
    cfg = _cfg(llmie, hs, bs, e4m3)
    dec = llmie.Decoder(cfg, eng)
    bounds = mpc.bounds("f16", "paged_e4m3" if e4m3 else "dense")
    ks, vs = (cfg["k_scale"], cfg["v_scale"]) if e4m3 else (1.0, 1.0)
    store = (lambda rows, which: mpc.e4m3_cache_rounding(rows, (ks, vs)[which])) if e4m3 else (lambda rows, which: mpc.h16(rows))
    sinks = _sinks(rng, L, nh)
    sinks_dev = torch.from_numpy(sinks).to(DEV)
    tab = llmie.rope_table(MAX_SEQ, hs, hs, cfg["rotary_base"], se.GPT_OSS_YARN)
    tab_plain = llmie.rope_table(MAX_SEQ, hs, hs, cfg["rotary_base"])
    shape = (L, bs, kvh, MAX_SEQ, hs)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    mp = MAX_SEQ // 128
    table = i32(np.random.default_rng(5).permutation(bs * mp + 2)[:bs * mp].reshape(bs, mp)) if paged else None
    cshape = (L, bs * mp + 2, kvh, 128, hs) if paged else shape
    # decode-only engines start from caches that already hold the contexts
    k0, v0, kq, vq = mpc.draw_caches(rng, shape, "f16", "paged_e4m3" if e4m3 else "dense")
    if prefill:
        k0, v0 = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    new_cache = lambda a, q: torch.zeros(cshape, dtype=F16, device=DEV) if prefill else torch.from_numpy(q if e4m3 else a).to(DEV).to(torch.uint8 if e4m3 else F16)
    # the three restatements: the engine's, one that ignores the sinks, one that rotates by the unscaled table
    refs = {name: (k0.astype(np.float64).copy(), v0.astype(np.float64).copy()) for name in ("exp", "no sinks", "unscaled table")}
    args = {"exp": (sinks, tab), "no sinks": (None, tab), "unscaled table": (sinks, tab_plain)}

    def restate(x, lens_, hist_, stored):
        out = {}
        for name, (kc, vc) in refs.items():
            out[name] = se.layer_restatement(cfg, ref_layers, x, kc, vc, lens_, hist_, windows, S, args[name][0], args[name][1], store,
                                             stored if name == "exp" else None)
        return out.pop("exp"), out

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
        elif bs == 1:
            dec.forward(xsd, od, kd, vd, new_ctx[0])
        else:
            dec.forward_ragged(xsd, od, kd, vd, i32(new_ctx))
        return od

    xs0 = torch.from_numpy(mpc.h16(rng.standard_normal((bs, H)).astype(np.float32))).to(DEV).to(F16)
    first = lambda: run_prefill(new_cache(k0, kq), new_cache(v0, vq)) if prefill else run_decode(xs0, new_cache(k0, kq), new_cache(v0, vq), [c + 1 for c in lens])
    try:
        plain = first()   # before anything is set
        dec.set_window(windows, S)
        dec.set_head_sinks(sinks_dev)
        dec.set_rope_scaling(se.GPT_OSS_YARN)
        kd, vd = new_cache(k0, kq), new_cache(v0, vq)
        dev = lambda: (mpc.TAB[kd.cpu().numpy()] * np.float32(ks), mpc.TAB[vd.cpu().numpy()] * np.float32(vs)) if e4m3 else None
        ctx = list(lens)
        if prefill:
            out = run_prefill(kd, vd)
            torch.cuda.synchronize()
            exp, others = restate(x, lens, [0] * bs, dev())
            _check(out, exp, others, bounds, "%s prefill" % kind)
        for step in range(3):
            xs = mpc.h16(rng.standard_normal((bs, H)).astype(np.float32))
            new_ctx = [c + 1 for c in ctx]
            od = run_decode(torch.from_numpy(xs).to(DEV).to(F16), kd, vd, new_ctx)
            torch.cuda.synchronize()
            exp, others = restate(xs, [1] * bs, ctx, dev())
            _check(od, exp, others, bounds, "%s decode step %d" % (kind, step))
            ctx = new_ctx
        # back, one at a time: the bits recorded before anything was set
        dec.set_window(None)
        dec.set_head_sinks(None)
        assert not torch.equal(first(), plain), "the scaled table changes nothing"
        dec.set_rope_scaling(None)
        assert torch.equal(first(), plain), "set_head_sinks(None) + set_rope_scaling(None) did not restore the pass"
        dec.set_head_sinks(sinks_dev)
        assert not torch.equal(first(), plain), "the sinks change nothing"
        dec.set_head_sinks(None)
        assert torch.equal(first(), plain)
        torch.cuda.synchronize()
    finally:
        dec.close()


def test_the_gpt_oss_layer_experts_window_sinks_and_yarn(llmie):
    """the smallest case of moe_mxfp4_engine_ref (3 ragged rows, 4 heads over 2 of 64, two sparse layers) with the full epilogue"""
    import moe_engine_cases as me
    import moe_engine_ref as er
    import moe_mxfp4_engine_ref as xr
    from test_moe_mxfp4_engine_gpu import descriptors
    case = dict(xr.BY_ID["mx4_decode_ragged_e8_r3"], epi=True, id="mx4_gptoss_sink_r3")
    b = xr.build(case)
    hs, L = case["hs"], len(case["sparse"])
    nh, kvh = er.geometry(hs)
    windows, sink_tokens = [64, 0], 4
    sinks = _sinks(np.random.default_rng(9), L, nh)
    tab = llmie.rope_table(me.MAX_SEQ, hs, hs, 10000.0, se.GPT_OSS_YARN)
    y64, la = se.moe_decode(b, False, sinks, tab, windows, sink_tokens)
    y16, lb = se.moe_decode(b, True, sinks, tab, windows, sink_tokens)
    stable = er.stable_rows(la, lb, case["k"])
    plain16, _ = se.moe_decode(b, True, np.full_like(sinks, -np.inf), llmie.rope_table(me.MAX_SEQ, hs, hs, 10000.0), [0, 0], 0)
    dec = me.make_engine(llmie, b["weights"], hs)
    sinks_dev = torch.from_numpy(sinks).to(DEV)
    try:
        dec.moe_attach(descriptors(llmie, b["weights"], case["sparse"], True), case["k"], max_tokens=me.MAX_BATCH)
        dec.set_window(windows, sinks=sink_tokens)
        dec.set_head_sinks(sinks_dev)
        dec.set_rope_scaling(se.GPT_OSS_YARN)
        got = me.run_case(llmie, dec, b)
    finally:
        dec.close()
    assert np.isfinite(got).all() and stable.any()
    worst = max(systematic_error(got[m], y16[m])[0] for m in np.nonzero(stable)[0])
    print("gpt-oss layer: worst stable row %.4f (bar 2e-2), %d of %d rows stable" % (worst, stable.sum(), len(stable)))
    assert worst <= 2e-2, worst
    assert min(systematic_error(plain16[m], y16[m])[0] for m in np.nonzero(stable)[0]) > 0.05, "window, sinks and YaRN do not matter to this case"


def test_refusals(llmie):
    rng = np.random.default_rng(3)
    # an fp32 engine has no SINK instantiation
    nh, kvh, hs = 2, 1, 128
    cfg32 = dict(_cfg(llmie, 128, 2), dtype=llmie.F32, wfmt=llmie.W_F32)
    e32, _ = mpc.engine_layers(llmie, mpc.draw_layers(rng, nh, kvh, hs, INTER, 2, f16=False), "f32")
    dec = llmie.Decoder(cfg32, e32)
    try:
        with pytest.raises(llmie.LlmieError, match=r"\(-2\).*head sinks need"):
            dec.set_head_sinks(torch.zeros((2, nh), device=DEV))
        dec.set_head_sinks(None)
        dec.set_rope_scaling(se.GPT_OSS_YARN)   # (its decode attention reads the table: allowed)
    finally:
        dec.close()
    # a geometry whose decode attention rotates by rotary_base: no table to scale
    cfg3 = dict(_cfg(llmie, 64, 2), head_num=6, kv_head_num=2, num_layers=1)
    e3, _ = mpc.engine_layers(llmie, mpc.draw_layers(rng, 6, 2, 64, INTER, 1), "f16")
    dec = llmie.Decoder(cfg3, e3)
    try:
        with pytest.raises(llmie.LlmieError, match=r"\(-2\).*rotary_base"):
            dec.set_rope_scaling(se.GPT_OSS_YARN)
        with pytest.raises(llmie.LlmieError, match=r"\(-2\).*head sinks need"):
            dec.set_head_sinks(torch.zeros((1, 6), device=DEV))
    finally:
        dec.close()
    # sinks set, and a call whose caches are not 16-byte aligned (the generic kernel's operands): refused, nothing written
    cfg = _cfg(llmie, 128, 2)
    eng, _ = mpc.engine_layers(llmie, mpc.draw_layers(rng, nh, kvh, hs, INTER, 2), "f16")
    dec = llmie.Decoder(cfg, eng)
    try:
        with pytest.raises(llmie.LlmieError, match="float32"):
            dec.set_head_sinks(torch.zeros((2, nh), dtype=F16, device=DEV))
        with pytest.raises(llmie.LlmieError, match="factor"):
            dec.set_rope_scaling(dict(se.GPT_OSS_YARN, factor=0.5))
        dec.set_head_sinks(torch.zeros((2, nh), device=DEV))
        n = 2 * 2 * kvh * MAX_SEQ * hs
        buf = torch.zeros(n + 8, dtype=F16, device=DEV)
        kd, vd = buf[4:4 + n].view(2, 2, kvh, MAX_SEQ, hs), torch.zeros((2, 2, kvh, MAX_SEQ, hs), dtype=F16, device=DEV)
        x = torch.randn((2, nh * hs), device=DEV).to(F16)
        with pytest.raises(llmie.LlmieError, match=r"\(-2\).*head sink"):
            dec.forward(x, torch.empty_like(x), kd, vd, 50)
        torch.cuda.synchronize()
        assert not bool(buf.any())
    finally:
        dec.close()
