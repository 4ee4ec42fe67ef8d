"""The decoder engine on MXFP4 weights (llmie_decoder_config.wfmt = LLMIE_W_MXFP4): the oracle is given the DE-QUANTISED weights
(tests/mxfp4_cases.py restates the format; every weight is then exactly an fp16 number), so what is left is the fp16 pipeline's error,
held to the bounds the int4 engine tests hold it to.  Decode (the unfused sequence at one batch per projection route), prefill (the
general sequence below and from 192 rows, where the projections run on the fp16 image), paged and ragged calls against dense ones
bit for bit, the e4m3 cache, a captured step, a 7B-geometry layer, and the C++ adaptors' driver."""
import os
import subprocess

import numpy as np
import pytest
import torch

import mxfp4_cases as MX
import oracle as orc
from conftest import systematic_error

pytestmark = pytest.mark.gpu
DEV, F16 = "cuda", torch.float16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NH, HS, I_SMALL, L2 = 8, 128, 2816, 2
FRO, PROJ = 3e-3, 2e-4       # tests/test_quant_gpu.py, tests/test_prefill_gpu.py: the fp16 pipeline's systematic-error bounds


def _h(a):
    return a.astype(np.float16).astype(np.float32)


def _model(rng, nh, kvh, hs, I, L, llmie=None):
    """(engine layers on the device, oracle layers on the de-quantised weights).  llmie given: the device quantiser and de-quantiser
    (held to the restatement bit for bit by tests/test_mxfp4_linear_gpu.py) instead of the numpy ones, for the large matrices"""
    H, QKV = nh * hs, (nh + 2 * kvh) * hs
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    eng, ora = [], []
    for _ in range(L):
        g1, g2 = _h(rng.uniform(0.8, 1.2, H).astype(np.float32)), _h(rng.uniform(0.8, 1.2, H).astype(np.float32))
        e, o = dict(attn_norm=d(g1).to(F16), ffn_norm=d(g2).to(F16)), dict(attn_norm=g1, ffn_norm=g2, qkv_bias=None, o_bias=None)
        for name, (n, k) in dict(qkv=(QKV, H), o=(H, H), gate_up=(2 * I, H), down=(H, I)).items():
            w = (rng.uniform(-1, 1, (n, k)).astype(np.float32) * np.float32(2 / np.sqrt(k))).astype(np.float16)
            if llmie is not None:
                wq_d, sc_d = torch.empty((n, k // 2), dtype=torch.uint8, device=DEV), torch.empty((n, k // 32), dtype=torch.uint8, device=DEV)
                llmie.quantize_mxfp4(d(w), wq_d, sc_d)
                deq = llmie.dequantize_mxfp4(wq_d, sc_d, torch.empty((n, k), dtype=F16, device=DEV)).float().cpu().numpy()
                e[name], o[name] = dict(data=wq_d, scale=sc_d), deq
                continue
            wq, sc = MX.quantize(w)
            deq = MX.dequantize(wq, sc)
            assert np.array_equal(deq, deq.astype(np.float16).astype(np.float64))      # every weight is an fp16 number
            e[name], o[name] = dict(data=d(wq), scale=d(sc)), deq.astype(np.float32)
        eng.append(e)
        ora.append(o)
    return eng, ora


def _cfg(llmie, nh, kvh, hs, I, L, max_seq, max_batch, **kw):
    return dict(head_num=nh, kv_head_num=kvh, head_size=hs, inter_size=I, num_layers=L, vocab_size=100, max_seq_len=max_seq,
                max_batch=max_batch, rotary_dim=hs, rotary_base=10000.0, rms_eps=1e-5, dtype=llmie.F16, wfmt=llmie.W_MXFP4, int4_group=0, **kw)


def _ocfg(nh, kvh, hs, I, L, max_seq):
    return dict(head_num=nh, kv_head_num=kvh, head_size=hs, inter_size=I, num_layers=L, vocab=100, max_seq_len=max_seq, rotary_dim=hs,
                rotary_base=10000.0, rms_eps=1e-5)


def _check_decode(got, exp):
    err = np.abs(got - exp)
    print("max err %.3g (max err / bound %.3g)" % (err.max(), (err / (2e-2 + 2e-2 * np.abs(exp))).max()))
    assert (err <= 2e-2 + 2e-2 * np.abs(exp)).all(), err.max()
    fro, proj = systematic_error(got, exp)
    print("relative Frobenius error %.3g, projection on the signal %.3g" % (fro, proj))
    assert fro <= FRO and proj <= PROJ, "relative Frobenius error %.3g, projection on the signal %.3g" % (fro, proj)


@pytest.fixture(scope="module")
def small(llmie):
    """the two small models (kv 8 and kv 2), built and quantised once"""
    rng = np.random.default_rng(91)
    return {kvh: _model(rng, NH, kvh, HS, I_SMALL, L2) for kvh in (8, 2)}


# one batch per projection route: GEMV (1, 2), MFMA (9, 40), row chunks (70)
@pytest.mark.parametrize("bs,kvh", [(1, 8), (2, 2), (9, 8), (40, 2), (70, 8)])
def test_decode_matches_oracle_on_dequantised_weights(llmie, small, bs, kvh):
    rng = np.random.default_rng(92 + bs)
    max_seq, step, H = 160, 131, NH * HS
    eng, ora = small[kvh]
    cfg = _cfg(llmie, NH, kvh, HS, I_SMALL, L2, max_seq, bs)
    assert llmie.decoder_plan_name(cfg, False, bs) == "unfused"
    dec = llmie.Decoder(cfg, eng)
    x = _h(rng.standard_normal((bs, H)).astype(np.float32))
    kc = _h(rng.standard_normal((L2, bs, kvh, max_seq, HS)).astype(np.float32) * 0.5)
    vc = _h(rng.standard_normal((L2, bs, kvh, max_seq, HS)).astype(np.float32) * 0.5)
    xd = torch.from_numpy(x).to(DEV).to(F16)
    out = dec.forward(xd, torch.empty_like(xd), torch.from_numpy(kc).to(DEV).to(F16), torch.from_numpy(vc).to(DEV).to(F16), step)
    torch.cuda.synchronize()
    exp = orc.self_decoder(_ocfg(NH, kvh, HS, I_SMALL, L2, max_seq), ora, x, kc, vc, step)
    _check_decode(out.float().cpu().numpy(), exp)
    dec.close()


# ragged on a history: 128 tokens (MFMA + row chunks); 300 tokens: the projections run on the fp16 image
@pytest.mark.parametrize("name,kvh,lens,hist", [("ragged_hist", 8, [70, 40, 18], [0, 10, 64]), ("ragged_hist_gqa", 2, [70, 40, 18], [5, 0, 64]),
                                               ("image_300", 8, [300], [20])])
def test_prefill_matches_oracle_on_dequantised_weights(llmie, small, name, kvh, lens, hist):
    rng = np.random.default_rng(93)
    max_seq, H, bs, T = 384, NH * HS, len(lens), int(sum(lens))
    eng, ora = small[kvh]
    cfg = _cfg(llmie, NH, kvh, HS, I_SMALL, L2, max_seq, bs)
    assert llmie.decoder_plan_name(cfg, True, T) == "general"
    dec = llmie.Decoder(cfg, eng)
    x = _h(rng.standard_normal((T, H)).astype(np.float32))
    kc = _h(rng.standard_normal((L2, bs, kvh, max_seq, HS)).astype(np.float32) * 0.5)
    vc = _h(rng.standard_normal((L2, bs, kvh, max_seq, HS)).astype(np.float32) * 0.5)
    k0, v0 = kc.copy(), vc.copy()
    kd, vd = torch.from_numpy(kc).to(DEV).to(F16), torch.from_numpy(vc).to(DEV).to(F16)
    xd = torch.from_numpy(x).to(DEV).to(F16)
    out = dec.prefill(xd, torch.empty_like(xd), kd, vd, torch.tensor(lens, dtype=torch.int32, device=DEV),
                      torch.tensor(hist, dtype=torch.int32, device=DEV), max(lens))
    torch.cuda.synchronize()
    ocfg = dict(head_num=NH, kv_head_num=kvh, head_size=HS, inter_size=I_SMALL, rms_eps=1e-5, rotary_dim=HS, rotary_base=10000.0)
    exp = orc.context_decoder(ocfg, ora, x, kc, vc, np.array(lens, np.int32), np.array(hist, np.int32))   # appends into kc / vc
    got = out.float().cpu().numpy()
    err = np.abs(got - exp)
    print("max err %.3g (max err / bound %.3g)" % (err.max(), (err / (3e-2 + 3e-2 * np.abs(exp))).max()))
    assert (err <= 3e-2 + 3e-2 * np.abs(exp)).all(), "max err %g (|exp| max %g)" % (err.max(), np.abs(exp).max())
    fro, proj = systematic_error(got, exp)
    print("relative Frobenius error %.3g, projection on the signal %.3g" % (fro, proj))
    assert fro <= FRO and proj <= PROJ, "relative Frobenius error %.3g, projection on the signal %.3g" % (fro, proj)
    # every appended K / V row against the oracle's, every other row untouched
    for got_c, exp_c, old in ((kd.float().cpu().numpy(), kc, k0), (vd.float().cpu().numpy(), vc, v0)):
        for b in range(bs):
            new = slice(hist[b], hist[b] + lens[b])
            assert np.abs(got_c[:, b, :, new] - exp_c[:, b, :, new]).max() <= 2e-2
            rest = np.ones(max_seq, bool)
            rest[new] = False
            assert np.array_equal(got_c[:, b][:, :, rest], old[:, b][:, :, rest])
    dec.close()


def _pages(llmie, rng, kd, vd, bs, max_seq, ctx):
    max_pages = (max_seq + 127) // 128
    num_pages = bs * max_pages + 3
    perm = torch.from_numpy(rng.permutation(num_pages)[:bs * max_pages].astype(np.int32)).reshape(bs, max_pages).to(DEV)
    kp = torch.zeros((kd.shape[0], num_pages, kd.shape[2], 128, kd.shape[4]), dtype=kd.dtype, device=DEV)
    vp = torch.zeros_like(kp)
    llmie.kv_pages_copy(kd, kp, perm, ctx, True)
    llmie.kv_pages_copy(vd, vp, perm, ctx, True)
    return kp, vp, perm


@pytest.mark.parametrize("bs,kvh,kv8", [(3, 2, False), (20, 8, False), (2, 8, True)])
def test_paged_and_ragged_decode_are_bit_identical_to_dense(llmie, small, bs, kvh, kv8):
    rng = np.random.default_rng(94)
    max_seq, step, H = 300, 257, NH * HS
    eng, _ = small[kvh]
    kw = dict(kv_fmt=llmie.KV_FP8, k_scale=1 / 32, v_scale=1 / 16) if kv8 else {}
    cfg = _cfg(llmie, NH, kvh, HS, I_SMALL, L2, max_seq, bs, **kw)
    for flags in (llmie.PLAN_PAGED, llmie.PLAN_RAGGED, llmie.PLAN_PAGED | llmie.PLAN_RAGGED):
        assert llmie.decoder_plan_name(cfg, False, bs, call_flags=flags) == "unfused"
    dec = llmie.Decoder(cfg, eng)
    shape = (L2, bs, kvh, max_seq, HS)
    if kv8:
        kd, vd = torch.randint(0, 0x58, shape, device=DEV, dtype=torch.uint8), torch.randint(0, 0x58, shape, device=DEV, dtype=torch.uint8)
    else:
        kd, vd = (torch.randn(shape, device=DEV) * 0.5).to(F16), (torch.randn(shape, device=DEV) * 0.5).to(F16)
    x = torch.randn((bs, H), device=DEV).to(F16)
    # same step for every sequence: dense == paged == ragged == paged ragged
    ctx_prev = torch.full((bs,), step - 1, dtype=torch.int32, device=DEV)
    ctx = torch.full((bs,), step, dtype=torch.int32, device=DEV)
    kp, vp, perm = _pages(llmie, rng, kd, vd, bs, max_seq, ctx_prev)
    kp2, vp2 = kp.clone(), vp.clone()
    kd2, vd2 = kd.clone(), vd.clone()
    dense = dec.forward(x, torch.empty_like(x), kd, vd, step).clone()
    assert torch.isfinite(dense).all()
    assert torch.equal(dec.forward_paged(x, torch.empty_like(x), kp, vp, perm, step), dense)
    assert torch.equal(dec.forward_ragged(x, torch.empty_like(x), kd2, vd2, ctx), dense)
    assert torch.equal(dec.forward_paged_ragged(x, torch.empty_like(x), kp2, vp2, perm, ctx), dense)
    assert torch.equal(kd2, kd) and torch.equal(vd2, vd) and torch.equal(kp2, kp) and torch.equal(vp2, vp)
    kback = torch.zeros_like(kd)
    llmie.kv_pages_copy(kback, kp, perm, ctx, False)
    assert torch.equal(kback[:, :, :, :step], kd[:, :, :, :step])
    # really ragged lengths: row b of the ragged call == the batch's row at a dense call of that step
    lens = [step - 7 * b for b in range(bs)]
    ctxr = torch.tensor(lens, dtype=torch.int32, device=DEV)
    kp3, vp3, perm3 = _pages(llmie, rng, kd, vd, bs, max_seq, ctxr - 1)
    rag = dec.forward_ragged(x, torch.empty_like(x), kd.clone(), vd.clone(), ctxr).clone()
    assert torch.equal(dec.forward_paged_ragged(x, torch.empty_like(x), kp3, vp3, perm3, ctxr), rag)
    for b in (0, bs - 1):
        one = dec.forward(x, torch.empty_like(x), kd.clone(), vd.clone(), lens[b])
        assert torch.equal(one[b], rag[b])
    dec.close()


def test_paged_prefill_is_bit_identical_to_dense(llmie, small):
    rng = np.random.default_rng(95)
    kvh, lens, hist, max_seq, H = 8, [100, 64], [0, 0], 256, NH * HS
    bs, T = len(lens), sum(lens)
    eng, _ = small[kvh]
    dec = llmie.Decoder(_cfg(llmie, NH, kvh, HS, I_SMALL, L2, max_seq, bs), eng)
    kd = torch.zeros((L2, bs, kvh, max_seq, HS), dtype=F16, device=DEV)
    vd = torch.zeros_like(kd)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    kp, vp, perm = _pages(llmie, rng, kd, vd, bs, max_seq, i32([0] * bs))
    x = torch.randn((T, H), device=DEV).to(F16)
    dense = dec.prefill(x, torch.empty_like(x), kd, vd, i32(lens), i32(hist), max(lens)).clone()
    paged = dec.prefill_paged(x, torch.empty_like(x), kp, vp, perm, i32(lens), i32(hist), max(lens))
    assert torch.isfinite(dense).all() and torch.equal(paged, dense)
    kback, vback = torch.zeros_like(kd), torch.zeros_like(vd)
    llmie.kv_pages_copy(kback, kp, perm, i32(lens), False)
    llmie.kv_pages_copy(vback, vp, perm, i32(lens), False)
    for b in range(bs):
        assert torch.equal(kback[:, b, :, :lens[b]], kd[:, b, :, :lens[b]]) and torch.equal(vback[:, b, :, :lens[b]], vd[:, b, :, :lens[b]])
    dec.close()


def test_decode_with_e4m3_cache_matches_oracle_on_dequantised_caches(llmie, small):
    """the e4m3 cache through the unfused sequence's attention launch (tests/test_kvfp8_gpu.py: a long context, where the oracle's
    un-quantised new token is 1 of 300; the fp16 decoder tolerance of that test)"""
    from test_kvfp8_gpu import TAB, _to_e4m3, KS, VS
    rng = np.random.default_rng(96)
    bs, kvh, max_seq, step, H = 2, 8, 320, 300, NH * HS
    eng, ora = small[kvh]
    cfg = _cfg(llmie, NH, kvh, HS, I_SMALL, L2, max_seq, bs, kv_fmt=llmie.KV_FP8, k_scale=KS, v_scale=VS)
    assert llmie.decoder_plan_name(cfg, False, bs) == "unfused"
    dec = llmie.Decoder(cfg, eng)
    x = _h(rng.standard_normal((bs, H)).astype(np.float32))
    kq = _to_e4m3(rng.standard_normal((L2, bs, kvh, max_seq, HS)).astype(np.float32) * 0.7 / KS)
    vq = _to_e4m3(rng.standard_normal((L2, bs, kvh, max_seq, HS)).astype(np.float32) * 0.7 / VS)
    kc, vc = TAB[kq] * np.float32(KS), TAB[vq] * np.float32(VS)
    xd = torch.from_numpy(x).to(DEV).to(F16)
    out = dec.forward(xd, torch.empty_like(xd), torch.from_numpy(kq).to(DEV), torch.from_numpy(vq).to(DEV), step)
    torch.cuda.synchronize()
    exp = orc.self_decoder(_ocfg(NH, kvh, HS, I_SMALL, L2, max_seq), ora, x, kc, vc, step)
    err = np.abs(out.float().cpu().numpy() - exp)
    assert (err <= 3e-2 + 3e-2 * np.abs(exp)).all(), "max err %g (|exp| max %g)" % (err.max(), np.abs(exp).max())
    dec.close()


def test_captured_decode_step_replays_the_eager_result(llmie, small):
    kvh, bs, max_seq, H = 8, 9, 160, NH * HS
    eng, _ = small[kvh]
    dec = llmie.Decoder(_cfg(llmie, NH, kvh, HS, I_SMALL, L2, max_seq, bs), eng)
    shape = (L2, bs, kvh, max_seq, HS)
    k0, v0 = (torch.randn(shape, device=DEV) * 0.5).to(F16), (torch.randn(shape, device=DEV) * 0.5).to(F16)
    xs = [torch.randn((bs, H), device=DEV).to(F16) for _ in range(4)]
    steps = [100, 101, 102, 103]
    ke, ve = k0.clone(), v0.clone()
    eager = [dec.forward(x, torch.empty_like(x), ke, ve, s).clone() for x, s in zip(xs, steps)]
    torch.cuda.synchronize()
    kg, vg = k0.clone(), v0.clone()
    xin, out = torch.zeros_like(xs[0]), torch.zeros_like(xs[0])
    step_dev = torch.tensor([steps[0]], dtype=torch.int32, device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        dec.forward(xin, out, kg, vg, -1, step_dev=step_dev)
    kg.copy_(k0)
    vg.copy_(v0)
    for x, s, e in zip(xs, steps, eager):
        xin.copy_(x)
        step_dev.fill_(s)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, e)
    assert torch.equal(kg, ke) and torch.equal(vg, ve)
    dec.close()


@pytest.fixture(scope="module")
def layer_7b(llmie):
    return _model(np.random.default_rng(97), 32, 32, 128, 11008, 1, llmie)


@pytest.mark.parametrize("bs", [1, 40])
def test_7b_geometry_layer_matches_oracle(llmie, layer_7b, bs):
    rng = np.random.default_rng(98 + bs)
    nh, hs, I, max_seq, step = 32, 128, 11008, 96, 40
    H = nh * hs
    eng, ora = layer_7b
    cfg = _cfg(llmie, nh, nh, hs, I, 1, max_seq, bs)
    assert llmie.decoder_resident_weight_bytes(cfg) == sum(n * k // 2 + n * k // 32 for n, k in ((3 * H, H), (H, H), (2 * I, H), (H, I)))
    dec = llmie.Decoder(cfg, eng)
    x = _h(rng.standard_normal((bs, H)).astype(np.float32))
    kc = _h(rng.standard_normal((1, bs, nh, max_seq, hs)).astype(np.float32) * 0.5)
    vc = _h(rng.standard_normal((1, bs, nh, max_seq, hs)).astype(np.float32) * 0.5)
    xd = torch.from_numpy(x).to(DEV).to(F16)
    out = dec.forward(xd, torch.empty_like(xd), torch.from_numpy(kc).to(DEV).to(F16), torch.from_numpy(vc).to(DEV).to(F16), step)
    torch.cuda.synchronize()
    _check_decode(out.float().cpu().numpy(), orc.self_decoder(_ocfg(nh, nh, hs, I, 1, max_seq), ora, x, kc, vc, step))
    dec.close()


def test_refusals(llmie, small):
    eng, _ = small[8]
    cfg = _cfg(llmie, NH, 8, HS, I_SMALL, L2, 160, 4)
    with pytest.raises(llmie.LlmieError, match="MXFP4"):
        llmie.Decoder(dict(cfg, flags=llmie.DEC_PACKED_ONLY), eng)
    dec = llmie.Decoder(cfg, eng)
    H = NH * HS
    buf = torch.zeros(4 * H + 8, dtype=F16, device=DEV)
    x = torch.zeros((4, H), dtype=F16, device=DEV)
    kd = torch.zeros((L2, 4, 8, 160, HS), dtype=F16, device=DEV)
    with pytest.raises(llmie.LlmieError, match="16-byte aligned hidden_out"):
        dec.forward(x, buf[1:1 + 4 * H].view(4, H), kd, kd.clone(), 5)
    with pytest.raises(llmie.LlmieError, match="adapters need"):
        dec.lora_attach(llmie.lora_table(2, L2), torch.zeros(4, dtype=torch.int32, device=DEV))
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=DEV)
    logits = torch.zeros((4, 100), dtype=F16, device=DEV)
    with pytest.raises(llmie.LlmieError, match="MXFP4 LM head"):
        dec.lm_head_sample(x, torch.ones(H, dtype=F16, device=DEV), dict(data=eng[0]["o"]["data"], scale=eng[0]["o"]["scale"]), llmie.W_MXFP4,
                           logits, i32(4, 8, 4), torch.zeros((4, 8, 4), dtype=F16, device=DEV), i32(4, 4), torch.zeros((4, 4), dtype=F16, device=DEV),
                           i32(4), torch.zeros(4, dtype=torch.uint8, device=DEV), i32(4), step=5, end_id=2)
    torch.cuda.synchronize()
    dec.close()


def test_cpp_driver(llmie):
    exe = os.path.join(ROOT, "llm-inference-engine_amd", "cpp_tests", "test_mxfp4_api")
    assert os.path.exists(exe), "build() compiles the C++ drivers"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "all passed" in r.stdout
