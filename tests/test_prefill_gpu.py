"""Prefill (context decoder) engine path: llmie_decoder_prefill (flash attention, packed tokens) against the oracle's
composition of the reference kernels (context_decoder.cpp:58-199 / context_attention.cpp:143-312), ragged batches with
history, GQA, several q/k tiles; plus the size-independent property prefill(n+1)[-1] == prefill(n) -> decode(n+1)."""
import numpy as np
import pytest
import torch

import oracle as orc
from conftest import systematic_error

FRO_F16, PROJ_F16 = 3e-3, 2e-4   # measured: 0.45e-3 .. 1.0e-3 and <= 1.1e-5 over the cases below; a 1 % gain error gives 1e-2 on both

pytestmark = pytest.mark.gpu
DEV, F16 = "cuda", torch.float16


def _h(a):
    return a.astype(np.float16).astype(np.float32)


def _model(rng, nh, kvh, hs, I, L, o_bias=False):
    H, QKV = nh * hs, (nh + 2 * kvh) * hs
    u = lambda shape, s: _h(rng.uniform(-1, 1, shape).astype(np.float32) * s)
    return [dict(attn_norm=_h(u((H,), 0.2) + 1), qkv=u((QKV, H), 2 / np.sqrt(H)), qkv_bias=None, o=u((H, H), 2 / np.sqrt(H)),
                 o_bias=u((H,), 0.1) if o_bias else None, ffn_norm=_h(u((H,), 0.2) + 1),
                 gate_up=u((2 * I, H), 2 / np.sqrt(H)), down=u((H, I), 2 / np.sqrt(I))) for _ in range(L)]


def _engine(llmie, layers, nh, kvh, hs, I, max_seq, max_batch):
    d = lambda a: None if a is None else torch.from_numpy(a).to(DEV).to(F16)
    eng = [dict(attn_norm=d(w["attn_norm"]), ffn_norm=d(w["ffn_norm"]), qkv=dict(data=d(w["qkv"])),
                o=dict(data=d(w["o"]), bias=d(w["o_bias"])), gate_up=dict(data=d(w["gate_up"])), down=dict(data=d(w["down"])))
           for w in layers]
    cfg = dict(head_num=nh, kv_head_num=kvh, head_size=hs, inter_size=I, num_layers=len(layers), vocab_size=100,
               max_seq_len=max_seq, max_batch=max_batch, rotary_dim=hs, rotary_base=10000.0, rms_eps=1e-5, dtype=llmie.F16,
               wfmt=llmie.W_F16, int4_group=128)
    return llmie.Decoder(cfg, eng)


def oracle_prefill(layers, x, kc, vc, lens, hist, nh, kvh, hs, I, max_seq):
    """kc/vc updated in place; returns hidden [T,H] (the oracle front-end's composition of the kernel oracles)"""
    cfg = dict(head_num=nh, kv_head_num=kvh, head_size=hs, inter_size=I, rms_eps=1e-5, rotary_dim=hs, rotary_base=10000.0)
    return orc.context_decoder(cfg, layers, x, kc, vc, lens, hist)


CASES = [("single_40", 8, 8, 1376, 2, [40], [0]), ("ragged_hist", 8, 8, 1376, 2, [70, 5, 33], [0, 10, 64]),
         ("gqa", 8, 2, 1024, 1, [17, 64], [3, 0]), ("long_300_bias", 8, 8, 512, 1, [300], [20]),
         # the three forms of the flash kernel (prefill_attention_f16 picks by grid and by the longest sequence): the cases above have
         # fewer 128-row query tiles than the chip has CUs -> 64 query rows per workgroup; 2 tiles x 16 heads x 8 sequences = 256 and
         # <= 512 rows per sequence -> 4 waves x 2 x 16 rows; > 512 rows -> 8 waves x 16 rows
         ("rt2_ragged_gqa", 16, 4, 512, 1, [256, 130, 200, 256, 129, 20, 255, 140], [0, 7, 0, 64, 0, 3, 100, 0]),
         ("w8_long_1100_600", 16, 16, 512, 1, [1100, 600], [20, 0])]


@pytest.mark.parametrize("name,nh,kvh,I,L,lens,hist", CASES, ids=[c[0] for c in CASES])
def test_prefill_matches_oracle(llmie, name, nh, kvh, I, L, lens, hist):
    rng = np.random.default_rng(41)
    hs, max_seq = 128, max(384, -(-max(h + l for h, l in zip(hist, lens)) // 128) * 128)
    H, bs, T = nh * hs, len(lens), int(sum(lens))
    layers = _model(rng, nh, kvh, hs, I, L, o_bias="bias" in name)
    dec = _engine(llmie, layers, nh, kvh, hs, I, max_seq, bs)
    x = _h(rng.standard_normal((T, H)).astype(np.float32))
    kc = _h(rng.standard_normal((L, bs, kvh, max_seq, hs)).astype(np.float32) * 0.5)
    vc = _h(rng.standard_normal((L, bs, kvh, max_seq, hs)).astype(np.float32) * 0.5)
    kd, vd = torch.from_numpy(kc).to(DEV).to(F16), torch.from_numpy(vc).to(DEV).to(F16)
    xd = torch.from_numpy(x).to(DEV).to(F16)
    out = torch.empty_like(xd)
    dec.prefill(xd, out, kd, vd, torch.tensor(lens, dtype=torch.int32, device=DEV),
                torch.tensor(hist, dtype=torch.int32, device=DEV), max(lens))
    exp = oracle_prefill(layers, x, kc, vc, np.array(lens, np.int32), np.array(hist, np.int32), nh, kvh, hs, I, max_seq)
    got = out.float().cpu().numpy()
    err = np.abs(got - exp)
    assert (err <= 3e-2 + 3e-2 * np.abs(exp)).all(), "max err %g (|exp| max %g)" % (err.max(), np.abs(exp).max())
    fro, proj = systematic_error(got, exp)   # a gain error of a whole layer would sit under the element-wise bound: these see it
    assert fro <= FRO_F16 and proj <= PROJ_F16, "relative Frobenius error %.3g, projection on the signal %.3g" % (fro, proj)
    assert np.abs(kd.float().cpu().numpy() - kc).max() <= 2e-2  # appended rows only differ by rounding; rest untouched
    dec.close()


def test_prefill_with_peaked_attention_rows(llmie):
    """Softmax rows with a large spread of logits (QKV weights scaled so that |q . k| / sqrt(d) reaches the tens, i.e. dozens of
    powers of two between the keys of one row): the flash kernel's numerators are fp16, so its running row maximum must be a TRUE
    maximum over all four lanes of a row -- with a merely consistent stabiliser (what a mis-lowered row swap produced for a few
    hours of round 3: the local maximum of one lane's 16 keys) numerators far above 1 overflow to inf and the output is NaN."""
    rng = np.random.default_rng(47)
    nh, kvh, hs, I, L, max_seq = 8, 8, 128, 512, 1, 384
    H, lens, hist = nh * hs, [300, 77], [0, 5]
    bs, T = len(lens), int(sum(lens))
    layers = _model(rng, nh, kvh, hs, I, L)
    layers[0]["qkv"][: 2 * nh * hs] *= np.float32(5.0)   # q and k rows x 5: logits x 25
    layers[0]["qkv"] = _h(layers[0]["qkv"])
    dec = _engine(llmie, layers, nh, kvh, hs, I, max_seq, bs)
    x = _h(rng.standard_normal((T, H)).astype(np.float32))
    kc = _h(rng.standard_normal((L, bs, kvh, max_seq, hs)).astype(np.float32) * 2.0)
    vc = _h(rng.standard_normal((L, bs, kvh, max_seq, hs)).astype(np.float32) * 0.5)
    kd, vd = torch.from_numpy(kc).to(DEV).to(F16), torch.from_numpy(vc).to(DEV).to(F16)
    xd = torch.from_numpy(x).to(DEV).to(F16)
    out = torch.empty_like(xd)
    dec.prefill(xd, out, kd, vd, torch.tensor(lens, dtype=torch.int32, device=DEV), torch.tensor(hist, dtype=torch.int32, device=DEV), max(lens))
    exp = oracle_prefill(layers, x, kc, vc, np.array(lens, np.int32), np.array(hist, np.int32), nh, kvh, hs, I, max_seq)
    got = out.float().cpu().numpy()
    assert np.isfinite(got).all(), "non-finite outputs: %d" % int((~np.isfinite(got)).sum())
    # a peaked softmax amplifies the fp16 rounding of q and k (logits of +-40 move by ~0.02): looser than the smooth cases, still
    # far below what a wrong normalisation gives
    fro, _ = systematic_error(got, exp)
    assert fro <= 2e-2, "relative Frobenius error %.3g" % fro
    dec.close()


def _quantise(w, fmt, group=128):
    """numpy definition of the engine's quantisers (tests/test_quant_gpu.py checks the device quantisers against it bit for bit):
    returns (codes, scales, de-quantised fp32 weights)"""
    if fmt == "int8":
        s = (np.abs(w).max(axis=1) / np.float32(127.0)).astype(np.float16)
        s[s == 0] = np.float16(1.0)
        q = np.clip(np.rint(w / s.astype(np.float32)[:, None]), -127, 127).astype(np.int8)
        return q, s, q.astype(np.float32) * s.astype(np.float32)[:, None]
    N, K = w.shape
    wg = w.reshape(N, K // group, group)
    s = (np.abs(wg).max(axis=2) / np.float32(7.0)).astype(np.float16)
    s[s == 0] = np.float16(1.0)
    q = np.clip(np.rint(wg / s.astype(np.float32)[:, :, None]), -8, 7).astype(np.int32)
    deq = (q.astype(np.float32) * s.astype(np.float32)[:, :, None]).reshape(N, K)
    q = q.reshape(N, K) + 8
    return (q[:, 0::2] | (q[:, 1::2] << 4)).astype(np.uint8), s, deq


QCASES = CASES + [("short_64", 8, 8, 1024, 2, [30, 34], [0, 7]), ("mid_150", 8, 8, 1024, 1, [150], [0])]


@pytest.mark.parametrize("fmt", ["int8", "int4"])
@pytest.mark.parametrize("name,nh,kvh,I,L,lens,hist", QCASES, ids=[c[0] for c in QCASES])
def test_quantised_prefill_matches_oracle_on_dequantised_weights(llmie, fmt, name, nh, kvh, I, L, lens, hist):
    """weight-only int8 / int4 engines (round 3): llmie_decoder_prefill on the quantised matrices against the oracle's context decoder
    on the DE-QUANTISED weights -- the error left is the fp16 pipeline's, held to the fp16 prefill bounds (<= 64 / 128 tokens: fused
    split-K form; up to 191: split-K passes; from 192: the prefill-sized forms of linear_wq)"""
    rng = np.random.default_rng(43)
    hs, max_seq = 128, max(384, -(-max(h + l for h, l in zip(hist, lens)) // 128) * 128)
    H, bs, T = nh * hs, len(lens), int(sum(lens))
    if fmt == "int4":
        I = I // 128 * 128   # group-128 scales along K: the down projection's K = I is a whole number of groups
    layers = _model(rng, nh, kvh, hs, I, L, o_bias="bias" in name)
    d = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
    eng, olayers = [], []
    for w in layers:
        e = dict(attn_norm=d(w["attn_norm"]).to(F16), ffn_norm=d(w["ffn_norm"]).to(F16))
        o = dict(w)
        for m in ("qkv", "o", "gate_up", "down"):
            q, s, deq = _quantise(w[m], fmt)
            e[m] = dict(data=d(q), scale=d(s))
            o[m] = deq
        e["o"]["bias"] = None if w["o_bias"] is None else d(w["o_bias"]).to(F16)
        eng.append(e)
        olayers.append(o)
    cfg = dict(head_num=nh, kv_head_num=kvh, head_size=hs, inter_size=I, num_layers=L, vocab_size=100, max_seq_len=max_seq, max_batch=bs,
               rotary_dim=hs, rotary_base=10000.0, rms_eps=1e-5, dtype=llmie.F16, wfmt=llmie.W_INT8 if fmt == "int8" else llmie.W_INT4,
               int4_group=128)
    dec = llmie.Decoder(cfg, eng)
    x = _h(rng.standard_normal((T, H)).astype(np.float32))
    kc = _h(rng.standard_normal((L, bs, kvh, max_seq, hs)).astype(np.float32) * 0.5)
    vc = _h(rng.standard_normal((L, bs, kvh, max_seq, hs)).astype(np.float32) * 0.5)
    kd, vd = torch.from_numpy(kc).to(DEV).to(F16), torch.from_numpy(vc).to(DEV).to(F16)
    xd = torch.from_numpy(x).to(DEV).to(F16)
    out = torch.empty_like(xd)
    dec.prefill(xd, out, kd, vd, torch.tensor(lens, dtype=torch.int32, device=DEV), torch.tensor(hist, dtype=torch.int32, device=DEV), max(lens))
    exp = oracle_prefill(olayers, x, kc, vc, np.array(lens, np.int32), np.array(hist, np.int32), nh, kvh, hs, I, max_seq)
    got = out.float().cpu().numpy()
    err = np.abs(got - exp)
    assert (err <= 3e-2 + 3e-2 * np.abs(exp)).all(), "max err %g (|exp| max %g)" % (err.max(), np.abs(exp).max())
    fro, proj = systematic_error(got, exp)
    assert fro <= FRO_F16 and proj <= PROJ_F16, "relative Frobenius error %.3g, projection on the signal %.3g" % (fro, proj)
    assert np.abs(kd.float().cpu().numpy() - kc).max() <= 2e-2
    dec.close()


def _engine_fmt(llmie, layers, fmt, nh, kvh, hs, I, max_seq, max_batch, offset=None):
    """engine in `fmt` on `layers` + the oracle's layers (de-quantised weights for int8 / int4); offset: None, "weights" or
    "gammas_weights" -- those operands handed over as views 8 bytes past a 16-byte boundary (e.g. views into one flat buffer)"""
    def d(a, off=False):
        if a is None:
            return None
        t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        t = t.to(F16) if t.is_floating_point() else t
        if not off:
            return t
        n = 8 // t.element_size()
        buf = torch.empty(t.numel() + n, dtype=t.dtype, device=DEV)
        v = buf[n:].view(t.shape)
        v.copy_(t)
        return v
    eng, olayers = [], []
    for w in layers:
        e = dict(attn_norm=d(w["attn_norm"], offset == "gammas_weights"), ffn_norm=d(w["ffn_norm"], offset == "gammas_weights"))
        o = dict(w)
        for m in ("qkv", "o", "gate_up", "down"):
            if fmt == "f16":
                e[m] = dict(data=d(w[m], offset is not None))
            else:
                q, s, deq = _quantise(w[m], fmt)
                e[m] = dict(data=d(q, offset is not None), scale=d(s))
                o[m] = deq
        e["o"]["bias"] = d(w["o_bias"])
        eng.append(e)
        olayers.append(o)
    cfg = dict(head_num=nh, kv_head_num=kvh, head_size=hs, inter_size=I, num_layers=len(layers), vocab_size=100, max_seq_len=max_seq,
               max_batch=max_batch, rotary_dim=hs, rotary_base=10000.0, rms_eps=1e-5, dtype=llmie.F16,
               wfmt=dict(f16=llmie.W_F16, int8=llmie.W_INT8, int4=llmie.W_INT4)[fmt], int4_group=128)
    return llmie.Decoder(cfg, eng), olayers


def _prefill_vs_oracle(dec, olayers, rng, nh, kvh, hs, I, max_seq, lens, hist, label):
    L, H, bs, T = len(olayers), nh * hs, len(lens), int(sum(lens))
    x = _h(rng.standard_normal((T, H)).astype(np.float32))
    kc = _h(rng.standard_normal((L, bs, kvh, max_seq, hs)).astype(np.float32) * 0.5)
    vc = _h(rng.standard_normal((L, bs, kvh, max_seq, hs)).astype(np.float32) * 0.5)
    kd, vd = torch.from_numpy(kc).to(DEV).to(F16), torch.from_numpy(vc).to(DEV).to(F16)
    xd = torch.from_numpy(x).to(DEV).to(F16)
    out = torch.empty_like(xd)
    dec.prefill(xd, out, kd, vd, torch.tensor(lens, dtype=torch.int32, device=DEV), torch.tensor(hist, dtype=torch.int32, device=DEV), max(lens))
    exp = oracle_prefill(olayers, x, kc, vc, np.array(lens, np.int32), np.array(hist, np.int32), nh, kvh, hs, I, max_seq)
    got = out.float().cpu().numpy()
    err = np.abs(got - exp)
    assert (err <= 3e-2 + 3e-2 * np.abs(exp)).all(), "%s: max err %g (|exp| max %g)" % (label, err.max(), np.abs(exp).max())
    fro, proj = systematic_error(got, exp)
    assert fro <= FRO_F16 and proj <= PROJ_F16, "%s: relative Frobenius error %.3g, projection on the signal %.3g" % (label, fro, proj)
    assert np.abs(kd.float().cpu().numpy() - kc).max() <= 2e-2, label
    assert np.abs(vd.float().cpu().numpy() - vc).max() <= 2e-2, label


# token counts across the projection routes of a small model: GEMV (5), skinny / split-K (40), the 65..192 forms (100, 150), the
# prefill-sized forms (300); single sequences without history and ragged batches with history
ODD_LENS = [([5], [0]), ([40], [0]), ([100], [0]), ([150], [0]), ([300], [0]), ([70, 30], [0, 9]), ([150, 4, 146], [3, 0, 21])]
# H = 384 / 1152 (head_num 3 / 9: not multiples of 256, H < 512 for 3), I not a multiple of 16 / 128, with and without an output
# bias (the lean in-place sequence and the classic one)
ODD = [("h384_kv1_i1000", 3, 1, 1000, False), ("h384_kv3_i1024_bias", 3, 3, 1024, True),
       ("h1152_kv3_i1000_bias", 9, 3, 1000, True), ("h1152_kv9_i1024", 9, 9, 1024, False)]


@pytest.mark.parametrize("fmt", ["f16", "int8", "int4"])
@pytest.mark.parametrize("name,nh,kvh,I,o_bias", ODD, ids=[c[0] for c in ODD])
def test_odd_shape_prefill_matches_oracle(llmie, fmt, name, nh, kvh, I, o_bias):
    """shapes config_ok accepts but no other prefill case uses: used to refuse (LLMIE_ERR_UNSUPPORTED) where the gate/up projection
    was sent to a fused SwiGLU form the shape does not have -- fp16 H < 512 at 65..192 tokens (and I % 16 != 0 below), int8
    H % 256 != 0 at 9..191 tokens"""
    rng = np.random.default_rng(53 + nh + I)
    hs, L, max_seq = 128, 2, 384
    if fmt == "int4":
        I = I // 128 * 128   # group-128 scales along K of the down projection
    layers = _model(rng, nh, kvh, hs, I, L, o_bias=o_bias)
    dec, olayers = _engine_fmt(llmie, layers, fmt, nh, kvh, hs, I, max_seq, 3)
    for lens, hist in ODD_LENS:
        _prefill_vs_oracle(dec, olayers, rng, nh, kvh, hs, I, max_seq, lens, hist, "%s %s lens %s hist %s" % (fmt, name, lens, hist))
    dec.close()


@pytest.mark.parametrize("fmt", ["f16", "int8", "int4"])
@pytest.mark.parametrize("offset", ["weights", "gammas_weights"])
def test_prefill_with_weights_at_8_byte_offsets(llmie, fmt, offset):
    """weight matrices (and norm gammas) handed over as views 8 bytes past a 16-byte boundary: the split-K short path, the fused
    SwiGLU forms and the out-of-place norms of the lean sequence take 16-byte vectors only -- such prefills must run the general
    kernels instead of refusing.  (max_batch 1: engines with a packed copy for batch decode need 16-byte aligned weights at create.)"""
    rng = np.random.default_rng(59)
    nh, hs, I, L, max_seq = 8, 128, 1024, 2, 384
    layers = _model(rng, nh, nh, hs, I, L)
    dec, olayers = _engine_fmt(llmie, layers, fmt, nh, nh, hs, I, max_seq, 1, offset=offset)
    for T in (5, 40, 100, 300):
        _prefill_vs_oracle(dec, olayers, rng, nh, nh, hs, I, max_seq, [T], [0], "%s %s T %d" % (fmt, offset, T))
    dec.close()


def test_prefill_then_decode_consistency(llmie):
    rng = np.random.default_rng(42)
    nh, hs, I, L, max_seq, n = 8, 128, 1376, 2, 256, 150
    H = nh * hs
    layers = _model(rng, nh, nh, hs, I, L)
    dec = _engine(llmie, layers, nh, nh, hs, I, max_seq, 1)
    xs = torch.from_numpy(_h(rng.standard_normal((n + 1, H)).astype(np.float32))).to(DEV).to(F16)
    z = lambda: torch.zeros((L, 1, nh, max_seq, hs), dtype=F16, device=DEV)
    k1, v1, k2, v2 = z(), z(), z(), z()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    full = dec.prefill(xs, torch.empty_like(xs), k1, v1, i32([n + 1]), i32([0]), n + 1)
    dec.prefill(xs[:n].contiguous(), torch.empty((n, H), dtype=F16, device=DEV), k2, v2, i32([n]), i32([0]), n)
    last = dec.forward(xs[n:n + 1].contiguous(), torch.empty((1, H), dtype=F16, device=DEV), k2, v2, n + 1)
    a, b = last.float().cpu().numpy(), full[n:n + 1].float().cpu().numpy()
    assert (np.abs(a - b) <= 2e-2 + 2e-2 * np.abs(b)).all(), np.abs(a - b).max()
    assert (k1.float() - k2.float()).abs().max().item() <= 2e-2
    # chunked prefill: 100 tokens, then 51 more on top of the history == one shot
    k3, v3 = z(), z()
    dec.prefill(xs[:100].contiguous(), torch.empty((100, H), dtype=F16, device=DEV), k3, v3, i32([100]), i32([0]), 100)
    part = dec.prefill(xs[100:].contiguous(), torch.empty((n + 1 - 100, H), dtype=F16, device=DEV), k3, v3, i32([n + 1 - 100]),
                       i32([100]), n + 1 - 100)
    c, d = part.float().cpu().numpy(), full[100:].float().cpu().numpy()
    assert (np.abs(c - d) <= 2e-2 + 2e-2 * np.abs(d)).all(), np.abs(c - d).max()
    dec.close()


def test_fp8_prefill_consistent_with_fp8_decode_and_tracks_fp16(llmie):
    """fp8 engine (e4m3 weights, per-token e4m3 activations): prefill and decode quantise every token row the same way,
    so prefill(n+1)[-1] must agree with prefill(n) -> decode(n+1) up to the chaotic rounding noise of dynamic fp8
    (see test_fp8_decoder_matches_oracle_composition), and the whole prefill stays close to the fp16 engine's."""
    rng = np.random.default_rng(43)
    nh, hs, I, L, max_seq, n = 8, 128, 1536, 2, 256, 140
    H = nh * hs
    layers = _model(rng, nh, nh, hs, I, L)
    d16 = _engine(llmie, layers, nh, nh, hs, I, max_seq, 1)
    eng8 = []
    for w in layers:
        lw = dict(attn_norm=torch.from_numpy(w["attn_norm"]).to(DEV).to(F16), ffn_norm=torch.from_numpy(w["ffn_norm"]).to(DEV).to(F16))
        for k in ("qkv", "o", "gate_up", "down"):
            wd = torch.from_numpy(w[k]).to(DEV).to(F16)
            q = torch.empty(wd.shape, dtype=torch.uint8, device=DEV)
            s = torch.empty(wd.shape[0], dtype=torch.float32, device=DEV)
            llmie.quantize_fp8(wd, q, s)
            lw[k] = dict(data=q, scale=s)
        eng8.append(lw)
    cfg = dict(head_num=nh, kv_head_num=nh, head_size=hs, inter_size=I, num_layers=L, vocab_size=100, max_seq_len=max_seq,
               max_batch=1, rotary_dim=hs, rotary_base=10000.0, rms_eps=1e-5, dtype=llmie.F16, wfmt=llmie.W_FP8, int4_group=128)
    d8 = llmie.Decoder(cfg, eng8)
    xs = torch.from_numpy(_h(rng.standard_normal((n + 1, H)).astype(np.float32))).to(DEV).to(F16)
    z = lambda: torch.zeros((L, 1, nh, max_seq, hs), dtype=F16, device=DEV)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    k1, v1, k2, v2, k3, v3 = z(), z(), z(), z(), z(), z()
    full8 = d8.prefill(xs, torch.empty_like(xs), k1, v1, i32([n + 1]), i32([0]), n + 1).float()
    d8.prefill(xs[:n].contiguous(), torch.empty((n, H), dtype=F16, device=DEV), k2, v2, i32([n]), i32([0]), n)
    last = d8.forward(xs[n:n + 1].contiguous(), torch.empty((1, H), dtype=F16, device=DEV), k2, v2, n + 1).float()
    rel = ((last - full8[n:n + 1]).norm() / full8[n:n + 1].norm()).item()
    print("fp8 prefill vs decode rel %.4f" % rel)
    assert rel < 0.06, rel  # two layers = four quantisation stages of ~1.5-2% rounding chaos each
    # rows of the first n tokens come from the same prefill arithmetic; token n's layer-1 K row carries the layer-0 noise
    assert (k1[:, :, :, :n].float() - k2[:, :, :, :n].float()).abs().max().item() <= 2e-2
    assert (k1.float() - k2.float()).abs().max().item() <= 0.4
    full16 = d16.prefill(xs, torch.empty_like(xs), k3, v3, i32([n + 1]), i32([0]), n + 1).float()
    rel16 = ((full8 - full16).norm() / full16.norm()).item()
    print("fp8 prefill vs fp16 prefill rel %.4f" % rel16)
    assert rel16 < 0.12, rel16  # measured 0.079: two layers x (e4m3 weights + e4m3 activations), 3 mantissa bits each
    d8.close()
    d16.close()


_NORM_QUANT_SCRIPT = r"""
import sys, os, importlib.util, numpy as np, torch
root = sys.argv[1]
spec = importlib.util.spec_from_file_location("llmie_amd", os.path.join(root, "llm-inference-engine_amd", "__init__.py"))
llmie = importlib.util.module_from_spec(spec); sys.modules["llmie_amd"] = llmie; spec.loader.exec_module(llmie)
torch.manual_seed(11)
nh, hs, I, L, max_seq, T = 32, 128, 11008, 2, 1024, 1024
H, QKV = nh * hs, 3 * nh * hs
layers = []
for l in range(L):
    m = {}
    for k, (n, kk) in dict(qkv=(QKV, H), o=(H, H), gate_up=(2 * I, H), down=(H, I)).items():
        w = ((torch.rand((n, kk), device="cuda") * 2 - 1) * 2 / kk ** 0.5).half()
        q = torch.empty((n, kk), dtype=torch.uint8, device="cuda"); s = torch.empty(n, dtype=torch.float32, device="cuda")
        llmie.quantize_fp8(w, q, s)
        m[k] = dict(data=q, scale=s)
        del w
    g1 = (torch.rand(H, device="cuda") * 0.4 + 0.8).half()
    g2 = (torch.rand(H, device="cuda") * 0.4 + 0.8).half()
    layers.append(dict(attn_norm=g1, ffn_norm=g2, **m))
cfg = dict(head_num=nh, kv_head_num=nh, head_size=hs, inter_size=I, num_layers=L, vocab_size=100, max_seq_len=max_seq,
           max_batch=2, rotary_dim=hs, rotary_base=10000.0, rms_eps=1e-5, dtype=llmie.F16, int4_group=128, wfmt=llmie.W_FP8)
dec = llmie.Decoder(cfg, layers)
x = torch.randn((T, H), device="cuda").half()
kc = torch.zeros((L, 2, nh, max_seq, hs), device="cuda", dtype=torch.float16)
vc = torch.zeros_like(kc)
i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
out = dec.prefill(x, torch.empty_like(x), kc, vc, i32([600, 424]), i32([0, 0]), 600)
np.save(sys.argv[2], np.concatenate([out.float().cpu().numpy().ravel(), kc[1, 1, 3, :424].float().cpu().numpy().ravel()]))
"""


def test_fp8_prefill_norm_quant_fusion_is_bit_identical(tmp_path):
    """fp8 prefill: RMSNorm kernels that emit the per-token e4m3 activations directly (rmsnorm_quant_kernel + pre-quantised
    tiled GEMM) against RMSNorm -> quantize_rows -> GEMM (LLMIE_NO_NORM_QUANT=1): hidden states and cache rows bit-equal.
    One process per setting (the switch is read once per process)."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "run.py"
    script.write_text(_NORM_QUANT_SCRIPT)
    outs = []
    for flag in (None, "1"):
        env = dict(os.environ)
        env.pop("LLMIE_NO_NORM_QUANT", None)
        if flag:
            env["LLMIE_NO_NORM_QUANT"] = flag
        dst = tmp_path / ("out_%s.npy" % (flag or "fused"))
        subprocess.run([sys.executable, str(script), root, str(dst)], check=True, env=env, timeout=600)
        outs.append(np.load(dst))
    assert np.isfinite(outs[0]).all() and np.abs(outs[0]).max() > 0
    assert np.array_equal(outs[0], outs[1])
