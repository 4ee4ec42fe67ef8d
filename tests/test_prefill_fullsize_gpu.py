"""The prefill path AT THE BENCH'S OWN SIZES: one Llama-2-7B-geometry layer (H = 4096, I = 11008, 32 heads)
prefilled as 1 x 2048 and as 8 x 512 tokens -- the eight-phase 256 x 256 / 256 x 128 GEMM plans, the two-launch SwiGLU plan and the
flash kernel with 16 query tiles -- against the oracle's composition of the reference kernels (context_decoder.cpp:58-199) on the
same inputs, for fp16 weights and for weight-only int8 / int4 (oracle on the DE-QUANTISED weights; README.md:36-39 plans them,
the reference holds no quantised kernel).  The oracle evaluates 80 sampled token rows of the layer output (oracle.py
context_decoder_rows: K and V of ALL tokens, everything else for the sampled rows -- a whole layer is ~0.8 TFLOP on the host) and
every K / V cache row.  (8 x 512 = 4096 tokens, 1 x 2048 = 2048: the bench's two prefill configurations.)"""
import numpy as np
import pytest
import torch

import oracle as orc
from conftest import systematic_error

pytestmark = pytest.mark.gpu
DEV, F16 = "cuda", torch.float16
NH, HS, I, GROUP = 32, 128, 11008, 128
H, QKV = NH * HS, 3 * NH * HS
# the bounds of tests/test_prefill_gpu.py (small models): element-wise fp16 pipeline tolerance, relative Frobenius error and
# projection of the error on the signal (a 1 % gain error of the layer gives 1e-2 on both)
FRO, PROJ = 3e-3, 2e-4


def _h(a):
    return a.astype(np.float16).astype(np.float32)


def _quant8(w):
    amax = np.abs(w).max(axis=1)
    s = (amax / np.float32(127.0)).astype(np.float16)
    s[s == 0] = np.float16(1.0)
    q = np.clip(np.rint(w / s.astype(np.float32)[:, None]), -127, 127).astype(np.int8)
    return q, s, q.astype(np.float32) * s.astype(np.float32)[:, None]


def _quant4(w, group):
    N, K = w.shape
    wg = w.reshape(N, K // group, group)
    s = (np.abs(wg).max(axis=2) / np.float32(7.0)).astype(np.float16)
    s[s == 0] = np.float16(1.0)
    q = np.clip(np.rint(wg / s.astype(np.float32)[:, :, None]), -8, 7).astype(np.int32)
    deq = (q.astype(np.float32) * s.astype(np.float32)[:, :, None]).reshape(N, K)
    q = q.reshape(N, K) + 8
    return (q[:, 0::2] | (q[:, 1::2] << 4)).astype(np.uint8), s, deq


def seven_b_weights():
    """the module's seeded layer (Llama-2-7B geometry) and 4096 input rows, fp16-representable fp32"""
    rng = np.random.default_rng(77)
    u = lambda n, k: _h(rng.uniform(-1, 1, (n, k)).astype(np.float32) * 2 / np.sqrt(k))
    return dict(qkv=u(QKV, H), o=u(H, H), gate_up=u(2 * I, H), down=u(H, I),
                attn_norm=_h(rng.uniform(0.8, 1.2, H).astype(np.float32)), ffn_norm=_h(rng.uniform(0.8, 1.2, H).astype(np.float32)),
                x=_h(rng.standard_normal((4096, H)).astype(np.float32)))


@pytest.fixture(scope="module")
def weights():
    return seven_b_weights()


_QUANTISED = {}   # (id of the weights dict, fmt, matrix) -> (codes, scales, de-quantised): each format is quantised once per process


def _quantised(W, fmt, name):
    key = (id(W), fmt, name)
    if key not in _QUANTISED:
        _QUANTISED[key] = _quant8(W[name]) if fmt == "int8" else _quant4(W[name], GROUP)
    return _QUANTISED[key]


def engine_layer(W, fmt):
    """(engine layer on the device, oracle layer: de-quantised weights for int8 / int4)"""
    d = lambda a: torch.from_numpy(a).to(DEV)
    eng, ol = dict(attn_norm=d(W["attn_norm"]).to(F16), ffn_norm=d(W["ffn_norm"]).to(F16)), \
        dict(attn_norm=W["attn_norm"], ffn_norm=W["ffn_norm"], qkv_bias=None, o_bias=None)
    for name in ("qkv", "o", "gate_up", "down"):
        if fmt == "f16":
            eng[name], ol[name] = dict(data=d(W[name]).to(F16)), W[name]
        else:
            q, s, deq = _quantised(W, fmt, name)
            eng[name], ol[name] = dict(data=d(q), scale=d(s)), deq
    return eng, ol


def engine_cfg(llmie, fmt, max_seq, max_batch):
    return dict(head_num=NH, kv_head_num=NH, head_size=HS, inter_size=I, num_layers=1, vocab_size=100, max_seq_len=max_seq,
                max_batch=max_batch, rotary_dim=HS, rotary_base=10000.0, rms_eps=1e-5, dtype=llmie.F16,
                wfmt=dict(f16=llmie.W_F16, int8=llmie.W_INT8, int4=llmie.W_INT4)[fmt], int4_group=GROUP)


OCFG = dict(head_num=NH, kv_head_num=NH, head_size=HS, inter_size=I, rms_eps=1e-5, rotary_dim=HS, rotary_base=10000.0)


@pytest.mark.parametrize("fmt", ["f16", "int8", "int4"])
def test_one_7b_layer_prefill_at_bench_sizes_matches_oracle(llmie, weights, fmt):
    W = weights
    d = lambda a: torch.from_numpy(a).to(DEV)
    eng, ol = engine_layer(W, fmt)
    max_seq = 2048
    dec = llmie.Decoder(engine_cfg(llmie, fmt, max_seq, 8), [eng])
    ocfg = OCFG
    rng = np.random.default_rng(78)
    kv_proj = []   # the oracle's K / V projection of the 4096 rows (the 1 x 2048 case uses its first 2048: the projection is row-wise)
    for lens in ([512] * 8, [2048]):
        bs, T = len(lens), sum(lens)
        hist = [0] * bs
        x = W["x"][:T]
        xd = d(x).to(F16)
        kd = torch.zeros((1, bs, NH, max_seq, HS), dtype=F16, device=DEV)
        vd = torch.zeros_like(kd)
        out = torch.empty_like(xd)
        dec.prefill(xd, out, kd, vd, torch.tensor(lens, dtype=torch.int32, device=DEV), torch.tensor(hist, dtype=torch.int32, device=DEV),
                    max(lens))
        # sampled rows: the edges of the 256-row GEMM tiles and of the 128-row query tiles, sequence starts / ends, random others
        fixed = [0, 1, 15, 16, 127, 128, 255, 256, 511, 512, 1023, 1024, 1791, 1792, 2046, 2047, T - 2, T - 1]
        rows = np.array(sorted(set(fixed) | set(rng.choice(T, 64, replace=False).tolist())))
        kc = np.zeros((1, bs, NH, max_seq, HS), np.float32)
        vc = np.zeros_like(kc)
        exp = orc.context_decoder_rows(ocfg, ol, x, kc, vc, lens, hist, rows, kv_proj=kv_proj[0][:T] if kv_proj else kv_proj)
        got = out.float().cpu().numpy()[rows]
        err = np.abs(got - exp)
        fro, proj = systematic_error(got, exp)
        kerr = np.abs(kd.float().cpu().numpy() - kc).max()
        verr = np.abs(vd.float().cpu().numpy() - vc).max()
        print("%s %dx%d: max err %.4g (|exp| max %.3g), rel Frobenius %.3g, projection %.3g, K cache %.3g, V cache %.3g"
              % (fmt, bs, lens[0], err.max(), np.abs(exp).max(), fro, proj, kerr, verr))
        assert (err <= 3e-2 + 3e-2 * np.abs(exp)).all(), "max err %g (|exp| max %g)" % (err.max(), np.abs(exp).max())
        assert fro <= FRO and proj <= PROJ, "relative Frobenius error %.3g, projection on the signal %.3g" % (fro, proj)
        # every K / V row of every token: the QKV GEMM's K / V columns + RoPE + append at full size (fp16 rounding of O(1) values)
        assert kerr <= 2e-2 and verr <= 2e-2
    dec.close()


# Token counts of the single-sequence sweep: the edges of every route the four projections take below the full 256-row grid
# (GEMV <= 8, the split-K forms at 33 / 65 rows, the slab-fused short path <= 128, two split-K passes 129..192, 128-row passes and
# partly filled 256-row grids 193..768, the full grid from 769).
SWEEP_T = [1, 8, 9, 33, 64, 65, 128, 129, 192, 193, 256, 257, 384, 385, 512, 513, 768, 769]
SWEEP_MAX_SEQ = 1024


def _close(got, exp, label):
    err = np.abs(got - exp)
    fro, proj = systematic_error(got, exp)
    assert (err <= 3e-2 + 3e-2 * np.abs(exp)).all(), "%s: max err %g (|exp| max %g)" % (label, err.max(), np.abs(exp).max())
    assert fro <= FRO and proj <= PROJ, "%s: relative Frobenius error %.3g, projection on the signal %.3g" % (label, fro, proj)
    return fro, proj


@pytest.mark.parametrize("fmt", ["f16", "int8", "int4"])
def test_7b_layer_prefill_sweep_over_short_and_mid_token_counts(llmie, weights, fmt):
    """One 7B-geometry layer (no biases: the lean in-place sequence) prefilled as ONE sequence of T tokens for every T in SWEEP_T
    against a single oracle run on the first 769 rows: a causal prefill without history is a prefix computation (row r depends on
    rows <= r only), so the oracle's rows < T are the expected rows of the T-token prefill, and its K / V cache rows < T the
    expected cache rows.  Sampled rows include T - 1 of every T.  Forms by T, read off the dispatch predicates and time models
    (the kernels behind each form: tests/test_linear_routes_gpu.py):
      fp16  <= 128 slab-fused short path; 129..192 split-K (two passes) with fused SwiGLU;
            QKV: partly filled 256-row grid 193..256, full grid with the RoPE epilogue from 257;
            O: 128-row split-K passes 193..384, partly filled grid 385..768, full grid 769;
            down: passes 193..512, partly filled grid 513..768; gate/up: two launches 193..512, fused SwiGLU from 513
      int8  <= 128 short path; 129..191 split-K; O / down: int8 split-K passes 192..256, fp16 image 257..768, int8 tiles 769
      int4  <= 64 short path; 65..191 group-128 split-K; fp16 image from 192"""
    W = weights
    eng, ol = engine_layer(W, fmt)
    dec = llmie.Decoder(engine_cfg(llmie, fmt, SWEEP_MAX_SEQ, 1), [eng])
    Tmax = max(SWEEP_T)
    x = W["x"][:Tmax]
    rng = np.random.default_rng(79)
    fixed = [0, 1, 15, 16, 127, 128, 255, 256] + [T - 1 for T in SWEEP_T]
    rows = np.array(sorted(set(fixed) | set(rng.choice(Tmax, 40, replace=False).tolist())))
    kc = np.zeros((1, 1, NH, SWEEP_MAX_SEQ, HS), np.float32)
    vc = np.zeros_like(kc)
    exp = orc.context_decoder_rows(OCFG, ol, x, kc, vc, [Tmax], [0], rows)
    xd = torch.from_numpy(x).to(DEV).to(F16)
    one, zero = torch.ones(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    for T in SWEEP_T:
        kd = torch.zeros((1, 1, NH, SWEEP_MAX_SEQ, HS), dtype=F16, device=DEV)
        vd = torch.zeros_like(kd)
        out = torch.empty((T, H), dtype=F16, device=DEV)
        dec.prefill(xd[:T], out, kd, vd, one * T, zero, T)
        sel = rows < T
        got = out.float().cpu().numpy()[rows[sel]]
        fro, proj = _close(got, exp[sel], "%s T=%d" % (fmt, T))
        kerr = np.abs(kd.float().cpu().numpy()[:, :, :, :T] - kc[:, :, :, :T]).max()
        verr = np.abs(vd.float().cpu().numpy()[:, :, :, :T] - vc[:, :, :, :T]).max()
        print("%s T=%d: rel Frobenius %.3g, projection %.3g, K cache %.3g, V cache %.3g" % (fmt, T, fro, proj, kerr, verr))
        assert kerr <= 2e-2 and verr <= 2e-2, "%s T=%d: K cache %g, V cache %g" % (fmt, T, kerr, verr)
    dec.close()


# BASELINE configs[1] (prefill_f16_b1_s128): one 128-token sequence, and a ragged 128-token batch behind cached history
CONFIG1 = [("single_128", [128], [0]), ("ragged_hist", [70, 40, 18], [0, 33, 5])]


def config1_run(llmie, W, fmt):
    """llmie_decoder_prefill of the CONFIG1 cases (+ one decode step at position 129 after the single sequence) on the module's
    layer; returns the outputs and caches as numpy.  Also run by tests/short_prefill_probe.py in a child process."""
    eng, ol = engine_layer(W, fmt)
    dec = llmie.Decoder(engine_cfg(llmie, fmt, SWEEP_MAX_SEQ, 3), [eng])
    res = {}
    for name, lens, hist in CONFIG1:
        x, kc, vc = config1_inputs(W, lens)
        kd, vd = torch.from_numpy(kc).to(DEV).to(F16), torch.from_numpy(vc).to(DEV).to(F16)
        xd = torch.from_numpy(x).to(DEV).to(F16)
        out = torch.empty_like(xd)
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
        dec.prefill(xd, out, kd, vd, i32(lens), i32(hist), max(lens))
        res[name] = out.float().cpu().numpy()
        res[name + "_k"], res[name + "_v"] = kd.float().cpu().numpy(), vd.float().cpu().numpy()
        if name == "single_128":
            xs = torch.from_numpy(W["x"][128:129]).to(DEV).to(F16)
            res["decode_129"] = dec.forward(xs, torch.empty_like(xs), kd, vd, 129).float().cpu().numpy()
            res["decode_129_k"] = kd.float().cpu().numpy()
    dec.close()
    return res


def config1_inputs(W, lens):
    """token rows and caches (random history rows, as the oracle's pre-filled cache) of a CONFIG1 case"""
    rng = np.random.default_rng(80 + len(lens))
    shape = (1, len(lens), NH, SWEEP_MAX_SEQ, HS)
    kc = _h(rng.standard_normal(shape).astype(np.float32) * 0.5)
    vc = _h(rng.standard_normal(shape).astype(np.float32) * 0.5)
    return W["x"][:sum(lens)], kc, vc


def _check_config1(W, fmt, res, label):
    ol = dict(attn_norm=W["attn_norm"], ffn_norm=W["ffn_norm"], qkv_bias=None, o_bias=None)
    for m in ("qkv", "o", "gate_up", "down"):
        ol[m] = W[m] if fmt == "f16" else _quantised(W, fmt, m)[2]
    for name, lens, hist in CONFIG1:
        x, kc, vc = config1_inputs(W, lens)
        T = sum(lens)
        exp = orc.context_decoder_rows(OCFG, ol, x, kc, vc, lens, hist, np.arange(T))
        _close(res[name], exp, "%s %s %s" % (label, fmt, name))
        assert np.abs(res[name + "_k"] - kc).max() <= 2e-2 and np.abs(res[name + "_v"] - vc).max() <= 2e-2, (label, fmt, name)
        if name == "single_128":
            # one decode step on the prefilled caches: the decoder test's bounds (tests/test_decoder_gpu.py)
            dcfg = dict(OCFG, num_layers=1, vocab=100, max_seq_len=SWEEP_MAX_SEQ)
            e = orc.self_decoder(dcfg, [ol], W["x"][128:129], kc, vc, 129)
            got = res["decode_129"]
            err = np.abs(got - e)
            assert (err <= 2e-2 + 2e-2 * np.abs(e)).all(), "%s %s decode: max err %g" % (label, fmt, err.max())
            fro, proj = systematic_error(got, e)
            assert fro <= FRO and proj <= PROJ, "%s %s decode: fro %.3g proj %.3g" % (label, fmt, fro, proj)
            assert np.abs(res["decode_129_k"] - kc).max() <= 2e-2


@pytest.mark.parametrize("fmt", ["f16", "int8", "int4"])
def test_7b_layer_config1_prefill_both_short_sequences(llmie, weights, fmt, tmp_path):
    """BASELINE configs[1] at 7B geometry against the oracle: [128] and ragged [70, 40, 18] behind histories [0, 33, 5], then one
    decode step at position 129 -- once on the default launch sequence (fp16 / int8: the slab-fused short path) and once, in a
    fresh process, with LLMIE_NO_FUSED_SHORT_PREFILL=1 (the prefill-sized sequence; the switch is read once per process)"""
    import os
    import subprocess
    import sys
    _check_config1(weights, fmt, config1_run(llmie, weights, fmt), "default")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / ("unfused_%s.npz" % fmt))
    env = dict(os.environ, LLMIE_NO_FUSED_SHORT_PREFILL="1")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "short_prefill_probe.py"), out, fmt], capture_output=True, text=True,
                       timeout=600, cwd=root, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    _check_config1(weights, fmt, dict(np.load(out)), "LLMIE_NO_FUSED_SHORT_PREFILL")
