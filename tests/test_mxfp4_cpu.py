"""MXFP4 weights without a GPU: the exports and their signatures, every host-side refusal with its code and message, the workspace
query, the planned route of every row-count range, the engine's plans for an MXFP4 config, the conditions that make the exact cases of
tests/mxfp4_cases.py exact, and the properties of the restated quantiser the GPU tests compare the device against."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mxfp4_cases as MX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def lib(llmie):
    llmie.build()
    return llmie.lib()


def _err(lib):
    return lib.llmie_last_error().decode()


P = C.c_void_p(4096)          # stand-in addresses: the refusals come before anything is dereferenced
ODD = C.c_void_p(4096 + 8)


def test_exports_and_signatures(lib, llmie):
    assert llmie.W_MXFP4 == 5
    hdr = open(os.path.join(ROOT, "include", "llmie.h")).read()
    assert "LLMIE_W_MXFP4 = 5" in hdr and "#define LLMIE_ABI_VERSION 3" in hdr
    _vp, _i, _sz = C.c_void_p, C.c_int, C.c_size_t
    want = {"llmie_quantize_mxfp4": [_vp, _vp, _vp, _i, _i, _vp], "llmie_dequantize_mxfp4": [_vp, _vp, _vp, _i, _i, _vp],
            "llmie_linear_mxfp4": [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]}
    for name, sig in want.items():
        assert name in llmie.EXPORTS
        fn = getattr(lib, name)
        assert list(fn.argtypes) == sig and fn.restype is C.c_int
    for name in ("quantize_mxfp4", "dequantize_mxfp4", "linear_mxfp4"):
        assert callable(getattr(llmie, name))


def test_refusals(lib):
    # quantiser
    assert lib.llmie_quantize_mxfp4(None, P, P, 4, 64, None) == INVALID and "quantize_mxfp4: NULL pointer" in _err(lib)
    assert lib.llmie_quantize_mxfp4(P, P, None, 4, 64, None) == INVALID
    assert lib.llmie_quantize_mxfp4(P, P, P, 0, 64, None) == INVALID and "bad shape" in _err(lib)
    assert lib.llmie_quantize_mxfp4(P, P, P, 4, -32, None) == INVALID
    assert lib.llmie_quantize_mxfp4(P, P, P, 4, 48, None) == UNSUPPORTED and "K % 32 == 0 (K=48)" in _err(lib)
    assert lib.llmie_quantize_mxfp4(ODD, P, P, 4, 64, None) == UNSUPPORTED and "16-byte aligned w" in _err(lib)
    # de-quantiser
    assert lib.llmie_dequantize_mxfp4(P, None, P, 4, 64, None) == INVALID and "dequantize_mxfp4: NULL pointer" in _err(lib)
    assert lib.llmie_dequantize_mxfp4(P, P, P, 4, 0, None) == INVALID
    assert lib.llmie_dequantize_mxfp4(P, P, P, 4, 40, None) == UNSUPPORTED and "K % 32 == 0 (K=40)" in _err(lib)
    assert lib.llmie_dequantize_mxfp4(P, P, ODD, 4, 64, None) == UNSUPPORTED and "16-byte aligned" in _err(lib)
    # projection
    lin = lambda x=P, wq=P, sc=P, y=P, M=4, K=64, N=16, ws=None, wsb=0: lib.llmie_linear_mxfp4(x, wq, sc, y, M, K, N, None, None, ws, wsb, None)
    assert lin(x=None) == INVALID and "linear_mxfp4: NULL pointer" in _err(lib)
    assert lin(sc=None) == INVALID
    assert lin(M=0) == INVALID and "bad shape M=0" in _err(lib)
    assert lin(ws=ODD, wsb=1 << 20) == INVALID and "workspace must be 16-byte aligned" in _err(lib)
    for kw in (dict(K=48), dict(K=96 + 16), dict(x=ODD), dict(wq=ODD)):
        assert lin(**kw) == UNSUPPORTED, kw
        assert "linear_mxfp4: needs K % 32 == 0 and 16-byte aligned x and wq" in _err(lib)
    # the route query refuses what the entry refuses, and the fused forms the format does not have
    route = lambda **kw: lib.llmie_linear_route(5, kw.get("x", P), kw.get("w", P), kw.get("scale", P), P, kw.get("M", 4), kw.get("K", 64), 16,
                                                kw.get("swiglu", 0), 0, None, None, None, 0)
    assert route(K=48) is None and "K % 32 == 0" in _err(lib)
    assert route(x=ODD) is None
    assert route(scale=None) is None and "NULL pointer" in _err(lib)
    assert route(swiglu=1) is None and "no fused norm or SwiGLU form" in _err(lib)
    assert route(scale=C.c_void_p(4097)) == b"mxfp4_gemv"          # scale rows carry no alignment beyond one byte


@pytest.mark.parametrize("K,N", [(4096, 256), (96, 17), (11040, 1003)])
def test_workspace_query_and_routes(lib, K, N):
    """M <= 8 GEMV, <= 64 MFMA, < 192 row chunks, from 192 the fp16 image where the workspace holds it -- else row chunks"""
    image = (N * K * 2 + 255) // 256 * 256
    names = {1: b"mxfp4_gemv", 8: b"mxfp4_gemv", 9: b"mxfp4_mfma", 64: b"mxfp4_mfma", 65: b"mxfp4_chunks", 191: b"mxfp4_chunks"}
    route = lambda M, ws, wsb: lib.llmie_linear_route(5, P, P, P, P, M, K, N, 0, 0, None, None, ws, wsb)
    for M, name in names.items():
        assert lib.llmie_linear_workspace_bytes(5, M, K, N) == 0
        assert route(M, None, 0) == name and route(M, P, 1 << 30) == name
    for M in (192, 300):
        assert lib.llmie_linear_workspace_bytes(5, M, K, N) == image
        with_ws = route(M, P, image)
        assert with_ws.startswith(b"image_prefill+"), with_ws
        assert route(M, None, 0) == b"mxfp4_chunks"
        assert route(M, P, image - 1) == b"mxfp4_chunks"               # short by one byte: no room for the image
    assert lib.llmie_linear_workspace_bytes(5, 192, 48, N) == 0          # K % 32 != 0: nothing to size
    assert lib.llmie_linear_workspace_bytes(5, 0, K, N) == 0


def _cfg(llmie, **kw):
    c = dict(head_num=8, kv_head_num=8, head_size=128, inter_size=2816, num_layers=2, vocab_size=100, max_seq_len=384, max_batch=80,
             rotary_dim=128, rotary_base=10000.0, rms_eps=1e-5, dtype=llmie.F16, wfmt=llmie.W_MXFP4, int4_group=0)
    c.update(kw)
    return c


def test_engine_plans(lib, llmie):
    kv8 = dict(kv_fmt=llmie.KV_FP8, k_scale=1 / 32, v_scale=1 / 16)
    for cfg in (_cfg(llmie), _cfg(llmie, kv_head_num=2), _cfg(llmie, **kv8), _cfg(llmie, flags=llmie.DEC_NO_PACKED_COPY)):
        for rows in (1, 2, 8, 9, 32, 64, 65, 80):
            for flags in (0, llmie.PLAN_PAGED, llmie.PLAN_RAGGED, llmie.PLAN_PAGED | llmie.PLAN_RAGGED):
                assert llmie.decoder_plan_name(cfg, False, rows, call_flags=flags) == "unfused", (rows, flags, _err(lib))
        for tokens in (1, 64, 128, 191, 192, 300, 2048):
            assert llmie.decoder_plan_name(cfg, True, tokens) == "general"
            text, status = llmie.decoder_prefill_layer_plan(cfg, tokens, batch=-(-tokens // 256), max_q_len=min(tokens, 256))
            assert status == 0, _err(lib)
            f = text.split()
            assert f[0] == "general" and "token_table=0" in f and "attn_norm=inplace" in f and "ffn_norm=inplace" in f
            assert "qkv=plain" in f and "pre=none" in f and "rope_done=0" in f and "rope_append=1" in f and "gate_up=two_launch" in f
            assert "qkv_gemm=1" in f and "gate_up_swiglu=2" in f
            assert ("kv=e4m3" in f) == ("kv_fmt" in cfg and cfg["kv_fmt"] == llmie.KV_FP8)
    # a hidden_out off a 16-byte boundary
    assert llmie.decoder_plan_name(_cfg(llmie), False, 4, call_flags=llmie.PLAN_HIDDEN_MISALIGNED) is None
    assert "MXFP4 weights need a 16-byte aligned hidden_out" in _err(lib)
    # no packed image is built
    po = _cfg(llmie, max_batch=16, flags=llmie.DEC_PACKED_ONLY)
    assert llmie.decoder_plan_name(po, False, 4) is None and "LLMIE_DEC_PACKED_ONLY is not available for MXFP4" in _err(lib)
    text, status = llmie.decoder_prefill_layer_plan(po, 64)
    assert text is None and status == UNSUPPORTED and "no packed image is built" in _err(lib)
    # adapters
    assert llmie.decoder_plan_name(_cfg(llmie), False, 4, call_flags=llmie.PLAN_LORA) is None and "adapters need" in _err(lib)
    assert llmie.decoder_plan_name(_cfg(llmie), True, 64, call_flags=llmie.PLAN_LORA) is None and "adapters need" in _err(lib)
    # blocks of 32 along K of every projection
    assert llmie.decoder_plan_name(_cfg(llmie, inter_size=2800), False, 4) is None
    # an attention geometry without the fused kernel: dense only
    odd = _cfg(llmie, head_num=6, kv_head_num=2, head_size=128)    # ratio 3
    assert llmie.decoder_plan_name(odd, False, 4) == "unfused"
    assert llmie.decoder_plan_name(odd, False, 4, call_flags=llmie.PLAN_PAGED) is None


def test_engine_sizes(lib, llmie):
    cfg = _cfg(llmie)
    H, QKV, I = 1024, 3072, 2816
    per_layer = sum(n * k // 2 + n * k // 32 for n, k in ((QKV, H), (H, H), (2 * I, H), (H, I)))
    assert llmie.decoder_resident_weight_bytes(cfg) == 2 * per_layer
    c = llmie.DecoderConfig(**cfg)
    assert lib.llmie_decoder_workspace_bytes(C.byref(c)) > 0
    # the prefill workspace holds the fp16 image of the largest matrix
    i4 = llmie.DecoderConfig(**dict(cfg, wfmt=llmie.W_INT4, int4_group=128))
    f16 = llmie.DecoderConfig(**dict(cfg, wfmt=llmie.W_F16))
    mx, ref, plain = (lib.llmie_decoder_prefill_workspace_bytes(C.byref(x), 300, 2) for x in (c, i4, f16))
    assert mx >= plain + 2 * I * H * 2 and mx <= ref


ALL = MX.CASES + MX.PROBES


@pytest.mark.parametrize("case", ALL, ids=[c["id"] for c in ALL])
def test_case_conditions_and_route(lib, case):
    for epi in MX.epilogues(case):
        MX.build(case, epi)          # asserts conditions()
    M, K, N = case["M"], case["K"], case["N"]
    need = lib.llmie_linear_workspace_bytes(5, M, K, N) if case["ws"] == "auto" else 0
    got = lib.llmie_linear_route(5, P, P, P, P, M, K, N, 0, 0, None, None, P if need else None, need)
    assert got is not None and got.decode() == case["route"]


def test_the_exact_cases_cover_what_the_issue_lists():
    shapes = {(c["M"], c["K"], c["N"]) for c in MX.CASES}
    for M in (1, 3, 8):
        for K in (32, 96, 4128):
            for N in (1, 17, 1003):
                assert (M, K, N) in shapes
    for M in (9, 16, 17, 64):
        for K in (32, 64, 2080):
            for N in (16, 17, 1000):
                assert (M, K, N) in shapes
    assert {(65, 4096, 48), (130, 4096, 48), (192, 4096, 256), (300, 4096, 256)} <= shapes
    assert {c["M"] for c in MX.CASES if c["ws"] is None and c["route"] == "mxfp4_chunks"} == {192, 300}
    routes = {c["route"] for c in MX.CASES}
    assert {"mxfp4_gemv", "mxfp4_mfma", "mxfp4_chunks"} <= routes and any(r.startswith("image_prefill+") for r in routes)
    # probes sit at both ends of the pinned exponent range
    assert {p["ebase"] for p in MX.PROBES} == {MX.E_MIN, MX.E_MAX - 3, -2}
    b = MX.build(next(p for p in MX.PROBES if p["ebase"] == MX.E_MIN), "plain")
    assert b["e"].min() == -23
    b = MX.build(next(p for p in MX.PROBES if p["ebase"] == MX.E_MAX - 3), "plain")
    assert b["e"].max() == 13


# ---------------------------------------------------------------- the restated quantiser
def _q1(values, pad=0.0):
    """quantise one block holding `values` (padded); returns (codes of the values, exponent)"""
    w = np.full((1, 32), pad, np.float16)
    w[0, :len(values)] = values
    wq, sc = MX.quantize(w)
    return MX.unpack(wq)[0, :len(values)], int(sc[0, 0]) - 127


def test_quantiser_tie_table_and_saturation():
    # under amax = 4 (e = 0): ties go to the even code
    codes, e = _q1([4.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5])
    assert e == 0 and codes.tolist() == [6, 0, 2, 2, 4, 4, 6]                  # 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4
    codes, e = _q1([5.0, -5.0, 5.5, 4.5])
    assert e == 0 and codes.tolist() == [6, 14, 7, 6]                          # 5 -> 4, the sign kept
    codes, e = _q1([7.0, 6.5, 7.9, -7.5, 6.0])
    assert e == 0 and codes.tolist() == [7, 7, 7, 15, 7]                       # (6, 8) saturates at 6
    # scaled by a power of two, the same codes
    for s in (-9, 5):
        codes, e = _q1(np.array([4.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5]) * 2.0 ** s)
        assert e == s and codes.tolist() == [6, 0, 2, 2, 4, 4, 6]


def test_quantiser_edges():
    codes, e = _q1([2.0 ** -24])                        # the clamp: e = -26 by the OCP rule
    assert e == -23 and codes.tolist() == [1]           # 0.5 * 2^-23: lossless
    codes, e = _q1([65504.0, 49152.0, 40960.0])
    assert e == 13 and codes.tolist() == [7, 7, 6]      # amax = 65504 -> e = 13; 40960 = 5 * 2^13 -> 4
    codes, e = _q1([0.0, -0.0])
    assert e == 0 and codes.tolist() == [0, 8]          # byte 127, the sign of a zero kept
    codes, e = _q1([1.0, -2.0 ** -20])
    assert e == -2 and codes.tolist() == [6, 8]         # a zero RESULT keeps the sign bit of w
    w = np.ones((1, 64), np.float16)
    w[0, 3], w[0, 40] = np.inf, np.nan
    assert MX.quantize(w)[1].tolist() == [[0xFF, 0xFF]]
    assert (MX.dequantize_f16(*MX.quantize(w)).view(np.uint16) == 0x7E00).all()


def test_quantiser_is_idempotent_and_lossless_on_the_subnormal_grid():
    for N, K in ((1, 32), (37, 96), (5, 11040)):
        w, special = MX.quantiser_inputs(N, K)
        wq, sc = MX.quantize(w)
        assert np.array_equal(sc == 0xFF, special)
        fine = ~np.repeat(special, 32, axis=1)
        back = np.where(fine, MX.dequantize_f16(wq, sc), np.float16(0))
        wq2, sc2 = MX.quantize(back)
        keep = ~np.repeat(special, 16, axis=1)
        assert np.array_equal(wq2[keep], wq[keep]) and np.array_equal(sc2[~special], sc[~special])
        # every scale the quantiser emits lies in the pinned range
        assert sc[~special].min() >= 127 + MX.E_MIN and sc[~special].max() <= 127 + MX.E_MAX
    sub = (np.arange(32, dtype=np.uint16) % 7).reshape(1, 32).view(np.float16)    # 0 .. 6 units of 2^-24: codes exist for all but 5
    sub = sub.copy()
    sub.view(np.uint16)[sub.view(np.uint16) == 5] = 4
    assert np.array_equal(MX.dequantize_f16(*MX.quantize(sub)).view(np.uint16), sub.view(np.uint16))


def test_magnitude_identity():
    """a code's magnitude is the fp16 whose bits are (code & 7) << 9, times 2^14: what the kernels' expansion relies on"""
    for code in range(8):
        h = np.array([code << 9], np.uint16).view(np.float16)[0]
        assert float(h) * 2.0 ** 14 == MX.MAG[code]


def test_cpp_driver_compiles(llmie):
    llmie.build()
    d = os.path.join(ROOT, "llm-inference-engine_amd", "cpp_tests")
    subprocess.check_call(["make", "-C", d, "test_mxfp4_api"], stdout=subprocess.DEVNULL)
    assert os.path.exists(os.path.join(d, "test_mxfp4_api"))
