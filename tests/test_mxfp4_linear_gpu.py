"""MXFP4 weights on the GPU: the quantiser and the de-quantiser against the numpy restatement of tests/mxfp4_cases.py, bit for bit, and
llmie_linear_mxfp4 on every route (mxfp4_gemv, mxfp4_mfma, mxfp4_chunks, the fp16 image) against the exactly known answers of that
module: no differing bit is allowed (+0 and -0 are the only two patterns taken for one another: the sign of an exact zero sum is the
summation order's to decide).  Each case asserts the planned route's name first.  Random data is held to the int4 tests' bound
against a float64 product over the de-quantised weights (the weights carry no extra rounding here, so the bound is inherited)."""
import ctypes as C

import numpy as np
import pytest
import torch

import mxfp4_cases as MX

pytestmark = pytest.mark.gpu
DEV, F16 = "cuda", torch.float16


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _u16(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def _assert_bits(got, expected, what, fold_zero=True):
    g, e = _u16(got), np.ascontiguousarray(expected).view(np.uint16).copy()
    if fold_zero:
        g[g == 0x8000] = 0
        e[e == 0x8000] = 0
    bad = g != e
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d elements differ; first at %s: got 0x%04x, exact 0x%04x" % (what, bad.sum(), bad.size, i, g[i], e[i]))


def _route(llmie, x, wq, scale, y, ws):
    M, K, N = x.shape[0], x.shape[1], wq.shape[0]
    if isinstance(ws, str):
        need = llmie.linear_workspace_bytes(llmie.W_MXFP4, M, K, N)
        ws = torch.empty(need, dtype=torch.uint8, device=DEV) if need else None
    return llmie.linear_route(llmie.W_MXFP4, x.data_ptr(), wq.data_ptr(), scale.data_ptr(), y.data_ptr(), M, K, N,
                              workspace=ws.data_ptr() if ws is not None else None, workspace_bytes=ws.numel() if ws is not None else 0)


def _run(llmie, case, x, wq, scale, y, **kw):
    """a device error ends the session: nothing more is launched on a GPU that has faulted.  A refusal on the host (LlmieError that is
    no failed launch) fails this test alone"""
    try:
        llmie.linear_mxfp4(x, wq, scale, y, workspace=case["ws"], **kw)
        torch.cuda.synchronize()
    except llmie.LlmieError as e:
        if "launch failed" not in str(e):
            raise
        pytest.exit("%s: %s" % (case["id"], e), returncode=3)
    except RuntimeError as e:          # torch: the synchronise reports the device's error
        pytest.exit("%s: %s" % (case["id"], e), returncode=3)
    return y


# ---------------------------------------------------------------- quantiser / de-quantiser
@pytest.mark.parametrize("N,K", [(1, 32), (37, 96), (5, 11040)])
def test_quantiser_matches_the_restatement(llmie, N, K):
    w, special = MX.quantiser_inputs(N, K)
    eq, es = MX.quantize(w)
    wq = torch.full((N, K // 2), 0xEE, dtype=torch.uint8, device=DEV)
    sc = torch.full((N, K // 32), 0xEE, dtype=torch.uint8, device=DEV)
    llmie.quantize_mxfp4(_dev(w), wq, sc)
    torch.cuda.synchronize()
    gs, gq = sc.cpu().numpy(), wq.cpu().numpy()
    assert np.array_equal(gs, es), "scale bytes differ at %s" % (np.argwhere(gs != es)[:4].tolist(),)
    keep = ~np.repeat(special, 16, axis=1)          # a block with inf / NaN: the scale byte 0xFF only, its codes are unspecified
    assert np.array_equal(gq[keep], eq[keep]), "%d code bytes differ" % (gq[keep] != eq[keep]).sum()
    if N * K >= 3 * 32:
        assert special.sum() == 2 and (gs[special] == 0xFF).all()


def test_quantiser_then_dequantiser_then_quantiser_is_the_identity(llmie):
    w, special = MX.quantiser_inputs(37, 96, seed=3)
    w = np.where(np.repeat(special, 32, axis=1), np.float16(1), w)
    N, K = w.shape
    wq, sc = torch.empty((N, K // 2), dtype=torch.uint8, device=DEV), torch.empty((N, K // 32), dtype=torch.uint8, device=DEV)
    llmie.quantize_mxfp4(_dev(w), wq, sc)
    w16 = llmie.dequantize_mxfp4(wq, sc, torch.empty((N, K), dtype=F16, device=DEV))
    wq2, sc2 = torch.empty_like(wq), torch.empty_like(sc)
    llmie.quantize_mxfp4(w16, wq2, sc2)
    torch.cuda.synchronize()
    assert torch.equal(wq, wq2) and torch.equal(sc, sc2)


def test_dequantiser_every_code_under_every_pinned_scale(llmie):
    """all 16 codes under every scale byte 104 .. 140, bit-exact (-0 stays -0); bytes 0, 100, 141, 254 against numpy's float64 ->
    float16 cast; 0xFF gives 0x7E00"""
    bytes_ = list(range(104, 141)) + [0, 100, 141, 254, 255]
    N, K = len(bytes_), 64
    codes = np.tile(np.arange(16, dtype=np.uint8), (N, K // 16))
    codes[:, 32:] = codes[:, 32:][:, ::-1]
    scale = np.repeat(np.array(bytes_, np.uint8)[:, None], 2, axis=1)
    scale[:37, 1] = np.roll(scale[:37, 0], 5)        # two different blocks per row
    wq = MX.pack(codes)
    exp = MX.dequantize_f16(wq, scale)
    pinned = np.repeat((scale >= 104) & (scale <= 140), 32, axis=1)
    assert np.array_equal(exp.astype(np.float64)[pinned], MX.dequantize(wq, scale)[pinned])    # exact in the pinned range
    got = llmie.dequantize_mxfp4(_dev(wq), _dev(scale), torch.full((N, K), float("nan"), dtype=F16, device=DEV))
    torch.cuda.synchronize()
    _assert_bits(got, exp, "dequantize_mxfp4", fold_zero=False)
    assert (_u16(got)[-1] == 0x7E00).all()


# ---------------------------------------------------------------- exact cases, every route
ALL = MX.CASES + MX.PROBES


@pytest.mark.parametrize("case", ALL, ids=[c["id"] for c in ALL])
def test_route_is_bit_exact(llmie, case):
    for epi in MX.epilogues(case):
        b = MX.build(case, epi, check=False)      # (the conditions are asserted for these very cases by test_mxfp4_cpu.py)
        x, wq, sc, bias = _dev(b["x"]), _dev(b["w"]), _dev(b["scale"]), _dev(b["bias"])
        fresh = lambda: torch.full((case["M"], case["N"]), float("nan"), dtype=F16, device=DEV)
        assert _route(llmie, x, wq, sc, fresh(), case["ws"]) == case["route"]
        if epi == "plain":
            _assert_bits(_run(llmie, case, x, wq, sc, fresh()), b["expected"], "%s plain" % case["id"])
            continue
        res = _dev(b["residual"])
        y1 = _run(llmie, case, x, wq, sc, fresh(), bias=bias, residual=res.clone())
        _assert_bits(y1, b["expected"], "%s bias + residual" % case["id"])
        y2 = res.clone()
        _run(llmie, case, x, wq, sc, y2, bias=bias, residual=y2)
        _assert_bits(y2, b["expected"], "%s residual in place" % case["id"])
        assert torch.equal(y1.view(torch.int16), y2.view(torch.int16)), "%s: in place differs from the separate residual" % case["id"]


# ---------------------------------------------------------------- random data
@pytest.fixture(scope="module")
def random_ops():
    """(x, wq, scale, float64 product over the de-quantised weights) per shape, computed once"""
    cache = {}

    def get(M, K, N):
        if (M, K, N) not in cache:
            rng = np.random.default_rng(M * 7 + N)
            w = (rng.standard_normal((N, K)) * 0.05 * rng.choice(np.array([1.0, 8.0, 0.1]), (N, 1))).astype(np.float16)
            wq, sc = MX.quantize(w)
            x = rng.standard_normal((M, K)).astype(np.float16)
            cache[(M, K, N)] = (x, wq, sc, x.astype(np.float64) @ MX.dequantize(wq, sc).T)
        return cache[(M, K, N)]
    return get


@pytest.mark.parametrize("M,K,N,route", [(1, 4096, 512, "mxfp4_gemv"), (2, 11008, 4097, "mxfp4_gemv"), (33, 11008, 256, "mxfp4_mfma"),
                                         (250, 4096, 768, "image_prefill+tiles256_part")])
def test_random_data_within_the_int4_bound(llmie, random_ops, M, K, N, route):
    x, wq, sc, exp = random_ops(M, K, N)
    xd, wd, sd = _dev(x), _dev(wq), _dev(sc)
    y = torch.full((M, N), float("nan"), dtype=F16, device=DEV)
    assert _route(llmie, xd, wd, sd, y, "auto") == route
    llmie.linear_mxfp4(xd, wd, sd, y)
    torch.cuda.synchronize()
    err = np.abs(y.float().cpu().numpy().astype(np.float64) - exp)
    print("M=%d K=%d N=%d: max err %.3g, max err / bound %.3g" % (M, K, N, err.max(), (err / (2e-3 + 2e-3 * np.abs(exp))).max()))
    assert (err <= 2e-3 + 2e-3 * np.abs(exp)).all()


@pytest.mark.parametrize("M", [3, 33, 100, 250])
def test_same_inputs_same_bits_and_nothing_written_behind_y(llmie, random_ops, M):
    K, N = 4096, 768 if M == 250 else 515
    x, wq, sc, _ = random_ops(M, K, N)
    xd, wd, sd = _dev(x), _dev(wq), _dev(sc)
    guard = 4096
    bufs = []
    for _ in range(2):
        buf = torch.full((M * N + guard,), float("nan"), dtype=F16, device=DEV)
        buf[M * N:] = 777.0
        llmie.linear_mxfp4(xd, wd, sd, buf[:M * N].view(M, N))
        bufs.append(buf)
    torch.cuda.synchronize()
    assert torch.equal(bufs[0].view(torch.int16), bufs[1].view(torch.int16))
    assert not torch.isnan(bufs[0][:M * N]).any()
    assert (bufs[0][M * N:] == 777.0).all()


@pytest.mark.parametrize("M", [4, 40])
def test_captured_graph_replays_the_eager_result(llmie, random_ops, M):
    K, N = 4096, 515
    x, wq, sc, _ = random_ops(M, K, N)
    xd, wd, sd = _dev(x), _dev(wq), _dev(sc)
    eager = llmie.linear_mxfp4(xd, wd, sd, torch.empty((M, N), dtype=F16, device=DEV))
    torch.cuda.synchronize()
    y = torch.zeros((M, N), dtype=F16, device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        llmie.linear_mxfp4(xd, wd, sd, y)
    for _ in range(2):
        y.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(y.view(torch.int16), eager.view(torch.int16))


def test_refusals_on_device_pointers(llmie):
    x = torch.zeros((4, 64), dtype=F16, device=DEV)
    wq, sc, y = torch.zeros((16, 32), dtype=torch.uint8, device=DEV), torch.full((16, 2), 127, dtype=torch.uint8, device=DEV), torch.zeros((4, 16), dtype=F16, device=DEV)
    lib = llmie.lib()
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    assert lib.llmie_linear_mxfp4(p(x, 2), p(wq), p(sc), p(y), 4, 32, 16, None, None, None, 0, None) == -2
    assert lib.llmie_linear_mxfp4(p(x), p(wq, 8), p(sc), p(y), 4, 32, 16, None, None, None, 0, None) == -2
    assert lib.llmie_linear_mxfp4(p(x), p(wq), p(sc, 1), p(y), 4, 32, 16, None, None, None, 0, None) == 0   # scales: any alignment
    torch.cuda.synchronize()
