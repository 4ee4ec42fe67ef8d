"""Every kind of tile plan of the 256-row GEMM family, run once through the public entry points at the smallest shape that has it.

K = 256 throughout: four fp16 / two e4m3 k-tiles, so the steady and the tail bodies of the kernels' k-loops both run.  The output is
pre-filled with 99.0, so a column band that no launch writes fails.  Reference: float64 on the host over the de-quantised operands
(SwiGLU: the projection rounded to fp16 before silu(gate) * up, as the entry points define it).  Bounds are those of the tests that
already cover the same entry points: test_f16_route_inplace_residual (fp16), test_quantised_route_inplace_residual (int8),
test_linear_fp8 (fp8), test_linear_swiglu_large_m and test_linear_fp8_swiglu (the SwiGLU forms).  The split cases also assert the 256
columns on either side of the seam between the two launches on their own: a range pointer (W, bias, residual, scales) offset wrongly
shows there first.

Which plan each case takes is asserted on the host by tests/test_gemm256_tiles_cpu.py.
"""
import functools

import numpy as np
import pytest
import torch

DEV, F16, K = "cuda", torch.float16, 256

# (id, form, M, N or two_inter, plan)
CASES = [
    ("wide", "plain", 2048, 8192, "256x32@0"),
    ("narrow", "plain", 1024, 4096, "128x32@0"),
    ("partial_ragged", "plain", 250, 4000, "128x32@0"),                # grid that does not fill the chip; ragged M and N
    ("split", "plain", 2048, 8448, "256x32@0 128x2@8192"),
    ("split_ragged", "plain", 2048, 8444, "256x32@0 128x2@8192"),      # last tile: 124 columns
    ("swiglu_split", "swiglu", 2048, 8328, "128x32@0 64x2@4096"),      # last tile: 4 columns
    ("swiglu_whole", "swiglu", 2048, 12288, "128x32@0 64x32@4096"),
]
_CASE = {c[0]: c for c in CASES}
ALL3 = ["wide", "narrow", "split"]


def _h(a):
    return a.astype(np.float16).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _operands(M, N):
    """x [M, K], w [N, K], bias [N], residual [M, N]: fp16-representable float32, shared by the formats (never modified)"""
    rng = np.random.default_rng(M * 31 + N)
    x, w = _h(rng.standard_normal((M, K)).astype(np.float32)), _h(rng.standard_normal((N, K)).astype(np.float32) / np.sqrt(K))
    return x, w, _h(rng.standard_normal(N).astype(np.float32)), _h(rng.standard_normal((M, N)).astype(np.float32))


def _d(a, dtype=F16):
    return torch.from_numpy(a).to(DEV).to(dtype)


def _check(y, exp, bound, plan):
    """bound(err, exp) -> bool array; whole output, then (two-launch plans) 256 columns on either side of the seam"""
    got = y.float().cpu().numpy()
    assert not (got == 99.0).all(axis=0).any(), "columns never written: %s" % np.nonzero((got == 99.0).all(axis=0))[0][:8]
    err = np.abs(got - exp)
    if " " in plan:
        seam = int(plan.split("@")[-1])
        for name, lo, hi in (("left", max(seam - 256, 0), seam), ("right", seam, min(seam + 256, exp.shape[1]))):
            ok = bound(err[:, lo:hi], exp[:, lo:hi])
            assert ok.all(), "columns [%d, %d) %s of the seam: %d wrong, max err %g" % (lo, hi, name, (~ok).sum(), err[:, lo:hi].max())
    ok = bound(err, exp)
    assert ok.all(), "%d wrong, max err %g, first wrong column %d" % ((~ok).sum(), err.max(), np.nonzero(~ok.all(axis=0))[0][0])


def _silu_mul(gu, inter):
    g, u = gu[:, :inter].astype(np.float64), gu[:, inter:].astype(np.float64)
    return g / (1.0 + np.exp(-g)) * u


def _fp8_operands(llmie, x, w):
    """device e4m3 codes + scales of w, and the float64 de-quantised operands of the fp8 projection (test_quant_gpu's definition)"""
    from test_quant_gpu import _e4m3_table, _to_e4m3
    wq = torch.empty(w.shape, dtype=torch.uint8, device=DEV)
    ws = torch.empty(w.shape[0], dtype=torch.float32, device=DEV)
    llmie.quantize_fp8(_d(w), wq, ws)
    wdeq = _e4m3_table()[wq.cpu().numpy()].astype(np.float64) * ws.cpu().numpy().astype(np.float64)[:, None]
    xs = (np.abs(x).max(axis=1) / np.float32(448.0)).astype(np.float32)
    xs[xs == 0] = 1.0
    _, xdeq = _to_e4m3(x / xs[:, None])
    return wq, ws, xdeq.astype(np.float64) * xs.astype(np.float64)[:, None], wdeq


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL3 + ["partial_ragged", "split_ragged"])
def test_f16_plan(llmie, name):
    _, _, M, N, plan = _CASE[name]
    x, w, b, r = _operands(M, N)
    y = torch.full((M, N), 99.0, dtype=F16, device=DEV)
    llmie.linear(_d(x), _d(w), y, bias=_d(b), residual=_d(r), workspace=None if name == "partial_ragged" else "auto")
    exp = x.astype(np.float64) @ w.astype(np.float64).T + b[None, :] + r
    _check(y, exp, lambda err, e: err <= 4e-3 + 2e-3 * np.abs(e), plan)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL3)
def test_int8_plan(llmie, name):
    from test_prefill_gpu import _quantise
    _, _, M, N, plan = _CASE[name]
    x, w, b, r = _operands(M, N)
    q, s, deq = _quantise(w, "int8", 0)
    y = torch.full((M, N), 99.0, dtype=F16, device=DEV)
    llmie.linear_w8a16(_d(x), torch.from_numpy(q).to(DEV), torch.from_numpy(s).to(DEV), y, bias=_d(b), residual=_d(r))
    exp = x.astype(np.float64) @ deq.astype(np.float64).T + b[None, :] + r
    _check(y, exp, lambda err, e: err <= 8e-3, plan)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL3)
def test_fp8_plan(llmie, name):
    _, _, M, N, plan = _CASE[name]
    x, w, b, r = _operands(M, N)
    wq, ws, xdeq, wdeq = _fp8_operands(llmie, x, w)
    work = torch.empty(llmie.linear_fp8_workspace_bytes(M, K, N), dtype=torch.uint8, device=DEV)
    y = torch.full((M, N), 99.0, dtype=F16, device=DEV)
    llmie.linear_fp8(_d(x), wq, ws, y, work, bias=_d(b), residual=_d(r))
    exp = xdeq @ wdeq.T + b[None, :] + r
    _check(y, exp, lambda err, e: err <= 3e-3 + 3e-3 * np.abs(e), plan)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["swiglu_split", "swiglu_whole"])
def test_f16_swiglu_plan(llmie, name):
    _, _, M, two_inter, plan = _CASE[name]
    x, w, _, _ = _operands(M, two_inter)
    y = torch.full((M, two_inter // 2), 99.0, dtype=F16, device=DEV)
    llmie.linear_swiglu(_d(x), _d(w), y)
    exp = _silu_mul(_h(x.astype(np.float64) @ w.astype(np.float64).T), two_inter // 2)
    _check(y, exp, lambda err, e: err <= 3e-3 + 3e-3 * np.abs(e), plan)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["swiglu_split", "swiglu_whole"])
def test_fp8_swiglu_plan(llmie, name):
    _, _, M, two_inter, plan = _CASE[name]
    x, w, _, _ = _operands(M, two_inter)
    wq, ws, xdeq, wdeq = _fp8_operands(llmie, x, w)
    work = torch.empty(llmie.linear_fp8_workspace_bytes(M, K), dtype=torch.uint8, device=DEV)
    y = torch.full((M, two_inter // 2), 99.0, dtype=F16, device=DEV)
    llmie.linear_fp8_swiglu(_d(x), wq, ws, y, work)
    exp = _silu_mul(_h(xdeq @ wdeq.T), two_inter // 2)
    _check(y, exp, lambda err, e: err <= 4e-3 + 4e-3 * np.abs(e), plan)
