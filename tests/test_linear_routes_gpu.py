"""Every projection route of llmie_linear / _w8a16 / _w4a16 with the residual add in place (y == residual).

llmie_decoder_prefill's lean sequence adds the O and down projections into their own residual stream (proj(attn, Wo, S, residual=S)):
correct only where every route reads a residual element in the lane that writes it.  Each case below names the route its shape,
workspace and operand offsets select (linear_f16_nk / linear_wq predicates and time models), runs y = x . W^T + b + r once with a
separate residual and once in place, compares both with a float64 reference on the (de-quantised) weights and requires the two
outputs to be bit-identical.  Every route has a case with ragged M and N edges.

Which route each case takes is asserted on the host, without a GPU, by tests/test_linear_routes_cpu.py (llmie_linear_route on these
very case lists: the id's leading part names the route).
"""
import numpy as np
import pytest
import torch

from test_prefill_gpu import _quantise

pytestmark = pytest.mark.gpu
DEV, F16 = "cuda", torch.float16


def _h(a):
    return a.astype(np.float16).astype(np.float32)


def _offset_view(a, elems):
    """fp16 device copy of `a` at `elems` fp16 elements (2 bytes each) past a 256-byte aligned allocation"""
    buf = torch.empty(a.size + elems, dtype=F16, device=DEV)
    v = buf[elems:].view(a.shape)
    v.copy_(torch.from_numpy(a).to(F16))
    return v


# (id, M, K, N, workspace, x offset in fp16 elements): the route each selects is the id's middle part
F16_CASES = [
    ("gemv_m5", 5, 4096, 4000, "auto", 0),             # M <= 8: K-split GEMV
    ("skinny_m40_nows", 40, 4096, 1000, None, 0),      # M <= 64 without a workspace: skinny MFMA kernel
    ("splitk0_m20", 20, 4096, 1000, "auto", 0),        # split-K form 0 (M <= 32)
    ("splitk2_m50", 50, 4096, 4000, "auto", 0),        # split-K form 2 (64-row LDS-DMA tile, 33..64)
    ("splitk1_m100", 100, 4096, 4000, "auto", 0),      # split-K form 1 (128-row LDS-DMA tile, 65..128)
    ("splitk1_m150", 150, 4096, 4000, "auto", 0),      # 129..192: two passes (128 + 22 rows)
    ("passes_m200", 200, 4096, 4096, "auto", 0),       # > 192, grid does not fill: 128-row split-K passes (time model)
    ("passes_m300_n4000", 300, 4096, 4000, "auto", 0),
    ("passes_m384_down", 384, 11008, 4096, "auto", 0),
    ("midtiles_m400", 400, 4096, 4096, "auto", 0),     # passes cost more than one partly filled 256 x 128 round: gemm256
    ("midtiles_m700_n4000", 700, 4096, 4000, "auto", 0),
    ("midtiles_m768_down", 768, 11008, 4096, "auto", 0),
    ("midtiles_m250_nows", 250, 4096, 4000, None, 0),  # no workspace: the partial grid whatever the time model says
    ("tiled_m100_nows", 100, 4096, 4000, None, 0),     # 64 < M <= 192 without a workspace: tiled_mfma_f16_kernel<true>
    ("tiled_m150_nows", 150, 1024, 1000, None, 0),
    ("generic_k1001", 70, 1001, 1000, "auto", 0),      # K % 8 != 0: launch_generic
    ("generic_xoff2", 300, 4096, 1000, "auto", 1),     # x 2 bytes past 16-byte alignment: launch_generic
]


def _run_f16(llmie, x, w, b, r, ws):
    y1 = torch.full(r.shape, 99.0, dtype=F16, device=DEV)
    llmie.linear(x, w, y1, bias=b, residual=r.clone(), workspace=ws)
    y2 = r.clone()
    llmie.linear(x, w, y2, bias=b, residual=y2, workspace=ws)
    torch.cuda.synchronize()
    return y1, y2


@pytest.mark.parametrize("name,M,K,N,ws,xoff", F16_CASES, ids=[c[0] for c in F16_CASES])
def test_f16_route_inplace_residual(llmie, name, M, K, N, ws, xoff):
    rng = np.random.default_rng(M * 31 + K + N)
    x, w = _h(rng.standard_normal((M, K)).astype(np.float32)), _h(rng.standard_normal((N, K)).astype(np.float32) / np.sqrt(K))
    b, r = _h(rng.standard_normal(N).astype(np.float32)), _h(rng.standard_normal((M, N)).astype(np.float32))
    xd = _offset_view(x, xoff)
    y1, y2 = _run_f16(llmie, xd, torch.from_numpy(w).to(DEV).to(F16), torch.from_numpy(b).to(DEV).to(F16),
                      torch.from_numpy(r).to(DEV).to(F16), ws)
    exp = x.astype(np.float64) @ w.astype(np.float64).T + b[None, :] + r
    for y in (y1, y2):
        err = np.abs(y.float().cpu().numpy() - exp)
        assert (err <= 4e-3 + 2e-3 * np.abs(exp)).all(), "max err %g" % err.max()
    assert torch.equal(y1, y2), "in-place residual differs from the separate one in %d elements" % (y1 != y2).sum().item()


# (id, bits, M, K, N, group, workspace)
WQ_CASES = [
    ("i8_gemv_m7", 8, 7, 4096, 4000, 0, "auto"),            # M <= 8: K-split GEMV on int8 rows
    ("i8_skinny_m40_nows", 8, 40, 4096, 1000, 0, None),     # M <= 64 without a workspace: skinny_mfma_w8_kernel
    ("i8_splitk_m100", 8, 100, 4096, 1000, 0, "auto"),      # linear_splitk(8): 8 < M < 192
    ("i8_splitk_m150", 8, 150, 4096, 4000, 0, "auto"),
    ("i8_midpasses_m200", 8, 200, 4096, 4096, 0, "auto"),   # 192..256, grid does not fill: int8 split-K passes (time model)
    ("i8_midpasses_m250_n4000", 8, 250, 4096, 4000, 0, "auto"),
    ("i8_image_m300", 8, 300, 4096, 4096, 0, "auto"),       # 257..768: fp16 image + partly filled 256-row grid
    ("i8_image_m700_down", 8, 700, 11008, 4000, 0, "auto"),
    ("i8_image_k1152_m100", 8, 100, 1152, 1000, 0, "auto"),  # K % 256 != 0 beyond 64 rows: fp16 image of W (any M)
    ("i4_gemv_m3", 4, 3, 4096, 4000, 128, "auto"),          # M <= 4: K-split GEMV on int4 rows
    ("i4_splitk_m50", 4, 50, 4096, 1000, 128, "auto"),      # group 128, M > 8: split-K, passes of 64 rows
    ("i4_splitk_m150", 4, 150, 4096, 4000, 128, "auto"),
    ("i4_chunks_g64_m20", 4, 20, 4096, 1000, 64, "auto"),   # group 64: GEMV row chunks
    ("i4_chunks_m40_nows", 4, 40, 1024, 1000, 128, None),   # no workspace: GEMV row chunks
    ("i4_image_m300", 4, 300, 4096, 4000, 128, "auto"),     # M >= 192: fp16 image + the fp16 GEMM
    ("i4_image_g64_m200", 4, 200, 4096, 4096, 64, "auto"),
]


@pytest.mark.parametrize("name,bits,M,K,N,group,ws", WQ_CASES, ids=[c[0] for c in WQ_CASES])
def test_quantised_route_inplace_residual(llmie, name, bits, M, K, N, group, ws):
    rng = np.random.default_rng(M * 37 + K + N + bits)
    x, w = _h(rng.standard_normal((M, K)).astype(np.float32)), _h(rng.standard_normal((N, K)).astype(np.float32) / np.sqrt(K))
    b, r = _h(rng.standard_normal(N).astype(np.float32)), _h(rng.standard_normal((M, N)).astype(np.float32))
    q, s, deq = _quantise(w, "int8" if bits == 8 else "int4", group)
    xd, qd, sd, bd, rd = (torch.from_numpy(a).to(DEV) for a in (x, q, s, b, r))
    xd, bd, rd = xd.to(F16), bd.to(F16), rd.to(F16)

    def run(y, residual):
        if bits == 8:
            llmie.linear_w8a16(xd, qd, sd, y, bias=bd, residual=residual, workspace=ws)
        else:
            llmie.linear_w4a16(xd, qd, sd, y, group, bias=bd, residual=residual, workspace=ws)

    y1 = torch.full((M, N), 99.0, dtype=F16, device=DEV)
    run(y1, rd.clone())
    y2 = rd.clone()
    run(y2, y2)
    torch.cuda.synchronize()
    exp = x.astype(np.float64) @ deq.astype(np.float64).T + b[None, :] + r
    for y in (y1, y2):
        err = np.abs(y.float().cpu().numpy() - exp)
        assert err.max() <= 8e-3, "max err %g" % err.max()
    assert torch.equal(y1, y2), "in-place residual differs from the separate one in %d elements" % (y1 != y2).sum().item()
