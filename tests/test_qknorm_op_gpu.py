"""llmie_qk_norm on the GPU against qknorm_cases.head_norm (float64, one fp16 rounding) on qknorm_cases.op_inputs.

Bound, derived: |got - ref| <= 2^-10 |ref| + 2^-24.  The only rounding of the operator is the final fp16 one, 2^-11 relative or half a
subnormal step (2^-25); the fp32 sum of at most 128 squares and the root contribute below 2^-17.  The reference is itself rounded to
fp16, so the two can differ by one fp16 step where the unrounded value lies near a tie: 2^-10 relative, 2^-24 for subnormals.
V columns keep their bits; a row's result does not depend on where the row lies; a refused call writes nothing.
"""
import numpy as np
import pytest
import torch

import qknorm_cases as qc

pytestmark = pytest.mark.gpu
DEV, F16 = "cuda", torch.float16
GEOMETRIES = [(128, 8, 1), (128, 4, 4), (64, 4, 2)]   # head size, heads, KV heads


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check(got, x, nh, kvh, qg, kg, eps, what):
    ref = qc.normed_qkv(x, nh, kvh, qg, kg, eps)
    g = got.double().cpu().numpy()
    assert torch.equal(got[:, nh + kvh:].cpu(), torch.from_numpy(x[:, nh + kvh:])), what + ": v columns touched"
    err, tol = np.abs(g - ref)[:, :nh + kvh], (2.0 ** -10 * np.abs(ref) + 2.0 ** -24)[:, :nh + kvh]
    print("%s: largest error / bound %.3f" % (what, (err / tol).max()))
    assert np.isfinite(g).all() and (err <= tol).all(), "%s: error / bound %.3g" % (what, (err / tol).max())


@pytest.mark.parametrize("hs,nh,kvh", GEOMETRIES)
@pytest.mark.parametrize("rows", [1, 3, 257])
def test_qk_norm_matches_head_norm(llmie, rows, hs, nh, kvh):
    x = qc.op_inputs(rows, nh, kvh, hs, seed=rows + hs)
    if rows == 257:
        x[200] = x[0]
    qg, kg = qc.gammas(1, hs, seed=hs + nh)
    xd = _dev(x)
    llmie.qk_norm(xd, nh, kvh, _dev(qg[0]), _dev(kg[0]), 1e-6)
    torch.cuda.synchronize()
    _check(xd, x, nh, kvh, qg[0], kg[0], 1e-6, "rows %d hs %d %d/%d" % (rows, hs, nh, kvh))
    if rows == 257:   # the same row at positions 0 and 200: the same bits
        assert torch.equal(xd[0], xd[200])


@pytest.mark.parametrize("eps", [0.0, 1e-5, 0.25])
def test_eps_is_read(llmie, eps):
    hs, nh, kvh = 128, 4, 4
    x = qc.op_inputs(3, nh, kvh, hs, seed=9)
    qg, kg = qc.gammas(1, hs, seed=4)
    xd = _dev(x)
    llmie.qk_norm(xd, nh, kvh, _dev(qg[0]), _dev(kg[0]), eps)
    torch.cuda.synchronize()
    _check(xd, x, nh, kvh, qg[0], kg[0], eps, "eps %g" % eps)
    # ... and eps = 1e-6 is another result on the head whose mean square is about 1e-6
    tq, _ = qc.tiny_heads(nh, kvh)
    other = qc.normed_qkv(x, nh, kvh, qg[0], kg[0], 1e-6)
    assert np.abs(other[:, tq] - xd[:, tq].double().cpu().numpy()).max() > 0.05 * np.abs(other[:, tq]).max()


def test_refused_calls_write_nothing(llmie):
    hs, nh, kvh = 128, 4, 2
    g = torch.ones(hs + 8, dtype=F16, device=DEV)
    good = g[:hs]
    cases = [("fp32", torch.randn((3, nh + 2 * kvh, hs), device=DEV), good, good, 1e-6, r"\(-2\).*fp16 only"),
             ("head size 32", torch.randn((3, nh + 2 * kvh, 32), device=DEV).to(F16), good[:32], good[:32], 1e-6, r"\(-2\).*head_size 64 / 128"),
             ("gamma off by 8 bytes", torch.randn((3, nh + 2 * kvh, hs), device=DEV).to(F16), g[4:4 + hs], good, 1e-6, r"\(-1\).*16-byte aligned"),
             ("negative eps", torch.randn((3, nh + 2 * kvh, hs), device=DEV).to(F16), good, good, -1.0, r"\(-1\).*eps"),
             ("nan eps", torch.randn((3, nh + 2 * kvh, hs), device=DEV).to(F16), good, good, float("nan"), r"\(-1\).*eps")]
    for what, x, qg, kg, eps, match in cases:
        x0 = x.clone()
        with pytest.raises(llmie.LlmieError, match=match):
            llmie.qk_norm(x, nh, kvh, qg, kg, eps)
        torch.cuda.synchronize()
        assert torch.equal(x, x0), what
    x = torch.randn((3, nh + 2 * kvh, hs), device=DEV).to(F16)
    x0 = x.clone()
    with pytest.raises(llmie.LlmieError, match=r"\(-1\).*kv_head_num"):
        llmie.qk_norm(x.view(3, 8, hs), 5, 2, good, good, 1e-6)
    torch.cuda.synchronize()
    assert torch.equal(x, x0)
