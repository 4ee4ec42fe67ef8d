"""llmie_moe_route against the float64 restatement of tests/moe_cases.py on router operands whose logits are exact in fp32 in any
summation order: selection, tie-breaks included, has one right answer, so the expert ids are compared for equality.  Weights: 1e-6
relative of float64 -- fp32 exp and one division; the project's bar for fp32 kernels is 1e-4, this keeps two decimal orders spare."""
import numpy as np
import pytest

import moe_cases as mc

pytestmark = pytest.mark.gpu


def _run(llmie, x, router, k, flags):
    import torch
    ids, w = llmie.moe_route(torch.from_numpy(x).cuda(), torch.from_numpy(router).cuda(), k, flags=flags)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), w.cpu().numpy()


@pytest.mark.parametrize("case", mc.CASES, ids=[c["id"] for c in mc.CASES])
def test_ids_exact_and_weights_close(llmie, case):
    b = mc.build(case)
    for flags in (0, mc.SOFTMAX_ALL):
        ids, w, r = mc.route(b["x"], b["router"], case["k"], flags)
        got_ids, got_w = _run(llmie, b["x"], b["router"], case["k"], flags)
        assert got_ids.dtype == np.int32 and got_w.dtype == np.float32 and got_ids.shape == ids.shape == got_w.shape
        assert np.array_equal(got_ids, ids), (case["id"], flags, np.argwhere(got_ids != ids)[:4].tolist())
        rel = np.abs(got_w.astype(np.float64) - w) / w
        print("%s flags=%d: worst weight error %.2e relative" % (case["id"], flags, rel.max()))
        assert rel.max() <= 1e-6, (case["id"], flags, float(rel.max()))
        if flags == 0:
            assert np.abs(got_w.astype(np.float64).sum(axis=1) - 1).max() <= 1e-6
        elif case["E"] > case["k"]:
            assert (got_w.astype(np.float64).sum(axis=1) < 1).all()


def test_nan_logits_rank_last_and_ids_stay_in_range(llmie):
    case = mc.BY_ID["r17_e128"]
    b = mc.build(case)
    E, k = case["E"], case["k"]
    x, router = b["x"].copy(), b["router"].copy()
    x[3, 5] = np.nan            # every logit of the row is a NaN
    x[7, :] = np.nan
    x[9, 0] = np.inf            # +-inf products: logits +inf, -inf or NaN
    router[40, 17] = np.nan     # one expert's logit is a NaN in every row
    with np.errstate(invalid="ignore", over="ignore"):
        ids, w, r = mc.route(x, router, k)
    got_ids, got_w = _run(llmie, x, router, k, 0)
    assert got_ids.min() >= 0 and got_ids.max() < E
    assert all(len(set(row)) == k for row in got_ids.tolist())
    clean = np.array([m for m in range(case["rows"]) if m not in (3, 7, 9)])
    assert np.array_equal(got_ids[clean], ids[clean]) and not (got_ids[clean] == 40).any()
    assert np.abs(got_w[clean].astype(np.float64) - w[clean]).max() <= 1e-6
    # all-NaN rows: every logit ranks as -inf, so the ids are the k lowest
    assert got_ids[3].tolist() == list(range(k)) and got_ids[7].tolist() == list(range(k))
    # small shapes: one expert, and k = E
    for E2, k2 in ((1, 1), (4, 4)):
        xx = np.full((2, 64), np.nan, np.float16)
        g, _ = _run(llmie, xx, np.ones((E2, 64), np.float16), k2, 0)
        assert g.tolist() == [list(range(k2))] * 2
