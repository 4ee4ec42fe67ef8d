"""What the engine cases of tests/moe_mxfp4_engine_ref.py claim, asserted from the reference alone (no GPU): the case list, exact
dequantisation of the expert matrices, the routing-stability cap, the bar between the two evaluations and the distance of an engine
that ignored its experts; for the epilogue cases, that each part of the epilogue moves the output by more than the bar."""
import numpy as np
import pytest
from conftest import systematic_error

import moe_engine_ref as er
import moe_mxfp4_engine_ref as xr

BAR = 2e-2


def test_case_list():
    ids = [c["base_id"] for c in xr.CASES if not c["epi"]]
    assert ids == [c["id"] for c in er.CASES if c["E"] == 8] and "decode_stack_e8" in ids and "decode_window_e8" in ids
    epi = [c for c in xr.CASES if c["epi"]]
    assert sorted(c["kind"] for c in epi) == ["decode", "prefill"]
    assert set(xr.SALT) <= set(xr.BY_ID)


@pytest.mark.parametrize("case", xr.CASES, ids=[c["id"] for c in xr.CASES])
def test_engine_case_reference_meets_the_stability_cap(case):
    """at most 10 % of the case's rows have an unstable routing, the two evaluations agree within half the bar on the stable rows, and an
    engine that ran dense FFNs instead of its experts would lie at least 10 bars away"""
    b, y16, y64, stable = xr.reference(case)
    rows = er.n_rows(case)
    assert y16.shape == (rows, er.H) and np.isfinite(y16).all()
    print("%s: %d of %d rows unstable" % (case["id"], int((~stable).sum()), rows))
    assert (~stable).sum() <= 0.1 * rows, (case["id"], int((~stable).sum()), rows)
    own = max(systematic_error(y16[m], y64[m])[0] for m in np.nonzero(stable)[0])
    assert own <= 1e-2, (case["id"], own)
    apart = systematic_error(xr.dense_twin(b)[stable], y16[stable])[0]
    assert apart >= 10 * BAR, (case["id"], apart)
    for lw, sparse in zip(b["weights"], case["sparse"]):
        for s in (lw["e_gate_up_s"], lw["e_down_s"]):
            assert 104 <= int(s.min()) and int(s.max()) <= 140


@pytest.mark.parametrize("cid", ["mx4_gptoss_decode_r32", "mx4_gptoss_prefill_t168"])
def test_epilogue_parts_show_in_the_engine_output(cid):
    """a sparse layer that dropped its biases or ran the plain act lies more than a bar away on the stable rows"""
    case = xr.BY_ID[cid]
    b, y16, y64, stable = xr.reference(case)
    for drop in ("router_bias", "e_gate_up_bias", "e_down_bias", "act"):
        w2 = [dict(lw) for lw in b["weights"]]
        c2 = case
        if drop == "act":
            c2 = dict(case, epi=False)   # (no bias either: the plain FFN)
        else:
            for lw in w2:
                lw[drop] = np.zeros_like(lw[drop])
        other = xr._run(dict(b, weights=w2, case=c2), True)[0]
        apart = systematic_error(other[stable], y16[stable])[0]
        print("%s without %s: %.3f" % (cid, drop, apart))
        assert apart >= 2 * BAR, (cid, drop, apart)
