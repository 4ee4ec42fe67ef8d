"""llmie_moe_ffn on both routes against the float64 restatement of tests/moe_cases.py.

Every case runs on the route the planner picks, on the grouped route by LLMIE_MOE_FORCE_GROUPED and, up to 16 rows, on the GEMV route
by LLMIE_MOE_FORCE_GEMV: the same inputs through both.  The router operands have exact logits (moe_cases), so the routing of the
device is the routing of the reference and every difference is arithmetic.

Bounds, from the reference alone (moe_cases.bounds): the largest element error and the relative Frobenius error of a run are held to
twice those of the fp16-rounded restatement against the float64 one; the projection of the error on the signal
(conftest.systematic_error) to the same relative bound, which Cauchy-Schwarz puts above it for any error of that size -- a dropped
or doubled expert weight projects at the order of the weight (test_moe_cpu.py shows it leaves the bounds by more than 10 x).

Bits: two runs agree; permuted rows give permuted output rows; a row alone gives the bits it has inside a batch on the same route;
two sentinel rows behind y[rows] and the bytes behind the declared workspace size are unchanged."""
import numpy as np
import pytest

import moe_cases as mc
from conftest import systematic_error

pytestmark = pytest.mark.gpu

SENTINEL_ROWS, SENTINEL_BYTES = 2, 1024
_built = {}


def built(case):
    """(operands, reference, device operands) of a case: built once, shared by the tests, never modified"""
    import torch
    if case["id"] not in _built:
        b = mc.build(case)
        dev = {n: torch.from_numpy(b[n]).cuda() for n in ("router", "gate_up", "down")}
        _built[case["id"]] = (b, mc.reference(b), dev)
    return _built[case["id"]]


def routes_of(case, llmie):
    out = [("default", 0), ("grouped", llmie.MOE_FORCE_GROUPED)]
    if case["rows"] <= mc.GEMV_MAX_ROWS:
        out.append(("gemv", llmie.MOE_FORCE_GEMV))
    return out


def run(llmie, case, dev, x, resid, flags):
    """y [rows, H] of the call, after checking the sentinels behind y and behind the declared workspace"""
    import torch
    rows, H = x.shape
    lib = llmie.lib()
    declared = lib.llmie_moe_workspace_bytes(rows, H, case["Ie"], case["E"], case["k"])
    ws = torch.full((declared + SENTINEL_BYTES,), 0xA5, dtype=torch.uint8, device="cuda")
    y = torch.full((rows + SENTINEL_ROWS, H), -777.0, dtype=torch.float16, device="cuda")
    xd = torch.from_numpy(x).cuda()
    rd = None if resid is None else torch.from_numpy(resid).cuda()
    llmie.moe_ffn(xd, dev["router"], dev["gate_up"], dev["down"], y, case["k"], resid=rd, flags=flags | case["flags"], workspace=ws, rows=rows,
                  workspace_bytes=declared)
    torch.cuda.synchronize()
    assert (y[rows:] == -777.0).all().item(), "a row behind y[rows] was written"
    assert (ws[declared:] == 0xA5).all().item(), "bytes behind the declared workspace size were written"
    return y[:rows].cpu().numpy()


@pytest.mark.parametrize("case", mc.CASES, ids=[c["id"] for c in mc.CASES])
def test_both_routes_against_float64(llmie, case):
    b, ref, dev = built(case)
    bd = ref["bounds"]
    plan = dict(w.split("=") for w in llmie.moe_ffn_plan(case["rows"], case["H"], case["Ie"], case["E"], case["k"]).split())
    assert (plan["route"], int(plan["rt"])) == mc.expected_plan(case["rows"], case["H"], case["Ie"], case["E"], case["k"])[:2]
    report = []
    for name, flags in routes_of(case, llmie):
        got = run(llmie, case, dev, b["x"], b["resid"], flags).astype(np.float64)
        assert np.isfinite(got).all()
        err = float(np.abs(got - ref["y64"]).max())
        rel, proj = systematic_error(got, ref["y64"])
        print("%s %s (%s): max |err| %.3e / %.3e, rel %.3e / %.3e, projection %.3e" % (case["id"], name, plan["route"] if name == "default" else name,
                                                                                      err, bd["max_abs"], rel, bd["rel"], proj))
        if not (err <= bd["max_abs"] and rel <= bd["rel"] and proj <= bd["rel"]):
            report.append((name, err, bd["max_abs"], rel, proj, bd["rel"]))
    assert not report, report


@pytest.mark.parametrize("cid", ["r4_e8", "r16_i2112", "r17_e128", "r100_counts", "r300_counts_rt4"])
def test_bits_do_not_depend_on_position_or_company(llmie, cid):
    case = mc.BY_ID[cid]
    b, ref, dev = built(case)
    rows = case["rows"]
    perm = np.random.default_rng(5).permutation(rows)
    for name, flags in routes_of(case, llmie)[1:]:   # the forced routes: a smaller call must not change the route
        first = run(llmie, case, dev, b["x"], b["resid"], flags)
        assert not np.array_equal(first, b["resid"] if b["resid"] is not None else np.zeros_like(first))
        again = run(llmie, case, dev, b["x"], b["resid"], flags)
        assert np.array_equal(again.view(np.uint16), first.view(np.uint16)), (cid, name, "two runs differ")
        if rows > 1:
            got = run(llmie, case, dev, b["x"][perm], None if b["resid"] is None else b["resid"][perm], flags)
            assert np.array_equal(got.view(np.uint16), first[perm].view(np.uint16)), (cid, name, "permuted rows")
        for m in sorted({0, rows // 2, rows - 1}):
            alone = run(llmie, case, dev, b["x"][m:m + 1], None if b["resid"] is None else b["resid"][m:m + 1], flags)
            assert np.array_equal(alone.view(np.uint16), first[m:m + 1].view(np.uint16)), (cid, name, "row %d alone" % m)


def test_no_residual_equals_a_zero_residual(llmie):
    case = mc.BY_ID["r17_e128"]
    b, ref, dev = built(case)
    for name, flags in routes_of(case, llmie)[1:]:
        zero = run(llmie, case, dev, b["x"], np.zeros_like(b["resid"]), flags)
        none = run(llmie, case, dev, b["x"], None, flags)
        assert np.array_equal(zero.view(np.uint16), none.view(np.uint16)) and np.abs(none).max() > 0
