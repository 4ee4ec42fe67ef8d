"""llmie_moe_ffn_ex / llmie_moe_route_ex on the GPU against the float64 restatement of tests/moe_mxfp4_cases.py: MXFP4 experts on every
shape of moe_cases, the two ends of the pinned exponent range, and the full epilogue (router / gate-up / down biases, clamped SwiGLU)
on fp16 and MXFP4 experts.

Every case runs on the route the planner picks, on the grouped route by LLMIE_MOE_FORCE_GROUPED and, up to 16 rows, on the GEMV route
by LLMIE_MOE_FORCE_GEMV.  Bounds from the reference alone (moe_cases.bounds): the largest element error, the relative Frobenius error
and the projection of the error on the signal, each held to twice the error of the fp16-rounded restatement.  The router operands
have exact logits, with the bias too, so the device's routing is the reference's.

Bits as in test_moe_ffn_gpu.py: two runs agree; permuted rows give permuted output rows; a row alone gives the bits it has inside a
batch on the same route; two sentinel rows behind y[rows] and the bytes behind the declared workspace size are unchanged."""
import numpy as np
import pytest

import moe_cases as mc
import moe_mxfp4_cases as mq
from conftest import systematic_error

pytestmark = pytest.mark.gpu

SENTINEL_ROWS, SENTINEL_BYTES = 2, 1024
_built = {}
DEV_NAMES = ("router", "router_bias", "gate_up", "down", "gate_up_q", "gate_up_s", "down_q", "down_s", "gate_up_bias", "down_bias")


def built(llmie, case):
    """(operands, reference, expert descriptor on the device) of a case: built once, shared by the tests, never modified"""
    import torch
    if case["id"] not in _built:
        b = mq.build(case)
        dev = {n: torch.from_numpy(b[n]).cuda() for n in DEV_NAMES if b.get(n) is not None}
        kw = dict(router_bias=dev.get("router_bias"), gate_up_bias=dev.get("gate_up_bias"), down_bias=dev.get("down_bias"), act=b["act"],
                  alpha=b["alpha"], limit=b["limit"])
        if case["fmt"] == "f16":
            ex = llmie.MoeExperts(dev["router"], dev["gate_up"], dev["down"], **kw)
        else:
            ex = llmie.MoeExperts(dev["router"], dev["gate_up_q"], dev["down_q"], gate_up_scale=dev["gate_up_s"], down_scale=dev["down_s"], **kw)
        _built[case["id"]] = (b, mq.reference(b), ex)
    return _built[case["id"]]


def routes_of(case, llmie):
    out = [("default", 0), ("grouped", llmie.MOE_FORCE_GROUPED)]
    if case["rows"] <= mc.GEMV_MAX_ROWS:
        out.append(("gemv", llmie.MOE_FORCE_GEMV))
    return out


def run(llmie, case, ex, x, resid, flags):
    """y [rows, H] of the call, after checking the sentinels behind y and behind the declared workspace"""
    import torch
    rows, H = x.shape
    declared = llmie.lib().llmie_moe_workspace_bytes(rows, H, case["Ie"], case["E"], case["k"])
    ws = torch.full((declared + SENTINEL_BYTES,), 0xA5, dtype=torch.uint8, device="cuda")
    y = torch.full((rows + SENTINEL_ROWS, H), -777.0, dtype=torch.float16, device="cuda")
    xd = torch.from_numpy(x).cuda()
    rd = None if resid is None else torch.from_numpy(resid).cuda()
    llmie.moe_ffn_ex(xd, ex, y, case["k"], resid=rd, flags=flags | case["flags"], workspace=ws, rows=rows, workspace_bytes=declared)
    torch.cuda.synchronize()
    assert (y[rows:] == -777.0).all().item(), "a row behind y[rows] was written"
    assert (ws[declared:] == 0xA5).all().item(), "bytes behind the declared workspace size were written"
    return y[:rows].cpu().numpy()


@pytest.mark.parametrize("case", mq.ALL_CASES, ids=[c["id"] for c in mq.ALL_CASES])
def test_every_route_against_float64(llmie, case):
    b, ref, ex = built(llmie, case)
    bd = ref["bounds"]
    plan = dict(w.split("=") for w in llmie.moe_ffn_plan_ex(case["rows"], case["H"], case["Ie"], case["E"], case["k"], 0, ex.format, b["act"]).split())
    assert (plan["route"], int(plan["rt"])) == mq.expected_plan(case)[:2]
    assert plan["format"] == case["fmt"]
    report = []
    for name, flags in routes_of(case, llmie):
        got = run(llmie, case, ex, b["x"], b["resid"], flags).astype(np.float64)
        assert np.isfinite(got).all()
        err = float(np.abs(got - ref["y64"]).max())
        rel, proj = systematic_error(got, ref["y64"])
        print("%s %s (%s): max |err| %.3e / %.3e, rel %.3e / %.3e, projection %.3e" % (case["id"], name, plan["route"] if name == "default" else name,
                                                                                      err, bd["max_abs"], rel, bd["rel"], proj))
        if not (err <= bd["max_abs"] and rel <= bd["rel"] and proj <= bd["rel"]):
            report.append((name, err, bd["max_abs"], rel, proj, bd["rel"]))
    assert not report, report


BIT_IDS = ["r4_e8_mxfp4", "r16_i2112_mxfp4", "r17_e128_mxfp4", "r100_counts_mxfp4", "r300_counts_rt4_mxfp4", "r17_e128_mxfp4_epi", "r100_counts_f16_epi"]


@pytest.mark.parametrize("cid", BIT_IDS)
def test_bits_do_not_depend_on_position_or_company(llmie, cid):
    case = mq.BY_ID[cid]
    b, ref, ex = built(llmie, case)
    rows = case["rows"]
    perm = np.random.default_rng(5).permutation(rows)
    for name, flags in routes_of(case, llmie)[1:]:   # the forced routes: a smaller call must not change the route
        first = run(llmie, case, ex, b["x"], b["resid"], flags)
        assert not np.array_equal(first, b["resid"] if b["resid"] is not None else np.zeros_like(first))
        again = run(llmie, case, ex, b["x"], b["resid"], flags)
        assert np.array_equal(again.view(np.uint16), first.view(np.uint16)), (cid, name, "two runs differ")
        if rows > 1:
            got = run(llmie, case, ex, b["x"][perm], None if b["resid"] is None else b["resid"][perm], flags)
            assert np.array_equal(got.view(np.uint16), first[perm].view(np.uint16)), (cid, name, "permuted rows")
        for m in sorted({0, rows // 2, rows - 1}):
            alone = run(llmie, case, ex, b["x"][m:m + 1], None if b["resid"] is None else b["resid"][m:m + 1], flags)
            assert np.array_equal(alone.view(np.uint16), first[m:m + 1].view(np.uint16)), (cid, name, "row %d alone" % m)
    # the tile height of the grouped route does not show in a row's bits
    g1 = run(llmie, case, ex, b["x"], b["resid"], llmie.MOE_FORCE_GROUPED | llmie.MOE_FORCE_RT1)
    g4 = run(llmie, case, ex, b["x"], b["resid"], llmie.MOE_FORCE_GROUPED | llmie.MOE_FORCE_RT4)
    assert np.array_equal(g1.view(np.uint16), g4.view(np.uint16)), (cid, "RT1 against RT4")


@pytest.mark.parametrize("cid", ["r4_e8", "r17_e128", "r33_e128_all", "r100_counts", "r300_counts_rt4"])
def test_plain_f16_descriptor_returns_the_bits_of_moe_ffn(llmie, cid):
    import torch
    base = mc.BY_ID[cid]
    case = mq._case(base, "f16")
    b = mq.build(case)
    dev = {n: torch.from_numpy(b[n]).cuda() for n in ("router", "gate_up", "down")}
    ex = llmie.MoeExperts(dev["router"], dev["gate_up"], dev["down"])
    xd = torch.from_numpy(b["x"]).cuda()
    rd = None if b["resid"] is None else torch.from_numpy(b["resid"]).cuda()
    for name, flags in routes_of(case, llmie):
        y0 = torch.zeros_like(xd)
        llmie.moe_ffn(xd, dev["router"], dev["gate_up"], dev["down"], y0, case["k"], resid=rd, flags=flags | case["flags"])
        got = run(llmie, case, ex, b["x"], b["resid"], flags)
        assert np.array_equal(got.view(np.uint16), y0.cpu().numpy().view(np.uint16)), (cid, name)
        assert np.abs(got.astype(np.float64)).max() > 0


@pytest.mark.parametrize("cid", ["r1_e8_mxfp4_epi", "r4_e8_f16_epi", "r17_e128_mxfp4_epi", "r100_counts_mxfp4_epi", "r300_counts_rt4_f16_epi"])
def test_route_ex_with_and_without_the_router_bias(llmie, cid):
    import torch
    case = mq.BY_ID[cid]
    b, ref, ex = built(llmie, case)
    xd = torch.from_numpy(b["x"]).cuda()
    ids, w = llmie.moe_route_ex(xd, ex, case["k"], flags=case["flags"])
    assert np.array_equal(ids.cpu().numpy(), ref["experts"])
    assert np.abs(w.cpu().numpy().astype(np.float64) - ref["weights"]).max() <= 1e-6
    bare = llmie.MoeExperts(ex.router, ex.gate_up, ex.down, gate_up_scale=ex.gate_up_scale, down_scale=ex.down_scale)
    e0, w0, _ = mc.route(b["x"], b["router"], case["k"], case["flags"])
    ids0, wd0 = llmie.moe_route_ex(xd, bare, case["k"], flags=case["flags"])
    assert np.array_equal(ids0.cpu().numpy(), e0)
    assert np.abs(wd0.cpu().numpy().astype(np.float64) - w0).max() <= 1e-6
    ids1, wd1 = llmie.moe_route(xd, ex.router, case["k"], flags=case["flags"])
    assert torch.equal(ids1, ids0) and torch.equal(wd1, wd0)


def test_device_quantiser_makes_the_layout_of_the_cases(llmie):
    """llmie_quantize_mxfp4 on the flattened fp16 expert matrices writes the codes and scale bytes the cases carry"""
    import torch
    case = mq.BY_ID["r4_e8_mxfp4"]
    b, ref, ex = built(llmie, case)
    q = llmie.MoeExperts.quantize(ex.router, torch.from_numpy(b["gate_up16"]).cuda(), torch.from_numpy(b["down16"]).cuda())
    for got, want in ((q.gate_up, "gate_up_q"), (q.gate_up_scale, "gate_up_s"), (q.down, "down_q"), (q.down_scale, "down_s")):
        assert np.array_equal(got.cpu().numpy(), b[want]), want
    assert q.format == llmie.W_MXFP4 and (q.experts, q.inter, q.hidden) == (case["E"], case["Ie"], case["H"])


def test_refusals_on_real_operands(llmie):
    """every refusal of the descriptor, through the binding (the codes: test_moe_mxfp4_cpu.py); y stays untouched"""
    import torch
    case = mq.BY_ID["r4_e8_mxfp4_epi"]
    b, ref, ex = built(llmie, case)
    xd = torch.from_numpy(b["x"]).cuda()
    y = torch.full_like(xd, -777.0)
    M = llmie.MoeExperts
    full = dict(gate_up_scale=ex.gate_up_scale, down_scale=ex.down_scale)
    codes1 = torch.zeros(ex.gate_up.numel() + 16, dtype=torch.uint8, device="cuda")[8:8 + ex.gate_up.numel()].view(ex.gate_up.shape)
    bad = [
        ("a NULL scale", M(ex.router, ex.gate_up, ex.down, gate_up_scale=ex.gate_up_scale, format=llmie.W_MXFP4), "scale"),
        ("a scale with fp16", M(ex.router, ex.gate_up, ex.down, down_scale=ex.down_scale, format=llmie.W_F16), "scale"),
        ("misaligned codes", M(ex.router, codes1, ex.down, **full), "16-byte"),
        ("int8 experts", M(ex.router, ex.gate_up, ex.down, format=llmie.W_INT8, **full), "format"),
        ("limit 0", M(ex.router, ex.gate_up, ex.down, act=llmie.MOE_ACT_SWIGLU_CLAMPED, alpha=1.702, limit=0.0, **full), "limit"),
        ("limit inf", M(ex.router, ex.gate_up, ex.down, act=llmie.MOE_ACT_SWIGLU_CLAMPED, alpha=1.702, limit=float("inf"), **full), "limit"),
        ("alpha nan", M(ex.router, ex.gate_up, ex.down, act=llmie.MOE_ACT_SWIGLU_CLAMPED, alpha=float("nan"), limit=7.0, **full), "alpha"),
        ("unknown act", M(ex.router, ex.gate_up, ex.down, act=3, **full), "act"),
    ]
    for what, d, word in bad:
        with pytest.raises(llmie.LlmieError, match=word):
            llmie.moe_ffn_ex(xd, d, y, case["k"])
    torch.cuda.synchronize()
    assert (y == -777.0).all().item()
    # a 2-byte aligned bias and unaligned scale bytes are taken: the same bits as the aligned operands give
    def off(t, nbytes):
        raw = torch.zeros(t.numel() * t.element_size() + 32, dtype=torch.uint8, device="cuda")
        v = raw[nbytes:nbytes + t.numel() * t.element_size()].view(t.dtype).view(t.shape)
        v.copy_(t)
        return v
    shifted = M(ex.router, ex.gate_up, ex.down, gate_up_scale=off(ex.gate_up_scale, 1), down_scale=off(ex.down_scale, 3), router_bias=off(ex.router_bias, 2),
                gate_up_bias=off(ex.gate_up_bias, 6), down_bias=off(ex.down_bias, 10), act=ex.act, alpha=ex.alpha, limit=ex.limit)
    for name, flags in routes_of(case, llmie):
        got = run(llmie, case, shifted, b["x"], b["resid"], flags)
        want = run(llmie, case, ex, b["x"], b["resid"], flags)
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), name
