"""MXFP4 experts and the gpt-oss epilogue on an engine (llmie_decoder_moe_attach_ex), every case of tests/moe_mxfp4_engine_ref.py.

Reference and bar as in test_moe_engine_gpu.py: the oracle's per-kernel composition in its fp16-rounded evaluation with the expert
FFN of tests/moe_mxfp4_cases.py on the exact values of the codes; relative Frobenius error <= 2e-2 per row on the rows whose routing
is stable.  Which rows those are, the 10 % cap and the distance of an experts-ignoring engine are asserted from the reference alone
in tests/test_moe_mxfp4_engine_cpu.py.
Also: attach_ex + detach gives the dense engine's bits; descriptors beside tuples; the attach refusals; a captured decode step replays
on rows that route differently (fresh process).  The C++ mirror's driver runs from tests/test_moe_mxfp4_cpp_gpu.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from conftest import systematic_error

import moe_engine_cases as me
import moe_engine_ref as er
import moe_mxfp4_engine_ref as xr

pytestmark = pytest.mark.gpu
DEV, F16 = me.DEV, me.F16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 2e-2
i32 = me.i32


def descriptors(llmie, weights, sparse, epi):
    """the `layers` argument of Decoder.moe_attach: one MoeExperts per sparse layer, None for a dense one"""
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    out = []
    for lw, s in zip(weights, sparse):
        if not s:
            out.append(None)
            continue
        kw = {}
        if epi:
            kw = dict(router_bias=d(lw["router_bias"]), gate_up_bias=d(lw["e_gate_up_bias"]), down_bias=d(lw["e_down_bias"]),
                      act=llmie.MOE_ACT_SWIGLU_CLAMPED, alpha=xr.ALPHA, limit=xr.LIMIT)
        out.append(llmie.MoeExperts(d(lw["router"]), d(lw["e_gate_up_q"]), d(lw["e_down_q"]), gate_up_scale=d(lw["e_gate_up_s"]),
                                    down_scale=d(lw["e_down_s"]), **kw))
    return out


@pytest.mark.parametrize("case", xr.CASES, ids=[c["id"] for c in xr.CASES])
def test_engine_case_against_the_oracle_composition(llmie, case):
    b, y16, y64, stable = xr.reference(case)
    dec = me.make_engine(llmie, b["weights"], case["hs"], kv8=case["cache"] == "e4m3")
    dec.moe_attach(descriptors(llmie, b["weights"], case["sparse"], case["epi"]), case["k"], max_tokens=max(er.n_rows(case), me.MAX_BATCH))
    if case["window"]:
        dec.set_window([case["window"]] + [0] * (len(case["sparse"]) - 1), sinks=case["sinks"])
    got = me.run_case(llmie, dec, b)
    dec.close()
    assert np.isfinite(got).all() and stable.any()
    worst = max(systematic_error(got[m], y16[m])[0] for m in np.nonzero(stable)[0])
    print("%s: worst stable row %.4f (bar %.3f), %d of %d rows stable" % (case["id"], worst, BAR, stable.sum(), len(stable)))
    assert worst <= BAR, (case["id"], worst)


def test_detach_restores_the_dense_bits_and_tuples_mix_with_descriptors(llmie):
    case = xr.BY_ID["mx4_gptoss_decode_r32"]
    b = xr.reference(case)[0]
    hs = case["hs"]
    dec, dense = me.make_engine(llmie, b["weights"], hs), me.make_engine(llmie, b["weights"], hs)
    g = torch.Generator().manual_seed(4)
    x = torch.randn((6, me.H), generator=g).to(DEV).to(F16)
    kd = (torch.randn((2, 6, 2, me.MAX_SEQ, hs), generator=g) * 0.5).to(DEV).to(F16)
    vd = (torch.randn((2, 6, 2, me.MAX_SEQ, hs), generator=g) * 0.5).to(DEV).to(F16)
    call = lambda eng: eng.forward(x, torch.empty_like(x), kd.clone(), vd.clone(), 99).clone()
    want = call(dense)
    ex = descriptors(llmie, b["weights"], (True, True), True)
    dec.moe_attach(ex, case["k"])
    attached = call(dec)
    dec.moe_detach()
    assert torch.equal(call(dec), want) and not torch.equal(attached, want)
    # an fp16 tuple beside an fp16 descriptor: one attach_ex call; the same bits as the tuples alone through llmie_decoder_moe_attach
    tuples = me.experts_of(b["weights"], (True, True))
    dec.moe_attach(tuples, case["k"])
    by_tuples = call(dec)
    dec.moe_detach()
    dec.moe_attach([tuples[0], llmie.MoeExperts(tuples[1]["router"], tuples[1]["gate_up"], tuples[1]["down"])], case["k"])
    assert torch.equal(call(dec), by_tuples)
    dec.moe_detach()
    for e in (dec, dense):
        e.close()


def test_attach_ex_refusals(llmie):
    case = xr.BY_ID["mx4_gptoss_decode_r32"]
    b = xr.reference(case)[0]
    hs, k, E = case["hs"], case["k"], case["E"]
    dec = me.make_engine(llmie, b["weights"], hs)
    ex = descriptors(llmie, b["weights"], (True, True), True)
    plain = descriptors(llmie, b["weights"], (True, True), False)
    tuples = me.experts_of(b["weights"], (True, True))
    with pytest.raises(llmie.LlmieError, match="expert format or act"):
        dec.moe_attach([ex[0], plain[1]], k)                                              # acts differ
    with pytest.raises(llmie.LlmieError, match="expert format or act"):
        dec.moe_attach([plain[0], tuples[1]], k)                                          # formats differ
    M = llmie.MoeExperts
    bad = M(plain[0].router, plain[0].gate_up, plain[0].down, gate_up_scale=plain[0].gate_up_scale, format=llmie.W_MXFP4)
    with pytest.raises(llmie.LlmieError, match="scale"):
        dec.moe_attach([bad, plain[1]], k)
    bad = M(plain[0].router, plain[0].gate_up, plain[0].down, gate_up_scale=plain[0].gate_up_scale, down_scale=plain[0].down_scale,
            act=llmie.MOE_ACT_SWIGLU_CLAMPED, alpha=1.702, limit=-1.0)
    with pytest.raises(llmie.LlmieError, match="limit"):
        dec.moe_attach([bad, None], k)
    lib = llmie.lib()
    err = lambda: lib.llmie_last_error().decode()
    arr = (llmie.MoeExpertsDesc * 2)(plain[0].desc(), plain[1].desc())
    need = dec.moe_workspace_bytes(me.MAX_BATCH, me.IE, E, k)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    assert lib.llmie_decoder_moe_attach_ex(dec.handle, arr, me.IE, E, k, 0, ws.data_ptr(), need - 1) == -4 and str(need) in err()
    assert lib.llmie_decoder_moe_attach_ex(dec.handle, arr, me.IE, E, k, 0, ws.data_ptr() + 16, need) == -4 and "256-byte aligned" in err()
    assert lib.llmie_decoder_moe_attach_ex(dec.handle, None, me.IE, E, k, 0, ws.data_ptr(), need) == -1 and "NULL pointer" in err()
    assert lib.llmie_decoder_moe_attach_ex(dec.handle, arr, me.IE, 129, k, 0, ws.data_ptr(), need) == -2 and "LLMIE_MOE_MAX_EXPERTS" in err()
    assert lib.llmie_decoder_moe_attach_ex(dec.handle, arr, 100, E, k, 0, ws.data_ptr(), need) == -2 and "inter=100" in err()
    empty = (llmie.MoeExpertsDesc * 2)()
    assert lib.llmie_decoder_moe_attach_ex(dec.handle, empty, me.IE, E, k, 0, ws.data_ptr(), need) == -1 and "no layer has a router" in err()
    # an adapter table and experts refuse each other, in this entry too
    table = llmie.lora_table(2, 2)
    seq_slot = torch.full((me.MAX_BATCH,), -1, dtype=torch.int32, device=DEV)
    dec.lora_attach(table, seq_slot)
    with pytest.raises(llmie.LlmieError, match="adapter table and experts"):
        dec.moe_attach(plain, k)
    dec.lora_detach()
    assert lib.llmie_decoder_moe_attach_ex(dec.handle, arr, me.IE, E, k, 0, ws.data_ptr(), need) == 0, err()
    # more rows than the attach workspace covers: refused before anything is enqueued
    T = 40
    hs2 = 128
    dec.close()
    b2 = xr.reference(xr.BY_ID["mx4_prefill_dense_e8_t5"])[0]
    dec = me.make_engine(llmie, b2["weights"], hs2)
    dec.moe_attach(descriptors(llmie, b2["weights"], (False, True), False), k)
    x = torch.randn((T, me.H), device=DEV).to(F16)
    y = torch.zeros_like(x)
    kc = torch.zeros((2, 1, 1, me.MAX_SEQ, hs2), dtype=F16, device=DEV)
    vc = torch.zeros_like(kc)
    with pytest.raises(llmie.LlmieError) as e:
        dec.prefill(x, y, kc, vc, i32([T]), i32([0]), T)
    assert "(-4)" in str(e.value) and "does not cover 40 rows" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert int(kc.abs().sum().item()) == 0 and int(y.abs().sum().item()) == 0
    dec.close()


def test_captured_step_follows_the_routing_of_new_rows():
    """fresh process: one decode step with MXFP4 experts captured with torch.cuda.graph; replays on other hidden rows, which route
    differently, equal the eager calls bit for bit (grouped route and GEMV route)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "moe_mxfp4_capture.py")], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["equal"] == [True, True, True], out
    assert out["routes_differ"] == [True, True], out
