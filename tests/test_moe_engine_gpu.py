"""Experts on an engine (llmie_decoder_moe_attach), every case of tests/moe_engine_ref.py: decode on dense, paged, ragged and e4m3
caches at 32 rows (grouped route) and 3 rows (GEMV route), prefill at 5 / 33 / 130 tokens and the three together on dense caches and
on pages with history, a dense layer between sparse ones, a sliding window with sinks.

Reference: built on the host from the oracle's per-kernel functions with the numpy expert FFN of tests/moe_cases.py in between
(moe_engine_ref.reference), in its fp16-rounded evaluation.  Bound: relative Frobenius error <= 2e-2 per row, the multi-layer fp16
bar of DESIGN.md section 2, on the rows whose routing is stable; which rows those are, that at most 10 % of a case's rows are not,
and that an engine which ignored its experts would lie >= 10 bars away are all decided from the reference alone and asserted in
tests/test_moe_cpu.py.
E = 1, k = 1 with the dense FFN's matrices as the one expert stays within the bar of the dense engine; attach + detach gives the
dense engine's bits; an adapter table and experts refuse each other; a captured decode step replays on rows that route differently.

llmie_decoder_prefill takes head_size 128 only, so the prefill cases run 2 / 1 heads of 128 where the decode cases run 4 / 2 of 64."""
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

pytestmark = pytest.mark.gpu
DEV, F16 = me.DEV, me.F16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 2e-2
i32 = me.i32


@pytest.mark.parametrize("case", er.CASES, ids=[c["id"] for c in er.CASES])
def test_engine_case_against_the_oracle_composition(llmie, case):
    b, y16, y64, stable = er.reference(case)
    dec = me.moe_engine(llmie, b["weights"], case["sparse"], case["hs"], case["k"], max_tokens=max(er.n_rows(case), me.MAX_BATCH),
                        kv8=case["cache"] == "e4m3")
    if case["window"]:
        dec.set_window([case["window"]] + [0] * (len(case["sparse"]) - 1), sinks=case["sinks"])
    got = me.run_case(llmie, dec, b)
    dec.close()
    assert np.isfinite(got).all() and stable.any()
    worst = max(systematic_error(got[m], y16[m])[0] for m in np.nonzero(stable)[0])
    print("%s: worst stable row %.4f (bar %.3f), %d of %d rows stable" % (case["id"], worst, BAR, stable.sum(), len(stable)))
    assert worst <= BAR, (case["id"], worst)


def prefill_entry(lens, hs, layers, seed):
    g = torch.Generator().manual_seed(seed)
    nh, kvh = me.geometry(hs)
    kd = (torch.randn((layers, len(lens), kvh, me.MAX_SEQ, hs), generator=g) * 0.5).to(DEV).to(F16)
    vd = (torch.randn((layers, len(lens), kvh, me.MAX_SEQ, hs), generator=g) * 0.5).to(DEV).to(F16)
    return lambda eng, x: eng.prefill(x, torch.empty_like(x), kd.clone(), vd.clone(), i32(lens), i32(0 for _ in lens), max(lens))


def decode_entry(hs, layers, bs, step, seed):
    g = torch.Generator().manual_seed(seed)
    nh, kvh = me.geometry(hs)
    kd = (torch.randn((layers, bs, kvh, me.MAX_SEQ, hs), generator=g) * 0.5).to(DEV).to(F16)
    vd = (torch.randn((layers, bs, kvh, me.MAX_SEQ, hs), generator=g) * 0.5).to(DEV).to(F16)
    return lambda eng, x: eng.forward(x, torch.empty_like(x), kd.clone(), vd.clone(), step)


def test_one_expert_with_the_dense_matrices_is_the_dense_engine(llmie):
    """E = 1, k = 1: weight 1, so the expert FFN on the dense FFN's matrices is the dense FFN; decode and prefill within the bar of
    the engine without experts, and after detach bit for bit that engine"""
    hs, inter = 128, me.IE
    w = me.layer_weights(hs, 2, 1, seed=5, inter=inter)
    for lw in w:
        lw["e_gate_up"], lw["e_down"] = lw["gate_up"][None].copy(), lw["down"][None].copy()
    dec = me.make_engine(llmie, w, hs, inter=inter)
    dense = me.make_engine(llmie, w, hs, inter=inter)
    dec.moe_attach(me.experts_of(w, (True, True)), 1, max_tokens=40)
    g = torch.Generator().manual_seed(13)
    xd, xp = torch.randn((4, me.H), generator=g).to(DEV).to(F16), torch.randn((38, me.H), generator=g).to(DEV).to(F16)
    dec_e = decode_entry(hs, 2, 4, 77, seed=1)
    pre_e = prefill_entry((5, 33), hs, 2, seed=2)
    attached = [dec_e(dec, xd).clone(), pre_e(dec, xp).clone()]
    want = [dec_e(dense, xd).clone(), pre_e(dense, xp).clone()]
    torch.cuda.synchronize()
    for a, b, name in zip(attached, want, ("decode", "prefill")):
        fro = max(systematic_error(a[m].float().cpu().numpy(), b[m].float().cpu().numpy())[0] for m in range(a.shape[0]))
        print("E=1 %s: worst row %.5f" % (name, fro))
        assert fro <= BAR and float(a.float().abs().sum()) > 0, (name, fro)
    dec.moe_detach()
    detached = [dec_e(dec, xd), pre_e(dec, xp)]
    torch.cuda.synchronize()
    assert torch.equal(detached[0], want[0]) and torch.equal(detached[1], want[1])
    for e in (dec, dense):
        e.close()


def test_attach_refusals_and_row_cover(llmie):
    hs, E, k = 128, 8, 2
    w = me.layer_weights(hs, 2, E, seed=3)
    dec = me.make_engine(llmie, w, hs)
    # an adapter table first: experts are refused; experts first: the table is refused
    table = llmie.lora_table(2, 2)
    seq_slot = torch.full((me.MAX_BATCH,), -1, dtype=torch.int32, device=DEV)
    dec.lora_attach(table, seq_slot)
    with pytest.raises(llmie.LlmieError, match="adapter table and experts"):
        dec.moe_attach(me.experts_of(w, (True, True)), k)
    dec.lora_detach()
    dec.moe_attach(me.experts_of(w, (True, True)), k)   # scratch for max_batch rows
    with pytest.raises(llmie.LlmieError, match="adapter table and experts"):
        dec.lora_attach(table, seq_slot)
    # more rows than the attach workspace covers: refused before anything is enqueued; what it covers runs
    T = 40
    x = torch.randn((T, me.H), device=DEV).to(F16)
    y = torch.zeros_like(x)
    kc = torch.zeros((2, 1, 1, me.MAX_SEQ, hs), dtype=F16, device=DEV)
    vc = torch.zeros_like(kc)
    with pytest.raises(llmie.LlmieError) as e:
        dec.prefill(x, y, kc, vc, i32([T]), i32([0]), T)
    assert "(-4)" in str(e.value) and "llmie_decoder_moe_attach does not cover 40 rows" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert int(kc.abs().sum().item()) == 0 and int(y.abs().sum().item()) == 0
    dec.prefill(x[:8], y[:8], kc, vc, i32([8]), i32([0]), 8)
    torch.cuda.synchronize()
    assert float(y[:8].float().abs().sum().item()) > 0
    # a flag with a row limit: attached fine, a call above the limit is refused before anything is enqueued
    dec.moe_detach()
    dec.moe_attach(me.experts_of(w, (True, True)), k, flags=llmie.MOE_FORCE_GEMV)
    kc.zero_(), vc.zero_(), y.zero_()
    with pytest.raises(llmie.LlmieError) as e:
        dec.prefill(x[:17], y[:17], kc, vc, i32([17]), i32([0]), 17)
    assert "(-2)" in str(e.value) and "LLMIE_MOE_FORCE_GEMV with 17 rows" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert int(kc.abs().sum().item()) == 0 and int(y.abs().sum().item()) == 0
    dec.prefill(x[:16], y[:16], kc, vc, i32([16]), i32([0]), 16)
    torch.cuda.synchronize()
    assert float(y[:16].float().abs().sum().item()) > 0
    dec.close()
    # engines the header excludes, bad expert geometry, short and misaligned workspaces
    lib = llmie.lib()
    arr = (llmie.MoeLayer * 2)()
    ex = me.experts_of(w, (True, True))
    for i in range(2):
        arr[i].router, arr[i].gate_up, arr[i].down = ex[i]["router"].data_ptr(), ex[i]["gate_up"].data_ptr(), ex[i]["down"].data_ptr()
    dec = me.make_engine(llmie, w, hs)
    need = dec.moe_workspace_bytes(me.MAX_BATCH, me.IE, E, k)
    assert need == lib.llmie_moe_workspace_bytes(me.MAX_BATCH, me.H, me.IE, E, k) > 0
    ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    err = lambda: lib.llmie_last_error().decode()
    assert lib.llmie_decoder_moe_attach(dec.handle, arr, me.IE, E, k, 0, ws.data_ptr(), need - 1) == -4 and str(need) in err()
    assert lib.llmie_decoder_moe_attach(dec.handle, arr, me.IE, E, k, 0, ws.data_ptr() + 16, need) == -4 and "256-byte aligned" in err()
    assert lib.llmie_decoder_moe_attach(dec.handle, None, me.IE, E, k, 0, ws.data_ptr(), need) == -1 and "NULL pointer" in err()
    assert lib.llmie_decoder_moe_attach(dec.handle, arr, me.IE, 129, k, 0, ws.data_ptr(), need) == -2 and "LLMIE_MOE_MAX_EXPERTS" in err()
    assert lib.llmie_decoder_moe_attach(dec.handle, arr, me.IE, E, 9, 0, ws.data_ptr(), need) == -2 and "top_k=9" in err()
    assert lib.llmie_decoder_moe_attach(dec.handle, arr, 100, E, k, 0, ws.data_ptr(), need) == -2 and "inter=100" in err()
    empty = (llmie.MoeLayer * 2)()
    assert lib.llmie_decoder_moe_attach(dec.handle, empty, me.IE, E, k, 0, ws.data_ptr(), need) == -1 and "no layer has a router" in err()
    assert lib.llmie_decoder_moe_attach(dec.handle, arr, me.IE, E, k, 0, ws.data_ptr(), need) == 0, err()
    assert lib.llmie_decoder_moe_detach(None) == -1 and "NULL decoder" in err()
    dec.close()
    lw = me.layer_weights(hs, 1, E, seed=3)
    d = lambda a: torch.from_numpy(a).to(DEV)
    cfg = dict(head_num=2, kv_head_num=1, head_size=hs, inter_size=me.INTER, num_layers=1, vocab_size=100, max_seq_len=me.MAX_SEQ, max_batch=me.MAX_BATCH,
               rotary_dim=hs, rotary_base=10000.0, rms_eps=1e-5, dtype=llmie.F32, wfmt=llmie.W_F32, int4_group=128, flags=0, kv_fmt=llmie.KV_NATIVE,
               k_scale=1.0, v_scale=1.0)
    f32 = llmie.Decoder(cfg, [dict(attn_norm=d(lw[0]["attn_norm"]).float(), ffn_norm=d(lw[0]["ffn_norm"]).float(),
                                   **{m: d(lw[0][m]).float() for m in ("qkv", "o", "gate_up", "down")})])
    with pytest.raises(llmie.LlmieError, match="experts need an fp16 engine"):
        f32.moe_attach(me.experts_of(lw, (True,)), k)
    f32.close()


def test_captured_step_follows_the_routing_of_new_rows():
    """fresh process: one decode step captured with torch.cuda.graph; replays on other hidden rows, which route differently, equal
    the eager calls bit for bit"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "moe_capture.py")], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["equal"] == [True, True, True], out
    assert out["routes_differ"] == [True, True], out
