"""Per-request adapters in the engine (llmie_decoder_lora_attach): every sequence of a mixed batch must agree with a second
engine, WITHOUT a table, that runs the merged weights fp16(W + scale B A) of the sequence's adapter (the base weights for slot -1;
int8: merge, then quantise both the same way).

Engine: 2 layers, head_num 4 / kv_head_num 2, inter 704, max_seq 384, max_batch 8, fp16 and int8 base; adapters of rank 8 / 16 /
64, the second with q and v only.  head_size: llmie_decoder_prefill takes head_size 128 only (its flash kernel; the entry refuses
anything else with or without a table), so the prefill + decode pipeline runs at head_size 128; the decode entries, which have no
such limit, are also checked at head_size 64.

Bound: relative Frobenius error <= 2e-2 per sequence (conftest.systematic_error), the multi-layer fp16 bar of DESIGN.md section 2;
the adapters are large enough that base and merged engines differ by >= 10 x that, which is asserted, so an engine that ignored its
table could not pass.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from conftest import systematic_error

import lora_engine_cases as lc

pytestmark = pytest.mark.gpu
DEV, F16 = lc.DEV, lc.F16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 2e-2
LENS = (5, 37, 130)            # cross a 16-row tile and a 128-token page
FIRST = (3, 20, 100)           # the two-chunk split: FIRST, then the rest on top of that history
SEQ_SLOTS = ((1, -1, 0), (1, 0, 2))   # the issue's mix; and one that takes the rank-64 adapter through prefill as well
STEPS = 4
_engines = {}


def engines(llmie, hs, int8):
    """(lora engine, its table, its seq_slot, base engine, [merged engine per adapter]) of one format, built once"""
    key = (hs, int8)
    if key not in _engines:
        base, ads = lc.base_weights(hs), lc.adapters(hs)
        lora = lc.lora_engine(llmie, base, ads, hs, int8, max_tokens=sum(LENS))
        _engines[key] = lora + (lc.make_engine(llmie, base, hs, int8), [lc.make_engine(llmie, lc.merged_weights(base, a, hs), hs, int8) for a in ads])
    return _engines[key]


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def pipeline(llmie, dec, hs, paged, two_chunks, x_prefill, x_decode):
    """prefill of the three sequences (one pass, or two chunks with history), then STEPS ragged decode steps; -> per sequence the
    hidden rows of everything it produced, in order"""
    bs, L = len(LENS), lc.LAYERS
    if paged:
        max_pages = (lc.MAX_SEQ + 127) // 128
        num_pages = bs * max_pages + 2
        table = torch.from_numpy(np.random.default_rng(1).permutation(num_pages)[:bs * max_pages].astype(np.int32)).reshape(bs, max_pages).to(DEV)
        k = torch.zeros((L, num_pages, lc.KVH, 128, hs), dtype=F16, device=DEV)
    else:
        k = torch.zeros((L, bs, lc.KVH, lc.MAX_SEQ, hs), dtype=F16, device=DEV)
    v = torch.zeros_like(k)
    start = np.concatenate([[0], np.cumsum(LENS)])
    chunks = [(FIRST, (0, 0, 0)), (tuple(n - f for n, f in zip(LENS, FIRST)), FIRST)] if two_chunks else [(LENS, (0, 0, 0))]
    out = [[] for _ in range(bs)]
    for lens, hist in chunks:
        x = torch.cat([x_prefill[start[b] + hist[b]:start[b] + hist[b] + lens[b]] for b in range(bs)]).contiguous()
        y = torch.empty_like(x)
        if paged:
            dec.prefill_paged(x, y, k, v, table, i32(lens), i32(hist), max(lens))
        else:
            dec.prefill(x, y, k, v, i32(lens), i32(hist), max(lens))
        c0 = np.concatenate([[0], np.cumsum(lens)])
        for b in range(bs):
            out[b].append(y[c0[b]:c0[b + 1]].float().cpu().numpy())
    for i in range(STEPS):
        ctx = i32(n + 1 + i for n in LENS)
        y = torch.empty_like(x_decode[i])
        if paged:
            dec.forward_paged_ragged(x_decode[i], y, k, v, table, ctx)
        else:
            dec.forward_ragged(x_decode[i], y, k, v, ctx)
        for b in range(bs):
            out[b].append(y[b:b + 1].float().cpu().numpy())
    torch.cuda.synchronize()
    return [np.concatenate(o) for o in out]


@pytest.mark.parametrize("seq_slots", SEQ_SLOTS, ids=["mix_1_none_0", "mix_1_0_2"])
@pytest.mark.parametrize("two_chunks", [False, True], ids=["one_pass", "two_chunks"])
@pytest.mark.parametrize("paged", [False, True], ids=["dense", "paged"])
@pytest.mark.parametrize("int8", [False, True], ids=["f16", "int8"])
def test_mixed_batch_agrees_with_merged_engines(llmie, int8, paged, two_chunks, seq_slots):
    hs = 128
    dec, table, seq_slot, base, merged = engines(llmie, hs, int8)
    g = torch.Generator().manual_seed(3)
    H = lc.NH * hs
    xp = torch.randn((sum(LENS), H), generator=g).to(DEV).to(F16)
    xd = [torch.randn((len(LENS), H), generator=g).to(DEV).to(F16) for _ in range(STEPS)]
    seq_slot[:3] = i32(seq_slots)
    got = pipeline(llmie, dec, hs, paged, two_chunks, xp, xd)
    base_out = pipeline(llmie, base, hs, paged, two_chunks, xp, xd)
    for b, s in enumerate(seq_slots):
        want = base_out[b] if s < 0 else pipeline(llmie, merged[s], hs, paged, two_chunks, xp, xd)[b]
        fro, proj = systematic_error(got[b], want)
        print("int8=%d paged=%d two_chunks=%d sequence %d slot %d: fro %.4f proj %.4f" % (int8, paged, two_chunks, b, s, fro, proj))
        assert fro <= BAR, (b, s, fro)
        if s >= 0:
            apart, _ = systematic_error(base_out[b], want)
            assert apart >= 10 * BAR, (b, s, apart)
    # (ii) the rows of a sequence without an adapter do not depend on the adapters beside them
    seq_slot[:3] = -1
    alone = pipeline(llmie, dec, hs, paged, two_chunks, xp, xd)
    for b, s in enumerate(seq_slots):
        assert np.array_equal(alone[b], got[b]) == (s < 0), (b, s)


@pytest.mark.parametrize("paged", [False, True], ids=["dense", "paged"])
@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("int8", [False, True], ids=["f16", "int8"])
def test_uniform_decode_agrees_with_merged_engines(llmie, int8, hs, paged):
    """llmie_decoder_forward / _forward_paged: one step index for the batch, on caches every engine shares"""
    dec, table, seq_slot, base, merged = engines(llmie, hs, int8)
    slots, step, bs, L = (1, -1, 0, 2), 131, 4, lc.LAYERS
    g = torch.Generator().manual_seed(4)
    kd = (torch.randn((L, bs, lc.KVH, lc.MAX_SEQ, hs), generator=g) * 0.5).to(DEV).to(F16)
    vd = (torch.randn((L, bs, lc.KVH, lc.MAX_SEQ, hs), generator=g) * 0.5).to(DEV).to(F16)
    x = torch.randn((bs, lc.NH * hs), generator=g).to(DEV).to(F16)
    max_pages = (lc.MAX_SEQ + 127) // 128
    bt = torch.arange(bs * max_pages, dtype=torch.int32, device=DEV).flip(0).reshape(bs, max_pages).contiguous()

    def run(e):
        if not paged:
            return e.forward(x, torch.empty_like(x), kd.clone(), vd.clone(), step).float().cpu().numpy()
        kp = torch.zeros((L, bs * max_pages, lc.KVH, 128, hs), dtype=F16, device=DEV)
        vp = torch.zeros_like(kp)
        ctx = torch.full((bs,), step - 1, dtype=torch.int32, device=DEV)
        llmie.kv_pages_copy(kd, kp, bt, ctx, True)
        llmie.kv_pages_copy(vd, vp, bt, ctx, True)
        return e.forward_paged(x, torch.empty_like(x), kp, vp, bt, step).float().cpu().numpy()

    seq_slot[:4] = i32(slots)
    got, base_out = run(dec), run(base)
    for b, s in enumerate(slots):
        want = base_out if s < 0 else run(merged[s])
        fro, _ = systematic_error(got[b], want[b])
        print("int8=%d hs=%d paged=%d row %d slot %d: fro %.4f" % (int8, hs, paged, b, s, fro))
        assert fro <= BAR, (b, s, fro)
        if s >= 0:
            assert systematic_error(base_out[b], want[b])[0] >= 10 * BAR
    seq_slot[:4] = -1
    assert np.array_equal(run(dec)[1], got[1])
    # an empty slot and a slot outside the table behave as -1
    seq_slot[:4] = i32((3, 3, 99, -5))
    assert np.array_equal(run(dec), run(dec)) and np.array_equal(run(dec)[1], got[1])


@pytest.mark.parametrize("int8", [False, True], ids=["f16", "int8"])
def test_detach_restores_the_previous_sequences(llmie, int8):
    """(iv) after llmie_decoder_lora_detach the next calls equal the never-attached engine bit for bit"""
    hs = 128
    base_w, ads = lc.base_weights(hs), lc.adapters(hs)
    dec, table, seq_slot = lc.lora_engine(llmie, base_w, ads, hs, int8, max_tokens=sum(LENS))
    base = engines(llmie, hs, int8)[3]
    g = torch.Generator().manual_seed(6)
    H = lc.NH * hs
    xp = torch.randn((sum(LENS), H), generator=g).to(DEV).to(F16)
    xd = [torch.randn((len(LENS), H), generator=g).to(DEV).to(F16) for _ in range(STEPS)]
    seq_slot[:3] = i32(SEQ_SLOTS[0])
    attached = pipeline(llmie, dec, hs, False, False, xp, xd)
    dec.lora_detach()
    detached = pipeline(llmie, dec, hs, False, False, xp, xd)
    want = pipeline(llmie, base, hs, False, False, xp, xd)
    for b in range(3):
        assert np.array_equal(detached[b], want[b])
    assert not np.array_equal(attached[0], want[0])
    dec.close()


@pytest.mark.parametrize("int8", [False, True], ids=["f16", "int8"])
def test_fp8_kv_cache_under_the_lora_sequence(llmie, int8):
    """the lora decode sequence on an e4m3 KV cache (the planner admits it where the geometry has the fused attention kernel): every
    row against its merged engine on the same cache bytes"""
    hs, bs, step, L = 128, 4, 131, lc.LAYERS
    base_w, ads = lc.base_weights(hs), lc.adapters(hs)
    dec, table, seq_slot = lc.lora_engine(llmie, base_w, ads, hs, int8, max_tokens=lc.MAX_BATCH, kv8=True)
    refs = [lc.make_engine(llmie, base_w, hs, int8, kv8=True)] + [lc.make_engine(llmie, lc.merged_weights(base_w, a, hs), hs, int8, kv8=True) for a in ads]
    g = torch.Generator().manual_seed(12)
    kd = torch.randint(0, 0x58, (L, bs, lc.KVH, lc.MAX_SEQ, hs), generator=g, dtype=torch.uint8).to(DEV)
    vd = torch.randint(0, 0x58, (L, bs, lc.KVH, lc.MAX_SEQ, hs), generator=g, dtype=torch.uint8).to(DEV)
    x = torch.randn((bs, lc.NH * hs), generator=g).to(DEV).to(F16)
    run = lambda e: e.forward(x, torch.empty_like(x), kd.clone(), vd.clone(), step).float().cpu().numpy()
    slots = (1, -1, 0, 2)
    seq_slot[:4] = i32(slots)
    got, base_out = run(dec), run(refs[0])
    for b, s in enumerate(slots):
        want = run(refs[s + 1])
        fro, _ = systematic_error(got[b], want[b])
        print("fp8 kv int8=%d row %d slot %d: fro %.4f" % (int8, b, s, fro))
        assert fro <= BAR, (b, s, fro)
        if s >= 0:   # (random cache bytes of full e4m3 range drown more of the adapters than a real cache: an engine that ignored its
            #  table would still miss the bar three times over)
            assert systematic_error(base_out[b], want[b])[0] >= 3 * BAR
    for e in [dec] + refs:
        e.close()


UNSUPPORTED, WORKSPACE = -2, -4


def _attach(llmie, dec, table_ptr, slots, seq_slot, ws, ws_bytes):
    rc = llmie.lib().llmie_decoder_lora_attach(dec.handle, table_ptr, slots, seq_slot.data_ptr(), ws, ws_bytes)
    return rc, llmie.lib().llmie_last_error().decode()


def test_attach_refusals(llmie):
    """llmie_decoder_lora_attach on engines the header excludes, with too many slots, with a short or misaligned workspace: each with
    its code and its message; and an engine that refused stays on its own sequences"""
    hs = 128
    base_w = lc.base_weights(hs)
    table = llmie.lora_table(4, lc.LAYERS)
    seq_slot = torch.full((lc.MAX_BATCH,), -1, dtype=torch.int32, device=DEV)
    ws = torch.empty(llmie.lora_workspace_bytes(lc.MAX_BATCH, 4) + 256, dtype=torch.uint8, device=DEV)
    for kw, word in ((dict(fmt="fp8"), "fp8-weight engine"), (dict(flags=llmie.DEC_PACKED_ONLY), "LLMIE_DEC_PACKED_ONLY"),
                     (dict(int8=True, flags=llmie.DEC_PACKED_ONLY), "LLMIE_DEC_PACKED_ONLY"), (dict(fmt="f32"), "fp16 engine")):
        dec = lc.make_engine(llmie, base_w, hs, kw.pop("int8", False), **kw)
        rc, err = _attach(llmie, dec, table.data.data_ptr(), 4, seq_slot, ws.data_ptr(), ws.numel())
        assert rc == UNSUPPORTED and err.startswith("decoder_lora_attach: adapters need an fp16 engine") and word in err, (kw, rc, err)
        with pytest.raises(llmie.LlmieError, match="decoder_lora_attach"):
            dec.lora_attach(table, seq_slot)
        if kw.get("flags"):   # still the engine it was: a decode step runs on its own (packed) sequence
            x = torch.randn((2, lc.NH * hs), device=DEV).to(F16)
            k = torch.zeros((lc.LAYERS, 2, lc.KVH, lc.MAX_SEQ, hs), dtype=F16, device=DEV)
            dec.forward(x, torch.empty_like(x), k, k.clone(), 3)
            torch.cuda.synchronize()
        dec.close()
    dec = lc.make_engine(llmie, base_w, hs, False)
    need = dec.lora_workspace_bytes(lc.MAX_BATCH, 4)
    assert need == llmie.lora_workspace_bytes(lc.MAX_BATCH, 4, 192)
    rc, err = _attach(llmie, dec, table.data.data_ptr(), llmie.LORA_MAX_SLOTS + 1, seq_slot, ws.data_ptr(), ws.numel())
    assert rc == UNSUPPORTED and "LLMIE_LORA_MAX_SLOTS" in err, err
    rc, err = _attach(llmie, dec, table.data.data_ptr(), 4, seq_slot, ws.data_ptr(), need - 1)
    assert rc == WORKSPACE and err.startswith("decoder_lora_attach: workspace") and str(need) in err, err
    rc, err = _attach(llmie, dec, table.data.data_ptr(), 4, seq_slot, ws.data_ptr() + 16, need)
    assert rc == WORKSPACE and "256-byte aligned" in err, err
    rc, err = _attach(llmie, dec, None, 4, seq_slot, ws.data_ptr(), need)
    assert rc == -1 and "NULL pointer" in err
    rc, err = _attach(llmie, dec, table.data.data_ptr(), 4, seq_slot, ws.data_ptr(), need)
    assert rc == 0, err
    dec.close()


def test_a_call_with_more_rows_than_the_attach_workspace_covers_is_refused(llmie):
    """attached with scratch for max_batch rows: a prefill of more tokens is LLMIE_ERR_WORKSPACE before anything runs, and decode goes on"""
    hs = 128
    dec, table, seq_slot = lc.lora_engine(llmie, lc.base_weights(hs), lc.adapters(hs), hs, False, max_tokens=lc.MAX_BATCH)
    T = 40
    x = torch.randn((T, lc.NH * hs), device=DEV).to(F16)
    y = torch.zeros_like(x)
    k = torch.zeros((lc.LAYERS, 1, lc.KVH, lc.MAX_SEQ, hs), dtype=F16, device=DEV)
    v = torch.zeros_like(k)
    seq_slot[:1] = 0
    with pytest.raises(llmie.LlmieError) as e:
        dec.prefill(x, y, k, v, i32([T]), i32([0]), T)
    assert "(-4)" in str(e.value) and "decoder_prefill: the adapter workspace" in str(e.value) and "does not cover 40 rows" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert int(k.abs().sum().item()) == 0 and int(y.abs().sum().item()) == 0   # nothing was enqueued
    dec.prefill(x[:8], y[:8], k, v, i32([8]), i32([0]), 8)   # what the scratch covers runs
    dec.forward(x[:1], y[:1], k, v, 9)
    torch.cuda.synchronize()
    assert float(y[:1].float().abs().sum().item()) > 0
    dec.close()


def test_python_slot_loader_checks(llmie):
    """lora_slot_load: a missing block of a fused module and modules of different rank are errors, not silent mis-stacking; emptying
    a slot over and over keeps one generation of tensors alive, not all of them"""
    table = llmie.lora_table(2, 1)
    t = lambda *shape: torch.zeros(shape, dtype=F16, device=DEV)
    with pytest.raises(llmie.LlmieError, match="every block"):
        llmie.lora_slot_load(table, 0, [dict(k=(t(8, 64), t(16, 8)), v=(t(8, 64), t(16, 8)))])
    with pytest.raises(llmie.LlmieError, match="rank 16"):
        llmie.lora_slot_load(table, 0, [dict(o=(t(8, 64), t(64, 8)), down=(t(16, 64), t(64, 16)))])
    llmie.lora_slot_load(table, 0, [dict(q=(t(8, 64), t(32, 8)), k=(t(8, 64), t(16, 8)), v=(t(8, 64), t(16, 8)))])
    a, b = table.keep[0][1][0]
    assert a.shape == (24, 64) and b.shape == (64, 8)
    for _ in range(5):
        llmie.lora_slot_load(table, 0, None)
    depth, node = 0, table.keep[0]
    while isinstance(node, tuple):
        depth, node = depth + 1, node[0]
    assert depth == 1, table.keep[0]
    torch.cuda.synchronize()


def test_captured_step_follows_the_device_arrays():
    """(iii) fresh process: one decode step captured with torch.cuda.graph; replays after rewriting seq_slot and after loading another
    adapter into a live slot equal the eager calls bit for bit"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lora_capture.py")], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["equal"] == [True, True, True], out
    assert out["distinct"] == [True, True], out


def test_lora_cpp_driver():
    """(v) the C++ driver of launchLoraApply"""
    bin_dir = os.path.join(ROOT, "llm-inference-engine_amd", "cpp_tests")
    path = os.path.join(bin_dir, "test_lora_api")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", bin_dir, "test_lora_api"])
    r = subprocess.run([path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "all passed" in r.stdout and "FAIL" not in r.stdout
    for what in ("LoraApply adapted rows", "LoraApply untouched rows", "LlamaModel slot -1 agrees with the base model",
                 "LlamaModel loaded slot moves the hidden rows", "LlamaModel same adapter in another slot, prefill",
                 "LlamaModel same adapter in another slot, decode", "LlamaModel emptied slot, prefill", "LlamaModel emptied slot, decode",
                 "LlamaModel without the fused engine refuses adapters"):
        assert what + " passed" in r.stdout, r.stdout[-3000:]
