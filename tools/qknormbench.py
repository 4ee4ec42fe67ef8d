#!/usr/bin/env python3
"""What QK-norm costs, at Qwen3 shapes (32 query heads over 8 and over 4 KV heads, head size 128, fp16 cache), same process, interleaved
rounds, medians:

    python tools/qknormbench.py [--ctx 2048] [--batches 1 32] [--prefill 2048] [--rounds 7] [--reps 10] [--out FILE]

  attn      one decode attention layer (device-resident context lengths, fused RoPE, separate merge kernel) per batch and KV-head
            count: `plain` = llmie_decoder_mha_sink without gammas, `qknorm` = llmie_decoder_mha_qknorm (the QKN instantiation),
            `composed` = llmie_qk_norm followed by the plain launch (what a per-kernel path pays)
  prefill   a 2-layer engine's prefill of 1 x --prefill tokens per layer, without QK-norm (RoPE + append in the QKV projection's
            epilogue) and with it (plain projection, then the RoPE + append launch, which normalises): the cost of not having the norm
            in the GEMM epilogues

Prints one JSON line (and writes it to --out).  Caches and weights are zero or random memory: only time is measured."""
import argparse
import importlib.util
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("llmie_amd", os.path.join(ROOT, "llm-inference-engine_amd", "__init__.py"))
llmie = importlib.util.module_from_spec(spec)
sys.modules["llmie_amd"] = llmie
spec.loader.exec_module(llmie)
NH, HS, INTER = 32, 128, 11008
H = NH * HS
F16 = torch.float16


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def interleaved(arms, rounds, reps):
    """{name: median seconds per call}; a round runs every arm once, in turn"""
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            times[k].append(timed(fn, reps))
    return {k: statistics.median(v) for k, v in times.items()}


def bench_attn(batch, kvh, ctx, rounds, reps):
    qkv = torch.randn((batch, NH + 2 * kvh, HS), device="cuda").to(F16)
    scratch = qkv.clone()
    kc = torch.zeros((1, batch, kvh, ctx, HS), dtype=F16, device="cuda")
    vc = torch.zeros_like(kc)
    out = torch.empty((batch, H), dtype=F16, device="cuda")
    ws = torch.empty(llmie.decoder_mha_workspace_bytes(batch, NH, HS, ctx), dtype=torch.uint8, device="cuda")
    lengths = torch.full((batch,), ctx, dtype=torch.int32, device="cuda")
    tab = torch.from_numpy(llmie.rope_table(ctx, HS, HS, 10000.0)).cuda()
    qg, kg = torch.ones(HS, dtype=F16, device="cuda"), torch.ones(HS, dtype=F16, device="cuda")
    plain = lambda x=qkv: llmie.decoder_mha_sink(x, None, kc, vc, out, 0, NH, kvh, lengths, ws, tab, HS, ctx, None)
    fused = lambda: llmie.decoder_mha_qknorm(qkv, None, kc, vc, out, 0, NH, kvh, lengths, ws, tab, HS, ctx, qg, kg, 1e-6)

    def composed():
        llmie.qk_norm(scratch, NH, kvh, qg, kg, 1e-6)
        plain(scratch)
    t = interleaved({"plain": plain, "qknorm": fused, "composed": composed}, rounds, reps)
    return dict(batch=batch, kv_heads=kvh, ctx=ctx, us={k: round(v * 1e6, 2) for k, v in t.items()})


def bench_prefill(tokens, kvh, rounds):
    layers = 2
    w = lambda n, k: dict(data=(torch.randn((n, k), device="cuda") * (1.0 / k ** 0.5)).to(F16))
    lw = [dict(attn_norm=torch.ones(H, dtype=F16, device="cuda"), ffn_norm=torch.ones(H, dtype=F16, device="cuda"), qkv=w((NH + 2 * kvh) * HS, H),
               o=w(H, H), gate_up=w(2 * INTER, H), down=w(H, INTER)) for _ in range(layers)]
    cfg = dict(head_num=NH, kv_head_num=kvh, head_size=HS, inter_size=INTER, num_layers=layers, vocab_size=32000, max_seq_len=tokens,
               max_batch=1, rotary_dim=HS, rotary_base=10000.0, rms_eps=1e-6, dtype=llmie.F16, wfmt=llmie.W_F16, int4_group=128)
    dec = llmie.Decoder(cfg, lw)
    kc = torch.zeros((layers, 1, kvh, tokens, HS), dtype=F16, device="cuda")
    vc = torch.zeros_like(kc)
    x = torch.randn((tokens, H), device="cuda").to(F16)
    y = torch.empty_like(x)
    lens, hist = torch.tensor([tokens], dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    qg, kg = torch.ones((layers, HS), dtype=F16, device="cuda"), torch.ones((layers, HS), dtype=F16, device="cuda")
    plans = {}
    res = {"plain": [], "qknorm": []}
    try:
        for name, flag in (("plain", 0), ("qknorm", llmie.PLAN_QK_NORM)):
            plans[name] = llmie.decoder_prefill_layer_plan(cfg, tokens, 1, tokens, call_flags=flag)[0]
        for r in range(rounds + 2):   # (the first two rounds = warm-up)
            for name, g in (("plain", (None, None)), ("qknorm", (qg, kg))):
                dec.set_qk_norm(g[0], g[1], 1e-6)
                res[name].append(timed(lambda: dec.prefill(x, y, kc, vc, lens, hist, tokens), 3) / layers)
    finally:
        dec.set_qk_norm(None, None)
        dec.close()
    return dict(tokens=tokens, kv_heads=kvh, us_per_layer={k: round(statistics.median(v[2:]) * 1e6, 1) for k, v in res.items()}, plans=plans)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ctx", type=int, default=2048)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--kv-heads", type=int, nargs="+", default=[8, 4])
    ap.add_argument("--prefill", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    res = dict(tool="qknormbench", device=torch.cuda.get_device_name(0))
    res["attn"] = [bench_attn(b, kvh, a.ctx, a.rounds, a.reps) for kvh in a.kv_heads for b in a.batches]
    res["prefill"] = [bench_prefill(a.prefill, kvh, a.rounds) for kvh in a.kv_heads[:1]]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
