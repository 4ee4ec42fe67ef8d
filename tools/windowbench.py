#!/usr/bin/env python3
"""Sliding-window attention against full attention at Llama-2-7B shapes (32 heads = 32 KV heads, head size 128, hidden 4096, inter
11008, fp16), same process, interleaved rounds, medians:

    python tools/windowbench.py [--ctx 32768] [--window 4096] [--sinks 4] [--batches 1 8] [--layers 32] [--prefill 8192]
                                [--rounds 7] [--reps 10] [--skip-step] [--out FILE]

  attn     one decode attention layer (llmie_decoder_mha_window, device-resident context lengths, separate merge kernel) at the context,
           with the window and without; next to it the same call at a context of `window` tokens, which is what a windowed layer should cost
  step     a whole decode step of an engine of --layers layers (Decoder.forward_ragged) at the context, every layer windowed / none
  prefill  the attention launches (the engine's MHA op timer) of a 2-layer prefill of 1 x --prefill tokens, windowed / full
  copy     a plain device copy of 1 GiB in the same process (read + write counted)

Prints one JSON line (and writes it to --out).  Caches and weights are uninitialised or random memory: only time is measured."""
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
NH, KVH, HS, INTER = 32, 32, 128, 11008
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


def copy_rate(rounds):
    a = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    b.copy_(a)
    torch.cuda.synchronize()
    t = statistics.median(timed(lambda: b.copy_(a), 3) for _ in range(rounds))
    return 2.0 * (1 << 30) / t


def bench_attn(batch, ctx, window, sinks, rounds, reps):
    max_seq = ctx
    qkv = torch.randn((batch, NH + 2 * KVH, HS), device="cuda").to(F16)
    kc = torch.zeros((1, batch, KVH, max_seq, HS), dtype=F16, device="cuda")
    vc = torch.zeros_like(kc)
    out = torch.empty((batch, H), dtype=F16, device="cuda")
    ws = torch.empty(llmie.decoder_mha_workspace_bytes(batch, NH, HS, max_seq), dtype=torch.uint8, device="cuda")
    long_ctx = torch.full((batch,), ctx, dtype=torch.int32, device="cuda")
    short_ctx = torch.full((batch,), min(window, ctx), dtype=torch.int32, device="cuda")
    call = lambda lengths, w, s: llmie.decoder_mha_window(qkv, None, kc, vc, out, 0, NH, KVH, lengths, ws, None, 0, max_seq, w, s)
    t = interleaved({"full": lambda: call(long_ctx, 0, 0), "window": lambda: call(long_ctx, window, sinks),
                     "full_at_window_ctx": lambda: call(short_ctx, 0, 0)}, rounds, reps)
    kv_bytes = 2.0 * batch * KVH * HS * 2
    return dict(batch=batch, us={k: round(v * 1e6, 2) for k, v in t.items()},
                tb_per_s={"full": round(kv_bytes * ctx / t["full"] / 1e12, 3), "window": round(kv_bytes * (window + sinks) / t["window"] / 1e12, 3)})


def _engine(layers, max_seq, max_batch):
    w = lambda n, k: dict(data=(torch.randn((n, k), device="cuda") * (1.0 / k ** 0.5)).to(F16))
    lw = [dict(attn_norm=torch.ones(H, dtype=F16, device="cuda"), ffn_norm=torch.ones(H, dtype=F16, device="cuda"), qkv=w((NH + 2 * KVH) * HS, H),
               o=w(H, H), gate_up=w(2 * INTER, H), down=w(H, INTER)) for _ in range(layers)]
    cfg = dict(head_num=NH, kv_head_num=KVH, head_size=HS, inter_size=INTER, num_layers=layers, vocab_size=32000, max_seq_len=max_seq,
               max_batch=max_batch, rotary_dim=HS, rotary_base=10000.0, rms_eps=1e-5, dtype=llmie.F16, wfmt=llmie.W_F16, int4_group=128)
    return llmie.Decoder(cfg, lw), lw


def bench_step(batch, layers, ctx, window, sinks, rounds, reps):
    dec, keep = _engine(layers, ctx, batch)
    kc = torch.empty((layers, batch, KVH, ctx, HS), dtype=F16, device="cuda")
    vc = torch.empty_like(kc)
    x = torch.randn((batch, H), device="cuda").to(F16)
    y = torch.empty_like(x)
    lengths = torch.full((batch,), ctx, dtype=torch.int32, device="cuda")
    out = {"full": [], "window": []}
    try:
        for _ in range(rounds):   # (set_window is host state: one arm at a time, alternated within every round)
            for name, win in (("full", None), ("window", [window] * layers)):
                dec.set_window(win, sinks if win else 0)
                dec.forward_ragged(x, y, kc, vc, lengths)
                torch.cuda.synchronize()
                out[name].append(timed(lambda: dec.forward_ragged(x, y, kc, vc, lengths), reps))
    finally:
        dec.set_window(None)
        dec.close()
    return dict(batch=batch, layers=layers, ms={k: round(statistics.median(v) * 1e3, 4) for k, v in out.items()})


def bench_prefill(tokens, window, sinks, rounds):
    layers = 2
    dec, keep = _engine(layers, tokens, 1)
    kc = torch.zeros((layers, 1, KVH, tokens, HS), dtype=F16, device="cuda")
    vc = torch.zeros_like(kc)
    x = torch.randn((tokens, H), device="cuda").to(F16)
    y = torch.empty_like(x)
    lens, hist = torch.tensor([tokens], dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    res = {"full": [], "window": []}
    try:
        for _ in range(rounds + 1):   # (first round = warm-up)
            for name, win in (("full", None), ("window", [window] * layers)):
                dec.set_window(win, sinks if win else 0)
                dec.profile_begin(64)
                dec.prefill(x, y, kc, vc, lens, hist, tokens)
                ms, n = dec.profile_end()["mha"]
                res[name].append(ms / max(n, 1))
    finally:
        dec.set_window(None)
        dec.close()
    return dict(tokens=tokens, mha_us_per_layer={k: round(statistics.median(v[2:]) * 1e3, 1) for k, v in res.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ctx", type=int, default=32768)
    ap.add_argument("--window", type=int, default=4096)
    ap.add_argument("--sinks", type=int, default=4)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--prefill", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    res = dict(tool="windowbench", ctx=a.ctx, window=a.window, sinks=a.sinks, device=torch.cuda.get_device_name(0))
    res["copy_tb_per_s"] = round(copy_rate(a.rounds) / 1e12, 3)
    res["attn"] = [bench_attn(b, a.ctx, a.window, a.sinks, a.rounds, a.reps) for b in a.batches]
    if not a.skip_step:
        res["step"] = [bench_step(b, a.layers, a.ctx, a.window, a.sinks, a.rounds, max(2, a.reps // 2)) for b in a.batches]
    res["prefill"] = bench_prefill(a.prefill, a.window, a.sinks, a.rounds)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
