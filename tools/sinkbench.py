#!/usr/bin/env python3
"""Attention with a learned sink logit per query head against attention without, at Llama-2-7B shapes (32 heads = 32 KV heads, head
size 128, hidden 4096, inter 11008, fp16), same process, interleaved rounds, medians:

    python tools/sinkbench.py [--ctxs 2048 32768] [--batches 1 8] [--prefill 2048] [--rounds 7] [--reps 10] [--out FILE]
    python tools/sinkbench.py --headline [--lib PATH] [--layers 32] [--ctx 2048] [--prefill 2048]

  attn      one decode attention layer (llmie_decoder_mha_sink, device-resident context lengths, separate merge kernel) per batch and
            context: head_sink = NULL (the launch llmie_decoder_mha_window makes), a sink array, and -- once -- the in-launch merge
  prefill   the attention launches (the engine's MHA op timer) of a 2-layer prefill of 1 x --prefill tokens, with head sinks / without
  headline  WITHOUT sinks: a whole batch-1 decode step of an engine of --layers layers at context --ctx (Decoder.forward) and its
            prefill of 1 x --prefill tokens.  --lib loads another build of the library (entries it lacks are dropped from the binding),
            so that two builds can be compared in alternating processes: the instantiations that existed before must not have moved

Prints one JSON line (and writes it to --out).  Caches and weights are uninitialised or random memory: only time is measured."""
import argparse
import ctypes
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


def bench_attn(batch, ctx, rounds, reps):
    qkv = torch.randn((batch, NH + 2 * KVH, HS), device="cuda").to(F16)
    kc = torch.zeros((1, batch, KVH, ctx, HS), dtype=F16, device="cuda")
    vc = torch.zeros_like(kc)
    out = torch.empty((batch, H), dtype=F16, device="cuda")
    ws = torch.empty(llmie.decoder_mha_workspace_bytes(batch, NH, HS, ctx), dtype=torch.uint8, device="cuda")
    lengths = torch.full((batch,), ctx, dtype=torch.int32, device="cuda")
    sink = torch.randn(NH, device="cuda")
    tickets = torch.zeros(batch * KVH, dtype=torch.int32, device="cuda")
    call = lambda s, t=None: llmie.decoder_mha_sink(qkv, None, kc, vc, out, 0, NH, KVH, lengths, ws, None, 0, ctx, s, tickets=t)
    t = interleaved({"plain": lambda: call(None), "sink": lambda: call(sink), "plain_tickets": lambda: call(None, tickets),
                     "sink_tickets": lambda: call(sink, tickets)}, rounds, reps)
    return dict(batch=batch, ctx=ctx, us={k: round(v * 1e6, 2) for k, v in t.items()})


def _engine(layers, max_seq, max_batch):
    w = lambda n, k: dict(data=(torch.randn((n, k), device="cuda") * (1.0 / k ** 0.5)).to(F16))
    lw = [dict(attn_norm=torch.ones(H, dtype=F16, device="cuda"), ffn_norm=torch.ones(H, dtype=F16, device="cuda"), qkv=w((NH + 2 * KVH) * HS, H),
               o=w(H, H), gate_up=w(2 * INTER, H), down=w(H, INTER)) for _ in range(layers)]
    cfg = dict(head_num=NH, kv_head_num=KVH, head_size=HS, inter_size=INTER, num_layers=layers, vocab_size=32000, max_seq_len=max_seq,
               max_batch=max_batch, rotary_dim=HS, rotary_base=10000.0, rms_eps=1e-5, dtype=llmie.F16, wfmt=llmie.W_F16, int4_group=128)
    return llmie.Decoder(cfg, lw), lw


def bench_prefill(tokens, rounds):
    layers = 2
    dec, keep = _engine(layers, tokens, 1)
    kc = torch.zeros((layers, 1, KVH, tokens, HS), dtype=F16, device="cuda")
    vc = torch.zeros_like(kc)
    x = torch.randn((tokens, H), device="cuda").to(F16)
    y = torch.empty_like(x)
    lens, hist = torch.tensor([tokens], dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    sinks = torch.randn((layers, NH), device="cuda")
    res = {"plain": [], "sink": []}
    try:
        for _ in range(rounds + 2):   # (the first two rounds = warm-up)
            for name, s in (("plain", None), ("sink", sinks)):
                dec.set_head_sinks(s)
                dec.profile_begin(64)
                dec.prefill(x, y, kc, vc, lens, hist, tokens)
                ms, n = dec.profile_end()["mha"]
                res[name].append(ms / max(n, 1))
    finally:
        dec.set_head_sinks(None)
        dec.close()
    return dict(tokens=tokens, mha_us_per_layer={k: round(statistics.median(v[2:]) * 1e3, 1) for k, v in res.items()})


def bench_headline(layers, ctx, tokens, rounds, reps):
    max_seq = max(ctx, tokens)
    dec, keep = _engine(layers, max_seq, 1)
    kc = torch.zeros((layers, 1, KVH, max_seq, HS), dtype=F16, device="cuda")
    vc = torch.zeros_like(kc)
    x1 = torch.randn((1, H), device="cuda").to(F16)
    y1 = torch.empty_like(x1)
    xp = torch.randn((tokens, H), device="cuda").to(F16)
    yp = torch.empty_like(xp)
    lens, hist = torch.tensor([tokens], dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    try:
        t = interleaved({"decode_step": lambda: dec.forward(x1, y1, kc, vc, ctx), "prefill": lambda: dec.prefill(xp, yp, kc, vc, lens, hist, tokens)},
                        rounds, reps)
    finally:
        dec.close()
    return dict(layers=layers, ctx=ctx, prefill_tokens=tokens, ms={k: round(v * 1e3, 4) for k, v in t.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ctxs", type=int, nargs="+", default=[2048, 32768])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--prefill", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--headline", action="store_true")
    ap.add_argument("--lib")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--ctx", type=int, default=2048)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.lib:   # another build: bind what it has (torch, imported above, has loaded its HIP runtime first, as llmie.lib() wants)
        llmie.LIB_PATH = os.path.abspath(a.lib)
        probe = ctypes.CDLL(llmie.LIB_PATH)
        for name in [n for n in llmie._SIGS if not hasattr(probe, n)]:
            del llmie._SIGS[name]
    res = dict(tool="sinkbench", device=torch.cuda.get_device_name(0), lib=a.lib or "in-tree")
    if a.headline:
        res["headline"] = bench_headline(a.layers, a.ctx, a.prefill, a.rounds, a.reps)
    else:
        res["attn"] = [bench_attn(b, c, a.rounds, a.reps) for c in a.ctxs for b in a.batches]
        res["prefill"] = bench_prefill(a.prefill, a.rounds)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
