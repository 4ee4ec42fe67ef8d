#!/usr/bin/env python3
"""Multi-LoRA serving: what per-request adapters cost a decode step and a prefill pass, at the Llama-2-7B geometry:

    python tools/lorabench.py [--fmt f16 int8] [--batch 1 8 32] [--ctx 2048] [--prefill 2048] [--rounds 7] [--reps 10] [--out FILE]

Arms, same build, same process, same weights, alternating inside every round (a, b, c, d, e, a, ...); the median round of each arm
is reported with its min and max:
  a  no table attached: today's fused sequences
  b  attached, every row -1: the price of leaving the fused sequences (the unfused decode / general prefill sequence, eight adapter
     launches per layer that exit at once)
  c  every row one rank-16 adapter
  d  every row a different rank-16 adapter (prefill of one sequence: the same as c)
  e  as d at rank 64
b - a is what the lora launch sequence costs before any adapter runs; c - b the eight launches per layer doing their work; d and e
the adapter bytes.  --trace ARM runs one arm alone (a letter a .. e), for a `rocprofv3 --kernel-trace --stats` run of its own
(tools/lorabench.py --trace d after `--`).  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the flagship benchmark's weights and engine construction)

ARMS = ("a_detached", "b_attached_none", "c_one_r16", "d_distinct_r16", "e_distinct_r64")


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps   # ms


def make_adapter(cfg, rank, g):
    """one adapter on all four modules of every layer: A ~ N(0, 1/K), B ~ N(0, 1/rank) / 8"""
    H, I = cfg["head_num"] * cfg["head_size"], cfg["inter_size"]
    QKV = (cfg["head_num"] + 2 * cfg["kv_head_num"]) * cfg["head_size"]
    shapes = dict(qkv=(3, QKV, H), o=(1, H, H), gate_up=(2, 2 * I, H), down=(1, H, I))

    def pair(blocks, N, K):
        A = (torch.randn((blocks * rank, K), generator=g, device="cuda") / K ** 0.5).half()
        B = (torch.randn((N, rank), generator=g, device="cuda") / (8 * rank ** 0.5)).half()
        return A, B
    return [{m: pair(*s) for m, s in shapes.items()} for _ in range(cfg["num_layers"])]


def run_config(llmie, cfg, weights, layers, fmt, rows_kind, B, ctx, rounds, reps, trace=""):
    """rows_kind: 'decode' (B sequences on ctx cached tokens) or 'prefill' (one sequence of B tokens)"""
    decode = rows_kind == "decode"
    H = cfg["head_num"] * cfg["head_size"]
    batch = B if decode else 1
    dec, kc, vc = bench.make_decoder(torch, llmie, cfg, weights, layers, fmt, batch, ctx + 1 if decode else B)
    g = torch.Generator(device="cuda").manual_seed(B)
    x = torch.randn((B, H), generator=g, device="cuda").half()
    y = torch.empty_like(x)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    slots = batch
    tables = {}
    for rank in (16, 64):
        t = llmie.lora_table(slots, cfg["num_layers"])
        for s in range(slots):
            llmie.lora_slot_load(t, s, make_adapter(cfg, rank, g), scale=1.0)
        tables[rank] = t
    seq_slot = i32([-1] * batch)
    ws = torch.empty(dec.lora_workspace_bytes(B, slots), dtype=torch.uint8, device="cuda")
    in_len, hist = i32([B]), i32([0])

    def step():
        if decode:
            dec.forward(x, y, kc, vc, ctx + 1)
        else:
            dec.prefill(x, y, kc, vc, in_len, hist, B)

    def arm(name):
        if name == "a_detached":
            dec.lora_detach()
            return
        dec.lora_attach(tables[64 if name.startswith("e") else 16], seq_slot, max_tokens=B, workspace=ws)
        seq_slot.copy_(i32([-1] * batch if name.startswith("b") else ([0] * batch if name.startswith("c") else list(range(batch)))))

    if trace:
        name = [n for n in ARMS if n.startswith(trace)][0]
        arm(name)
        for _ in range(reps):
            step()
        torch.cuda.synchronize()
        dec.close()
        return dict(traced=name, fmt=fmt, kind=rows_kind, rows=B, reps=reps)
    for name in ARMS:   # every arm warm
        arm(name)
        step()
        step()
    torch.cuda.synchronize()
    t = {name: [] for name in ARMS}
    for _ in range(rounds):
        for name in ARMS:
            arm(name)
            step()   # (the first call behind a switch of sequences is not timed)
            t[name].append(timed(step, reps))
    res = dict(fmt=fmt, kind=rows_kind, rows=B, ctx=ctx if decode else 0,
               plan=dict(detached=llmie.decoder_plan_name(dec.cfg, 0 if decode else 1, B), attached="lora"))
    for name in ARMS:
        res[name + "_ms"] = statistics.median(t[name])
        res[name + "_ms_min_max"] = [min(t[name]), max(t[name])]
    res["b_minus_a_ms"] = res["b_attached_none_ms"] - res["a_detached_ms"]
    res["c_minus_b_ms"] = res["c_one_r16_ms"] - res["b_attached_none_ms"]
    res["d_minus_c_ms"] = res["d_distinct_r16_ms"] - res["c_one_r16_ms"]
    res["e_minus_d_ms"] = res["e_distinct_r64_ms"] - res["d_distinct_r16_ms"]
    res["attached_over_detached"] = res["b_attached_none_ms"] / res["a_detached_ms"]
    dec.close()
    del kc, vc, tables
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fmt", nargs="*", default=["f16", "int8"])
    ap.add_argument("--batch", type=int, nargs="*", default=[1, 8, 32])
    ap.add_argument("--ctx", type=int, default=2048)
    ap.add_argument("--prefill", type=int, nargs="*", default=[2048])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--layers", type=int, default=0, help="fewer layers than the model's 32 (a rehearsal; not a measurement)")
    ap.add_argument("--trace", default="", choices=["", "a", "b", "c", "d", "e"], help="one arm alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lorabench: needs a GPU (a time measured anywhere else says nothing)")
    llmie = bench.load_llmie()
    cfg = dict(bench.LLAMA2_7B)
    if a.layers:
        cfg["num_layers"] = a.layers
    weights = bench.build_weights(torch, cfg, 0)
    results = []
    for fmt in a.fmt:
        layers = weights["layers"] if fmt == "f16" else bench.quantize_layers(torch, llmie, weights["layers"], fmt)
        for B in a.batch:
            results.append(run_config(llmie, cfg, weights, layers, fmt, "decode", B, a.ctx, a.rounds, a.reps, a.trace))
        for T in a.prefill:
            results.append(run_config(llmie, cfg, weights, layers, fmt, "prefill", T, a.ctx, a.rounds, a.reps if a.trace else max(a.reps // 3, 2), a.trace))
        del layers
        torch.cuda.empty_cache()
    res = dict(bench="lora", device=torch.cuda.get_device_name(0), rounds=a.rounds, reps=a.reps, layers=cfg["num_layers"], results=results)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
