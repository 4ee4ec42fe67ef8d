#!/usr/bin/env python3
"""Token scoring micro-benchmark: llmie.score_tokens (RMSNorm + LM head + log-softmax, logits never written) against the composition
of the older entries -- rmsnorm on a copy + linear into [T, V] fp16 logits + torch.log_softmax(...).gather -- at the Llama-2-7B
LM head (V = 32000, H = 4096), fp16:

    python tools/scorebench.py [--rows 2048 4096] [--rounds 9] [--reps 5] [--out FILE]

Rounds of the two arms are interleaved (A B A B ...) and the median round of each arm is reported, with the TFLOP/s of the
2 * T * V * H product, the peak device memory each arm needs beyond its inputs, and the largest difference of the two arms'
log-probabilities.  Prints one JSON line (and writes it to --out)."""
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
EPS = 1e-5


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def peak_extra(fn):
    """peak device bytes allocated while fn runs, beyond what was allocated before it"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def bench(T, V, H, rounds, reps):
    g = torch.Generator(device="cpu").manual_seed(T)
    hidden = torch.randn((T, H), generator=g).to("cuda").half()
    gamma = (1 + 0.1 * torch.randn(H, generator=g)).to("cuda").half()
    W = (torch.randn((V, H), generator=g) * (1.2 / H ** 0.5)).to("cuda").half()
    targets = torch.randint(0, V, (T,), generator=g).to("cuda").to(torch.int32)
    tgt64 = targets.long().unsqueeze(1)
    ws = torch.empty(llmie.score_tokens_workspace_bytes(T, H, V), dtype=torch.uint8, device="cuda")

    def fused():
        return llmie.score_tokens(hidden, W, targets, gamma=gamma, eps=EPS, workspace=ws)

    def composed():
        xn = hidden.clone()
        llmie.rmsnorm(xn, None, gamma, EPS)
        logits = torch.empty((T, V), dtype=torch.float16, device="cuda")
        llmie.linear(xn, W, logits)
        return torch.log_softmax(logits, dim=-1, dtype=torch.float32).gather(1, tgt64).squeeze(1)

    diff = (fused() - composed()).abs().max().item()   # (also the warm-up of both arms' shapes)
    for _ in range(2):
        fused()
        composed()
    torch.cuda.synchronize()
    tf, tc = [], []
    for _ in range(rounds):
        tf.append(timed(fused, reps))
        tc.append(timed(composed, reps))
    # the fused arm's scratch is the caller's workspace: count it, plus whatever the call allocates beside its [T] output
    mem_f = ws.numel() + peak_extra(fused) - T * 4
    mem_c = peak_extra(composed) - T * 4
    flop = 2.0 * T * V * H
    mf, mc = statistics.median(tf), statistics.median(tc)
    return dict(rows=T, vocab=V, hidden=H, fused_ms=mf * 1e3, composed_ms=mc * 1e3, fused_tflops=flop / mf / 1e12,
                composed_tflops=flop / mc / 1e12, fused_over_composed=mf / mc, fused_ms_min_max=[min(tf) * 1e3, max(tf) * 1e3],
                composed_ms_min_max=[min(tc) * 1e3, max(tc) * 1e3], fused_extra_bytes=int(mem_f), composed_extra_bytes=int(mem_c),
                workspace_bytes=ws.numel(), logits_bytes=T * V * 2, max_abs_logprob_diff=diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[2048, 4096])
    ap.add_argument("--vocab", type=int, default=32000)
    ap.add_argument("--hidden", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scorebench: needs a GPU (a time measured anywhere else says nothing)")
    res = dict(bench="score_tokens", device=torch.cuda.get_device_name(0), rounds=a.rounds, reps=a.reps,
               shapes=[bench(T, a.vocab, a.hidden, a.rounds, a.reps) for T in a.rows])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
