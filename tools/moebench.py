#!/usr/bin/env python3
"""Mixture-of-experts FFN: llmie_moe_ffn against the dense FFN launches of the same weight bytes, at the Mixtral-8x7B layer shape
(H = 4096, Ie = 14336, E = 8, k = 2):

    python tools/moebench.py [--decode 1 2 3 4 5 6 8 12 16] [--prefill 128 512 2048] [--rounds 7] [--reps 20] [--mxfp4] [--out FILE]

Arms, same process, same weights, alternating inside every round; the median round of each arm is reported with its min and max.
  decode rows R (1 .. 16):  gemv     llmie_moe_ffn under LLMIE_MOE_FORCE_GEMV
                            grouped  llmie_moe_ffn under LLMIE_MOE_FORCE_GROUPED
                            dense    k sequential dense FFNs of the expert shape on the R rows (llmie_linear_swiglu + llmie_linear,
                                     each on another expert's matrices): the same weight bytes at one row
  prefill T tokens:         rt1 / rt4  llmie_moe_ffn grouped under LLMIE_MOE_FORCE_RT1 / _RT4
                            dense      ONE dense FFN of inter size Ie on the T tokens (each token runs k experts: the MoE layer does
                                       k times these FLOPs)
--mxfp4 adds the same arms on the MXFP4 image of the same experts (llmie_moe_ffn_ex; mx_gemv, mx_grouped, mx_rt1, mx_rt4), interleaved
with the fp16 arms in every round, and reports each one's ratio to its fp16 arm and the weight bytes per second of the faster route
(fp16: 2 bytes per weight, MXFP4: 17 / 32).  Decode rows above 16 have no GEMV arm (LLMIE_MOE_FORCE_GEMV stops at 16 rows).
The rows of a call are independent normal vectors and the router is random, so the pairs spread over the experts as a trained
router's roughly would.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (load_llmie)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps   # ms


def measure(arms, rounds, reps):
    for fn in arms.values():   # every arm warm
        fn()
        fn()
    torch.cuda.synchronize()
    t = {n: [] for n in arms}
    for _ in range(rounds):
        for n, fn in arms.items():
            fn()
            t[n].append(timed(fn, reps))
    return {n: dict(ms=statistics.median(v), min=min(v), max=max(v)) for n, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--decode", type=int, nargs="*", default=[1, 2, 3, 4, 5, 6, 8, 12, 16])
    ap.add_argument("--prefill", type=int, nargs="*", default=[128, 512, 2048])
    ap.add_argument("--hidden", type=int, default=4096)
    ap.add_argument("--inter", type=int, default=14336)
    ap.add_argument("--experts", type=int, default=8)
    ap.add_argument("--top-k", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--mxfp4", action="store_true", help="add the MXFP4-expert arms beside the fp16 ones")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("moebench: needs a GPU (a time measured anywhere else says nothing)")
    llmie = bench.load_llmie()
    H, Ie, E, k = a.hidden, a.inter, a.experts, a.top_k
    g = torch.Generator(device="cuda").manual_seed(0)
    router = (torch.randn((E, H), generator=g, device="cuda") / H ** 0.5).half()
    gate_up = (torch.randn((E, 2 * Ie, H), generator=g, device="cuda") / H ** 0.5).half()
    down = (torch.randn((E, H, Ie), generator=g, device="cuda") / Ie ** 0.5).half()
    exq = llmie.MoeExperts.quantize(router, gate_up, down) if a.mxfp4 else None
    top = max(a.decode + a.prefill)
    ws = llmie.moe_workspace(top, H, Ie, E, k)
    results = []
    for kind, rows_list in (("decode", a.decode), ("prefill", a.prefill)):
        for R in rows_list:
            x = torch.randn((R, H), generator=g, device="cuda").half()
            resid = torch.randn((R, H), generator=g, device="cuda").half()
            y, act, yd = torch.empty_like(x), torch.empty((R, Ie), dtype=torch.float16, device="cuda"), torch.empty_like(x)
            ids, _ = llmie.moe_route(x, router, k)
            chosen = ids[0].tolist()

            def moe(flags):
                return lambda: llmie.moe_ffn(x, router, gate_up, down, y, k, resid=resid, flags=flags, workspace=ws)

            def moe_mx(flags):
                return lambda: llmie.moe_ffn_ex(x, exq, y, k, resid=resid, flags=flags, workspace=ws)

            def dense(experts):
                def run():
                    for e in experts:
                        llmie.linear_swiglu(x, gate_up[e], act)
                        llmie.linear(act, down[e], yd, residual=resid)
                return run

            if kind == "decode":
                arms = dict(grouped=moe(llmie.MOE_FORCE_GROUPED), dense=dense(chosen))
                if R <= 16:
                    arms["gemv"] = moe(llmie.MOE_FORCE_GEMV)
                if a.mxfp4:
                    arms["mx_grouped"] = moe_mx(llmie.MOE_FORCE_GROUPED)
                    if R <= 16:
                        arms["mx_gemv"] = moe_mx(llmie.MOE_FORCE_GEMV)
                reps = a.reps
            else:
                arms = dict(rt1=moe(llmie.MOE_FORCE_GROUPED | llmie.MOE_FORCE_RT1), rt4=moe(llmie.MOE_FORCE_GROUPED | llmie.MOE_FORCE_RT4),
                            dense=dense(chosen[:1]))
                if a.mxfp4:
                    arms.update(mx_rt1=moe_mx(llmie.MOE_FORCE_GROUPED | llmie.MOE_FORCE_RT1), mx_rt4=moe_mx(llmie.MOE_FORCE_GROUPED | llmie.MOE_FORCE_RT4))
                reps = max(a.reps // 4, 2)
            try:   # the dense launches refuse some shapes (a fused SwiGLU projection above 64 rows with inter % 256 != 0): no dense arm then
                arms["dense"]()
            except llmie.LlmieError:
                del arms["dense"]
            r = measure(arms, a.rounds, reps)
            res = dict(kind=kind, rows=R, plan=llmie.moe_ffn_plan(R, H, Ie, E, k), **{n + "_ms": v["ms"] for n, v in r.items()},
                       **{n + "_min_max": [v["min"], v["max"]] for n, v in r.items()})
            if a.mxfp4:
                # the weights a call streams: every expert some pair selects, once (counted from the routing of this call's rows)
                touched = len(set(ids.flatten().tolist()))
                weights = touched * 3 * Ie * H
                f16 = min(v["ms"] for n, v in r.items() if n in ("gemv", "grouped", "rt1", "rt4"))
                mx4 = min(v["ms"] for n, v in r.items() if n.startswith("mx_"))
                res.update(experts_touched=touched, f16_best_ms=f16, mx_best_ms=mx4, mx_over_f16=mx4 / f16,
                           f16_weight_tb_s=weights * 2 / f16 / 1e9, mx_weight_tb_s=weights * 17 / 32 / mx4 / 1e9)
                for n in ("gemv", "grouped", "rt1", "rt4"):
                    if n in r and "mx_" + n in r:
                        res["mx_%s_over_%s" % (n, n)] = r["mx_" + n]["ms"] / r[n]["ms"]
                if "mx_gemv" in r:
                    res["mx_grouped_over_mx_gemv"] = r["mx_grouped"]["ms"] / r["mx_gemv"]["ms"]
            if kind == "decode" and "gemv" in r:
                if "dense" in r:
                    res["gemv_over_dense"] = r["gemv"]["ms"] / r["dense"]["ms"]
                res["grouped_over_gemv"] = r["grouped"]["ms"] / r["gemv"]["ms"]
            elif kind == "prefill":
                best = min(r["rt1"]["ms"], r["rt4"]["ms"])
                res["tokens_per_s"] = R / best * 1e3
                res["rt4_over_rt1"] = r["rt4"]["ms"] / r["rt1"]["ms"]
                if "dense" in r:
                    res["dense_ffn_over_moe"] = r["dense"]["ms"] / best
            results.append(res)
            print(json.dumps(res), file=sys.stderr)
    line = json.dumps(dict(bench="moe", mxfp4=bool(a.mxfp4), device=torch.cuda.get_device_name(0), hidden=H, inter=Ie, experts=E, top_k=k, rounds=a.rounds, reps=a.reps,
                           results=results))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
