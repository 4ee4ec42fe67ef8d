#!/usr/bin/env python3
"""MXFP4 weights against int4 (group 128) and fp16, at the Llama-2-7B geometry:

    python tools/mxfp4bench.py [--rounds 5] [--reps 100] [--replays 40] [--step-reps 100] [--layers 32] [--out profiles/mxfp4_bench.json]

Two measurements, one process, the arms alternating inside every round (mxfp4, int4, [fp16,] mxfp4, ...); the median round of each
arm is reported with its min and max:
  projections  llmie_linear_mxfp4 against llmie_linear_w4a16 on the four projection shapes of a 7B layer at M = 1, 4, 8, 32, 64.  Every
               call reads another copy of the matrix out of a pool larger than the 256 MiB Infinity Cache, so the weights come from
               HBM as they do in a decode step; the calls of a window are replayed from a captured graph (device time, no interpreter):
               a window is --replays x --reps calls, 20 ms (the smallest shape) to 0.6 s.  bytes = codes + scales + activations in + out;
               roofline = bytes / time / 8 TB/s.
  decode step  a 32-layer engine step (no LM head) at batch 1 and 32 on 2048 cached tokens: MXFP4 (the unfused sequence) against
               int4 (its fused GEMV / packed sequences) and fp16.  bytes = layer matrices + scales + the KV rows read.  A window is
               --step-reps steps: 0.2 s at batch 1, about 1 s at batch 32.
There is no gate: the int4 arm of the same run is what the MXFP4 arm is read against (4.25 against 4.125 bits per weight).
Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the flagship benchmark's weights and engine construction)

HBM_BYTES_PER_S = 8e12
POOL_BYTES = 640 << 20          # per arm and shape: 2.5 x the Infinity Cache


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps   # ms


def summary(ts):
    return dict(ms=statistics.median(ts), ms_min_max=[min(ts), max(ts)])


def bench_projection(llmie, M, K, N, rounds, reps, replays, g):
    wbytes = {"mxfp4": N * K // 2 + N * K // 32, "int4": N * K // 2 + N * (K // 128) * 2}
    copies = max(2, -(-POOL_BYTES // wbytes["int4"]))
    x = torch.randn((M, K), generator=g, device="cuda").half()
    y = torch.empty((M, N), dtype=torch.float16, device="cuda")
    codes = torch.randint(0, 256, (copies, N, K // 2), generator=g, device="cuda", dtype=torch.uint8)   # both arms read the same nibbles
    e8m0 = torch.randint(118, 122, (copies, N, K // 32), generator=g, device="cuda", dtype=torch.uint8)
    gscale = (torch.rand((copies, N, K // 128), generator=g, device="cuda") * 0.01 + 0.001).half()
    ws = {}
    for fmt, code in (("mxfp4", llmie.W_MXFP4), ("int4", llmie.W_INT4)):
        need = llmie.linear_workspace_bytes(code, M, K, N)
        ws[fmt] = torch.empty(need, dtype=torch.uint8, device="cuda") if need else None
    turn = dict(mxfp4=0, int4=0)

    def call(fmt):
        i = turn[fmt] = (turn[fmt] + 1) % copies
        if fmt == "mxfp4":
            llmie.linear_mxfp4(x, codes[i], e8m0[i], y, workspace=ws[fmt])
        else:
            llmie.linear_w4a16(x, codes[i], gscale[i], y, 128, workspace=ws[fmt])

    # a call takes microseconds on the device and several times that in the interpreter: each arm's `reps` calls (cycling through
    # the pool) are captured once and replayed, so the window holds device time only
    arms = ("mxfp4", "int4")
    graphs = {}
    for fmt in arms:
        for _ in range(3):
            call(fmt)
        torch.cuda.synchronize()
        graphs[fmt] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[fmt], stream=torch.cuda.Stream()):
            for _ in range(reps):
                call(fmt)
    torch.cuda.synchronize()
    t = {fmt: [] for fmt in arms}
    for _ in range(rounds):
        for fmt in arms:
            graphs[fmt].replay()
            t[fmt].append(timed(graphs[fmt].replay, replays) / reps)
    res = dict(M=M, K=K, N=N, copies=copies,
               routes=dict(mxfp4=llmie.linear_route(llmie.W_MXFP4, x.data_ptr(), codes.data_ptr(), e8m0.data_ptr(), y.data_ptr(), M, K, N),
                           int4=llmie.linear_route(llmie.W_INT4, x.data_ptr(), codes.data_ptr(), gscale.data_ptr(), y.data_ptr(), M, K, N, group=128,
                                                   workspace=ws["int4"].data_ptr() if ws["int4"] is not None else None,
                                                   workspace_bytes=ws["int4"].numel() if ws["int4"] is not None else 0)))
    for fmt in arms:
        s = summary(t[fmt])
        nbytes = wbytes[fmt] + M * K * 2 + M * N * 2
        s.update(bytes=nbytes, roofline=nbytes / (s["ms"] * 1e-3) / HBM_BYTES_PER_S)
        res[fmt] = s
    res["mxfp4_over_int4"] = res["mxfp4"]["ms"] / res["int4"]["ms"]
    return res


def quantize_layers_mxfp4(llmie, layers):
    out = []
    for lw in layers:
        q = dict(attn_norm=lw["attn_norm"], ffn_norm=lw["ffn_norm"])
        for name in ("qkv", "o", "gate_up", "down"):
            n, k = lw[name].shape
            wq = torch.empty((n, k // 2), dtype=torch.uint8, device="cuda")
            sc = torch.empty((n, k // 32), dtype=torch.uint8, device="cuda")
            llmie.quantize_mxfp4(lw[name], wq, sc)
            q[name] = dict(data=wq, scale=sc)
        out.append(q)
    return out


def bench_decode(llmie, cfg, weights, layer_sets, B, ctx, rounds, reps):
    H = cfg["head_num"] * cfg["head_size"]
    arms = ("mxfp4", "int4", "f16")
    # one pair of caches for the three engines: a step appends at slot ctx, which the next arm overwrites
    kv_shape = (cfg["num_layers"], B, cfg["kv_head_num"], ctx + 1, cfg["head_size"])
    kc = torch.empty(kv_shape, dtype=torch.float16, device="cuda").uniform_(-0.5, 0.5, generator=weights["gen"])
    vc = torch.empty(kv_shape, dtype=torch.float16, device="cuda").uniform_(-0.5, 0.5, generator=weights["gen"])
    code = dict(mxfp4=llmie.W_MXFP4, int4=llmie.W_INT4, f16=llmie.W_F16)
    decs = {fmt: llmie.Decoder(dict(cfg, max_seq_len=ctx + 1, max_batch=B, rotary_dim=cfg["head_size"], rotary_base=10000.0, rms_eps=1e-5,
                                    dtype=llmie.F16, wfmt=code[fmt], int4_group=128), layer_sets[fmt]) for fmt in arms}
    x = torch.randn((B, H), generator=weights["gen"], device="cuda").half()
    y = torch.empty_like(x)

    def step(fmt):
        decs[fmt].forward(x, y, kc, vc, ctx + 1)

    for fmt in arms:
        step(fmt)
        step(fmt)
    torch.cuda.synchronize()
    t = {fmt: [] for fmt in arms}
    for _ in range(rounds):
        for fmt in arms:
            step(fmt)
            t[fmt].append(timed(lambda: step(fmt), reps))
    elems = (cfg["head_num"] + 2 * cfg["kv_head_num"]) * cfg["head_size"] * H + H * H + 3 * H * cfg["inter_size"]
    per_weight = dict(mxfp4=0.5 + 1 / 32, int4=0.5 + 2 / 128, f16=2.0)
    kv = 2 * cfg["num_layers"] * B * ctx * cfg["kv_head_num"] * cfg["head_size"] * 2
    res = dict(batch=B, ctx=ctx, plans={fmt: llmie.decoder_plan_name(decs[fmt].cfg, 0, B) for fmt in arms})
    for fmt in arms:
        s = summary(t[fmt])
        nbytes = int(elems * per_weight[fmt]) * cfg["num_layers"] + kv
        s.update(bytes=nbytes, roofline=nbytes / (s["ms"] * 1e-3) / HBM_BYTES_PER_S, tokens_per_s=B / (s["ms"] * 1e-3))
        res[fmt] = s
    res["mxfp4_over_int4"] = res["mxfp4"]["ms"] / res["int4"]["ms"]
    res["mxfp4_over_f16"] = res["mxfp4"]["ms"] / res["f16"]["ms"]
    for dec in decs.values():
        dec.close()
    del decs, kc, vc
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=100, help="projection calls per captured graph")
    ap.add_argument("--replays", type=int, default=40, help="replays of the captured graph per timed window")
    ap.add_argument("--step-reps", type=int, default=100, help="decode steps per timed window")
    ap.add_argument("--rows", type=int, nargs="*", default=[1, 4, 8, 32, 64])
    ap.add_argument("--batch", type=int, nargs="*", default=[1, 32])
    ap.add_argument("--ctx", type=int, default=2048)
    ap.add_argument("--layers", type=int, default=0, help="fewer layers than the model's 32 (a rehearsal; not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mxfp4_bench.json"))
    a = ap.parse_args()
    if a.rounds < 5:
        sys.exit("mxfp4bench: at least 5 rounds")
    if not torch.cuda.is_available():
        sys.exit("mxfp4bench: needs a GPU (a time measured anywhere else says nothing)")
    llmie = bench.load_llmie()
    cfg = dict(bench.LLAMA2_7B)
    if a.layers:
        cfg["num_layers"] = a.layers
    H, I = cfg["head_num"] * cfg["head_size"], cfg["inter_size"]
    QKV = (cfg["head_num"] + 2 * cfg["kv_head_num"]) * cfg["head_size"]
    g = torch.Generator(device="cuda").manual_seed(4)
    projections = []
    for name, K, N in (("qkv", H, QKV), ("o", H, H), ("gate_up", H, 2 * I), ("down", I, H)):
        for M in a.rows:
            r = bench_projection(llmie, M, K, N, a.rounds, a.reps, a.replays, g)
            r["name"] = name
            projections.append(r)
        torch.cuda.empty_cache()
    weights = bench.build_weights(torch, cfg, 0)
    layer_sets = dict(f16=weights["layers"], int4=bench.quantize_layers(torch, llmie, weights["layers"], "int4"),
                      mxfp4=quantize_layers_mxfp4(llmie, weights["layers"]))
    decode = [bench_decode(llmie, cfg, weights, layer_sets, B, a.ctx, a.rounds, a.step_reps) for B in a.batch]
    res = dict(bench="mxfp4", device=torch.cuda.get_device_name(0), rounds=a.rounds, reps=a.reps, step_reps=a.step_reps, layers=cfg["num_layers"],
               projections=projections, decode=decode)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
