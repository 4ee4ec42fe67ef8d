#!/usr/bin/env python3
"""MLA decode attention per layer, at DeepSeek shapes (16 and 128 heads, fp16 latent cache of 576 halves per token), same process,
interleaved rounds, medians:

    python tools/mlabench.py [--heads 16 128] [--batches 1 8 32] [--ctx 2048 8192] [--rounds 7] [--reps 10] [--out FILE]

  decode    llmie_mla_decode alone (device-resident context lengths, grid sized from max_seq_len = ctx), dense and paged
  chain     the four launches of a layer: mla_kv_append, mla_q_absorb, mla_decode, mla_out_project (dense and paged)
  torch     a torch fp16 composition of the same absorbed math on the same tensors: matmul -> softmax -> matmul (dense cache)
  bound     the arithmetic bound max(ctx * 1152 B * batch / HBM rate, FLOPs / MFMA rate) of the attention, FLOPs = 2 * batch * heads *
            ctx * (576 + 512); the rates are the datasheet peaks bench.py reports under `peaks` (--hbm-gbs, --mfma-tflops)

With --prefill (lengths of one sequence) and --prefill-ragged (the lengths of one ragged batch) the prompt rows follow, no history:
  append, up, flash   llmie_mla_kv_append_rows, llmie_mla_kv_up, llmie_mla_prefill, each alone, and `sum`, the three in a row (dense)
  torch     a torch fp16 composition on the same tensors, per sequence: matmul for the up-projection, then causal
            scaled_dot_product_attention with k = cat(k_nope, k_pe) (q_pe rotated ahead of the clock); null where torch refuses it
  bound     max(bytes / HBM rate, FLOPs / MFMA rate): bytes = the latent rows read, kv_up written and read once, q and out; FLOPs =
            2 * 512 * 256 per token and head for the projection + 2 * (192 + 128) per visible (query, key) pair and head

With --verify ROWS... (e.g. 2 4 8 16) the speculative step follows, per heads x ctx x batch and row count, one interleaved run per cell:
  verify    llmie_mla_verify: `rows` chain rows per sequence, the last of them at context ctx (hist = ctx - rows)
  decode    ONE llmie_mla_decode call at context ctx; rows x decode is the only route to a chain without the verify kernel
  prefill   (--verify-prefill, the first cell of every row count) llmie_mla_kv_up + llmie_mla_prefill with hist = ctx - rows: the
            un-absorbed route, which projects the whole history up on every step

With --e4m3 the e4m3 latent cache (640 bytes per token) follows instead of the rows above, one interleaved run per cell:
  decode_e4m3   llmie_mla_decode_e4m3 on the quantised copy of the cache the fp16 `decode` of the same run reads (dense); their ratio,
            and the HBM bound at ctx * 640 B * batch

With --sparse [--top-k 2048] [--sparse-ctx 8192 32768] [--index-ctx 8192 32768 131072] the sparse decode step follows instead, per
heads x batch one interleaved run, then per index context x batch:
  dense_sameK / sparse_sameK   llmie_mla_decode at ctx = top_k beside llmie_mla_decode_sparse over sel = 0 .. top_k - 1: the same rows,
            so their ratio (gather_over_dense) is the price of the gather
  dense_ctxC / sparse_ctxC     llmie_mla_decode over a full context C beside llmie_mla_decode_sparse over a random sorted selection of it
  index_topk   llmie_mla_index_topk (both launches) by device events; kernel_us: each kernel's own time from a profiled pass of the
            same call; the bound ctx * 256 B * batch / HBM rate of the logits

Prints one JSON line (and writes it to --out): microseconds, and the ratios decode / bound and torch / decode.  Only time is measured."""
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
F16 = torch.float16
SCALE = 1.0 / 192 ** 0.5


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def interleaved(arms, rounds, reps):
    """{name: (median, min, max) seconds per call}; a round runs every arm once, in turn; every arm is warmed up first"""
    for fn in arms.values():
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            times[k].append(timed(fn, reps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def bench(heads, batch, ctx, rounds, reps, hbm_gbs, mfma_tflops):
    dev = "cuda"
    pages = ctx // 128
    dense = torch.empty((1, batch, ctx, 576), dtype=F16, device=dev).normal_(0, 0.5)
    pool = dense.view(1, batch * pages, 128, 576).clone()
    table = torch.randperm(batch * pages, device=dev).int().view(batch, pages).contiguous()
    q = torch.randn((batch, heads, 192), device=dev).to(F16)
    kv_b = (torch.randn((heads, 256, 512), device=dev) / 128 ** 0.5).to(F16)
    kv_a = (0.5 * torch.randn((batch, 576), device=dev)).to(F16)
    gamma = torch.ones(512, dtype=F16, device=dev)
    tab = torch.from_numpy(llmie.rope_table(ctx, 64, 64, 10000.0)).to(dev)
    lengths = torch.full((batch,), ctx, dtype=torch.int32, device=dev)
    q_lat = torch.empty((batch, heads, 576), dtype=F16, device=dev)
    o_lat = torch.empty((batch, heads, 512), dtype=F16, device=dev)
    out = torch.empty((batch, heads * 128), dtype=F16, device=dev)
    ws = llmie.mla_workspace(batch, heads, ctx)
    llmie.mla_q_absorb(q, kv_b, tab, q_lat, lengths, ctx)
    paged = dict(block_table=table, max_seq_len=ctx)

    def decode(cache, **kw):
        llmie.mla_decode(q_lat, cache, 0, lengths, SCALE, o_lat, ws, **kw)

    def chain(cache, **kw):
        llmie.mla_kv_append(kv_a, gamma, 1e-6, tab, cache, 0, lengths, **kw)
        llmie.mla_q_absorb(q, kv_b, tab, q_lat, lengths, ctx)
        decode(cache, **kw)
        llmie.mla_out_project(o_lat, kv_b, out)

    def composed():
        c = dense[0]
        p = torch.softmax(torch.matmul(q_lat, c.transpose(1, 2)) * SCALE, dim=-1)
        return torch.matmul(p, c[:, :, :512])

    t = interleaved({"decode": lambda: decode(dense), "decode_paged": lambda: decode(pool, **paged), "chain": lambda: chain(dense),
                     "chain_paged": lambda: chain(pool, **paged), "torch": composed}, rounds, reps)
    flops = 2.0 * batch * heads * ctx * (576 + 512)
    t_hbm, t_mfma = ctx * 1152.0 * batch / (hbm_gbs * 1e9), flops / (mfma_tflops * 1e12)
    bound = max(t_hbm, t_mfma)
    return dict(heads=heads, batch=batch, ctx=ctx, plan=llmie.mla_decode_plan(batch, heads, ctx)[0],
                us={k: round(v[0] * 1e6, 1) for k, v in t.items()}, spread_us={k: [round(v[1] * 1e6, 1), round(v[2] * 1e6, 1)] for k, v in t.items()},
                bound_us=round(bound * 1e6, 2), bound_by="hbm" if t_hbm >= t_mfma else "mfma",
                decode_over_bound=round(t["decode"][0] / bound, 2), torch_over_decode=round(t["torch"][0] / t["decode"][0], 2))


def bench_e4m3(heads, batch, ctx, rounds, reps, hbm_gbs, mfma_tflops):
    """decode_e4m3 beside the fp16 decode of the same interleaved run (dense), on caches that hold the same latents"""
    dev, c_scale = "cuda", 0.0123
    dense = torch.empty((1, batch, ctx, 576), dtype=F16, device=dev).normal_(0, 0.5)
    e4 = torch.empty((1, batch, ctx, 640), dtype=torch.uint8, device=dev)
    e4[..., :512] = (dense[..., :512].float() / c_scale).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    e4[..., 512:] = dense[..., 512:].contiguous().view(torch.uint8)
    q_lat = (torch.randn((batch, heads, 576), device=dev) / 24).to(F16)
    lengths = torch.full((batch,), ctx, dtype=torch.int32, device=dev)
    o16, o8 = (torch.empty((batch, heads, 512), dtype=F16, device=dev) for _ in range(2))
    ws = llmie.mla_workspace(batch, heads, ctx)
    t = interleaved({"decode": lambda: llmie.mla_decode(q_lat, dense, 0, lengths, SCALE, o16, ws),
                     "decode_e4m3": lambda: llmie.mla_decode_e4m3(q_lat, e4, c_scale, 0, lengths, SCALE, o8, ws)}, rounds, reps)
    flops = 2.0 * batch * heads * ctx * (576 + 512)
    t_hbm, t_mfma = ctx * 640.0 * batch / (hbm_gbs * 1e9), flops / (mfma_tflops * 1e12)
    return dict(heads=heads, batch=batch, ctx=ctx, plan=llmie.mla_decode_e4m3_plan(batch, heads, ctx)[0],
                us={k: round(v[0] * 1e6, 1) for k, v in t.items()}, spread_us={k: [round(v[1] * 1e6, 1), round(v[2] * 1e6, 1)] for k, v in t.items()},
                e4m3_over_f16=round(t["decode_e4m3"][0] / t["decode"][0], 3), hbm_bound_640_us=round(t_hbm * 1e6, 2),
                bound_us=round(max(t_hbm, t_mfma) * 1e6, 2), bound_by="hbm" if t_hbm >= t_mfma else "mfma",
                e4m3_over_hbm_bound=round(t["decode_e4m3"][0] / t_hbm, 2))


def bench_prefill(heads, lens, rounds, reps, hbm_gbs, mfma_tflops):
    dev, batch, total, span = "cuda", len(lens), sum(lens), -(-max(lens) // 128) * 128
    cache = torch.zeros((1, batch, span, 576), dtype=F16, device=dev)
    kv_b = (torch.randn((heads, 256, 512), device=dev) / 128 ** 0.5).to(F16)
    kv_a = (0.5 * torch.randn((total, 576), device=dev)).to(F16)
    q = torch.randn((total, heads, 192), device=dev).to(F16)
    gamma = torch.ones(512, dtype=F16, device=dev)
    tab = torch.from_numpy(llmie.rope_table(span, 64, 64, 10000.0)).to(dev)
    starts = [sum(lens[:b]) for b in range(batch + 1)]
    cum = torch.tensor(starts, dtype=torch.int32, device=dev)
    hist = torch.zeros(batch, dtype=torch.int32, device=dev)
    kv_up = torch.empty((batch, span, heads, 256), dtype=F16, device=dev)
    out = torch.empty((total, heads * 128), dtype=F16, device=dev)
    mq = max(lens)

    def append():
        llmie.mla_kv_append_rows(kv_a, gamma, 1e-6, tab, cache, 0, cum, hist, mq, span)

    def up():
        llmie.mla_kv_up(cache, kv_b, kv_up, 0, cum, hist, mq)

    def flash():
        llmie.mla_prefill(q, kv_up, cache, tab, 0, cum, hist, SCALE, out, mq)

    def three():
        append(), up(), flash()

    # the composition's query: q_pe rotated ahead of the clock
    pos = torch.cat([torch.arange(n, device=dev) for n in lens])
    c, s_, x0, x1 = tab[pos, :, 0][:, None], tab[pos, :, 1][:, None], q[..., 128:160].float(), q[..., 160:].float()
    q_rot = torch.cat([q[..., :128], (x0 * c - x1 * s_).to(F16), (x1 * c + x0 * s_).to(F16)], -1)
    w = kv_b.view(heads * 256, 512)

    def composed():
        for b, n in enumerate(lens):
            rows = cache[0, b, :n]
            u = torch.matmul(rows[:, :512], w.t()).view(n, heads, 256)
            k = torch.cat([u[..., :128], rows[:, None, 512:].expand(n, heads, 64)], -1)
            t0 = starts[b]
            torch.nn.functional.scaled_dot_product_attention(q_rot[t0:t0 + n].transpose(0, 1)[None], k.transpose(0, 1)[None],
                                                             u[..., 128:].transpose(0, 1)[None], is_causal=True, scale=SCALE)

    three()
    arms = {"append": append, "up": up, "flash": flash, "sum": three}
    try:
        composed()
        torch.cuda.synchronize()
        arms["torch"] = composed
    except Exception as e:   # (a shape torch's attention refuses: the row says so)
        print("torch composition refused: %s" % str(e).splitlines()[0], file=sys.stderr)
    t = interleaved(arms, rounds, reps)
    pairs = sum(n * (n + 1) / 2 for n in lens)
    flops = 2.0 * 512 * 256 * total * heads + 2.0 * (192 + 128) * pairs * heads
    nbytes = total * 1152.0 + 2 * total * heads * 512.0 + total * heads * (384 + 256.0)
    t_hbm, t_mfma = nbytes / (hbm_gbs * 1e9), flops / (mfma_tflops * 1e12)
    bound = max(t_hbm, t_mfma)
    return dict(heads=heads, lens=lens, plan=llmie.mla_prefill_plan(batch, heads, mq, span, span, total_tokens=total)[0],
                us={k: round(v[0] * 1e6, 1) for k, v in t.items()}, spread_us={k: [round(v[1] * 1e6, 1), round(v[2] * 1e6, 1)] for k, v in t.items()},
                bound_us=round(bound * 1e6, 2), bound_by="hbm" if t_hbm >= t_mfma else "mfma", sum_over_bound=round(t["sum"][0] / bound, 2),
                torch_over_sum=round(t["torch"][0] / t["sum"][0], 2) if "torch" in t else None)


def bench_verify(heads, batch, ctx, rows, rounds, reps, with_prefill):
    dev = "cuda"
    cache = torch.empty((1, batch, ctx, 576), dtype=F16, device=dev).normal_(0, 0.5)
    q_lat = torch.randn((batch, rows, heads, 576), device=dev).to(F16)
    o_lat = torch.empty((batch, rows, heads, 512), dtype=F16, device=dev)
    hist = torch.full((batch,), ctx - rows, dtype=torch.int32, device=dev)
    lengths = torch.full((batch,), ctx, dtype=torch.int32, device=dev)
    ws_v, ws_d = llmie.mla_verify_workspace(batch, rows, heads, ctx), llmie.mla_workspace(batch, heads, ctx)
    q1, o1 = q_lat[:, 0].contiguous(), torch.empty((batch, heads, 512), dtype=F16, device=dev)
    arms = {"verify": lambda: llmie.mla_verify(q_lat, cache, 0, hist, SCALE, o_lat, workspace=ws_v),
            "decode": lambda: llmie.mla_decode(q1, cache, 0, lengths, SCALE, o1, ws_d)}
    if with_prefill:
        kv_b = (torch.randn((heads, 256, 512), device=dev) / 128 ** 0.5).to(F16)
        tab = torch.from_numpy(llmie.rope_table(ctx, 64, 64, 10000.0)).to(dev)
        q = torch.randn((batch * rows, heads, 192), device=dev).to(F16)
        cum = torch.arange(0, (batch + 1) * rows, rows, dtype=torch.int32, device=dev)
        kv_up = torch.empty((batch, ctx, heads, 256), dtype=F16, device=dev)
        out = torch.empty((batch * rows, heads * 128), dtype=F16, device=dev)

        def prefill():
            llmie.mla_kv_up(cache, kv_b, kv_up, 0, cum, hist, rows)
            llmie.mla_prefill(q, kv_up, cache, tab, 0, cum, hist, SCALE, out, rows)

        arms["prefill"] = prefill
    t = interleaved(arms, rounds, reps)
    us = {k: round(v[0] * 1e6, 1) for k, v in t.items()}
    return dict(heads=heads, batch=batch, ctx=ctx, rows=rows, plan=llmie.mla_verify_plan(batch, rows, heads, ctx)[0], us=us,
                spread_us={k: [round(v[1] * 1e6, 1), round(v[2] * 1e6, 1)] for k, v in t.items()},
                rows_x_decode_us=round(rows * t["decode"][0] * 1e6, 1), rows_decode_over_verify=round(rows * t["decode"][0] / t["verify"][0], 2))


def bench_sparse(heads, batch, ctxs, top_k, rounds, reps):
    """llmie_mla_decode_sparse at top_k entries beside llmie_mla_decode, one interleaved run: the identity selection 0 .. top_k - 1 against
    the dense decode at ctx = top_k (the same rows: the price of the gather), and a random sorted selection out of every full context
    against the dense decode over that context"""
    dev, span = "cuda", max(ctxs)
    cache = torch.empty((1, batch, span, 576), dtype=F16, device=dev).normal_(0, 0.5)
    q_lat = (torch.randn((batch, heads, 576), device=dev) / 24).to(F16)
    o_d, o_s = (torch.empty((batch, heads, 512), dtype=F16, device=dev) for _ in range(2))
    ws_d, ws_s = llmie.mla_workspace(batch, heads, span), llmie.mla_workspace(batch, heads, top_k)
    count = torch.full((batch,), top_k, dtype=torch.int32, device=dev)

    def arms_at(ctx, sel, tag):
        lengths = torch.full((batch,), ctx, dtype=torch.int32, device=dev)
        return {"dense_%s" % tag: lambda: llmie.mla_decode(q_lat, cache, 0, lengths, SCALE, o_d, ws_d, max_ctx=ctx),
                "sparse_%s" % tag: lambda: llmie.mla_decode_sparse(q_lat, cache, 0, lengths, sel, count, SCALE, o_s, ws_s)}

    arms = arms_at(top_k, torch.arange(top_k, dtype=torch.int32, device=dev).repeat(batch, 1).contiguous(), "same%d" % top_k)
    for ctx in ctxs:
        sel = torch.rand((batch, ctx), device=dev).topk(top_k, dim=1).indices.sort(dim=1).values.int().contiguous()
        arms.update(arms_at(ctx, sel, "ctx%d" % ctx))
    t = interleaved(arms, rounds, reps)
    return dict(heads=heads, batch=batch, top_k=top_k, plan=llmie.mla_decode_sparse_plan(batch, heads, top_k, span)[0],
                us={k: round(v[0] * 1e6, 1) for k, v in t.items()}, spread_us={k: [round(v[1] * 1e6, 1), round(v[2] * 1e6, 1)] for k, v in t.items()},
                gather_over_dense=round(t["sparse_same%d" % top_k][0] / t["dense_same%d" % top_k][0], 3),
                dense_over_sparse={str(c): round(t["dense_ctx%d" % c][0] / t["sparse_ctx%d" % c][0], 2) for c in ctxs})


def bench_index(batch, ctx, top_k, rounds, reps, hbm_gbs):
    """llmie_mla_index_topk: the entry (both launches) by device events, then each kernel's own time from a profiled pass of the same call"""
    from torch.profiler import ProfilerActivity, profile
    dev = "cuda"
    k_idx = torch.randn((1, batch, ctx, 128), device=dev, dtype=F16)
    q_idx = torch.randn((batch, 64, 128), device=dev, dtype=F16)
    w_idx = torch.randn((batch, 64), device=dev) / 8
    lengths = torch.full((batch,), ctx, dtype=torch.int32, device=dev)
    sel, cnt = torch.empty((batch, top_k), dtype=torch.int32, device=dev), torch.empty(batch, dtype=torch.int32, device=dev)
    ws = llmie.mla_index_workspace(batch, ctx)

    def call():
        llmie.mla_index_topk(q_idx, w_idx, k_idx, 0, lengths, sel, cnt, ws)

    t = interleaved({"index_topk": call}, rounds, reps)["index_topk"]
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            call()
        torch.cuda.synchronize()
    kernels = {}
    for ev in prof.key_averages():
        for name in ("mla_index_logits_kernel", "mla_index_select_kernel"):
            if name in ev.key:
                total = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0)
                kernels[name] = round(total / max(ev.count, 1), 1)
    bound = ctx * 256.0 * batch / (hbm_gbs * 1e9)
    return dict(batch=batch, ctx=ctx, top_k=top_k, plan=llmie.mla_index_topk_plan(batch, top_k, ctx)[0], us=round(t[0] * 1e6, 1),
                spread_us=[round(t[1] * 1e6, 1), round(t[2] * 1e6, 1)], kernel_us=kernels or None, hbm_bound_us=round(bound * 1e6, 2),
                logits_over_bound=round(kernels["mla_index_logits_kernel"] / (bound * 1e6), 2) if "mla_index_logits_kernel" in kernels else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--ctx", type=int, nargs="+", default=[2048, 8192])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--mfma-tflops", type=float, default=2500.0)
    ap.add_argument("--prefill", type=int, nargs="*", default=[], help="prompt lengths of the batch-1 prefill rows, e.g. 512 2048 8192")
    ap.add_argument("--prefill-ragged", type=int, nargs="*", default=[], help="the prompt lengths of one ragged prefill batch")
    ap.add_argument("--verify", type=int, nargs="*", default=[], help="query rows per sequence of the speculative step, e.g. 2 4 8 16")
    ap.add_argument("--verify-prefill", action="store_true", help="add the kv_up + mla_prefill route to the first cell of every row count")
    ap.add_argument("--verify-only", action="store_true", help="skip the decode / chain / torch rows")
    ap.add_argument("--e4m3", action="store_true", help="the e4m3 latent cache: decode_e4m3 beside the fp16 decode, per heads x ctx x batch (these rows only)")
    ap.add_argument("--sparse", action="store_true", help="the sparse decode step (these rows only): decode_sparse beside decode, and index_topk")
    ap.add_argument("--top-k", type=int, default=2048)
    ap.add_argument("--sparse-ctx", type=int, nargs="+", default=[8192, 32768], help="full contexts the sparse decode is compared with")
    ap.add_argument("--index-ctx", type=int, nargs="*", default=[8192, 32768, 131072], help="contexts of the index_topk rows")
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mlabench measures on the GPU: there is no CPU path"
    res = dict(tool="mlabench", device=torch.cuda.get_device_name(0), peaks=dict(hbm_GBs_datasheet=a.hbm_gbs, mfma_f16_TFLOPs_datasheet=a.mfma_tflops))
    if a.sparse:
        res["sparse_rows"] = [bench_sparse(h, b, a.sparse_ctx, a.top_k, a.rounds, a.reps) for h in a.heads for b in a.batches]
        res["index_rows"] = [bench_index(b, c, a.top_k, a.rounds, a.reps, a.hbm_gbs) for c in a.index_ctx for b in a.batches]
    elif a.e4m3:
        res["e4m3_rows"] = [bench_e4m3(h, b, c, a.rounds, a.reps, a.hbm_gbs, a.mfma_tflops) for h in a.heads for c in a.ctx for b in a.batches]
    elif not a.verify_only:
        res["rows"] = [bench(h, b, c, a.rounds, a.reps, a.hbm_gbs, a.mfma_tflops) for h in a.heads for c in a.ctx for b in a.batches]
    if a.verify:
        cells = [(h, b, c) for h in a.heads for c in a.ctx for b in a.batches]
        res["verify_rows"] = [bench_verify(h, b, c, r, a.rounds, a.reps, a.verify_prefill and (h, b, c) == cells[0]) for r in a.verify
                              for h, b, c in cells]
    if a.prefill or a.prefill_ragged:
        res["prefill_rows"] = [bench_prefill(h, lens, a.rounds, a.reps, a.hbm_gbs, a.mfma_tflops) for h in a.heads
                               for lens in [[n] for n in a.prefill] + ([a.prefill_ragged] if a.prefill_ragged else [])]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
