#!/usr/bin/env python3
"""Speculative decoding: what a verify step costs against a plain decode step, at the Llama-2-7B geometry, fp16, paged cache:

    python tools/specbench.py [--batch 1 8] [--k 2 4 7] [--ctx 2048] [--rounds 7] [--reps 20] [--out FILE]

plain step   forward_paged_ragged (one token per sequence on top of ctx cached tokens) + lm_head_sample_params
verify step  input_embedding + prefill_paged (k + 1 inputs per sequence on top of ctx cached tokens) + rmsnorm + linear over the
             batch * (k + 1) rows + spec_verify; the n-gram drafter's launch is timed on its own (ngram_ms)

    python tools/specbench.py --sampled [--batch 1 8] [--k 2 4 7] [--rounds 7] [--reps 50]

the sampled-draft arm: the device time of llmie_spec_verify_sampled beside llmie_spec_verify on the same [batch * (k + 1), 32000]
fp16 logits (no model: the entries alone, between device events), the drafts drawn by llmie_sample_logits from draft logits that
are the target's plus noise -- so that acceptances and rejections (the residual pass) both occur; the two arms alternate inside
every round.

    python tools/specbench.py --tree 8 16 32 64 [--batch 1 8] [--k 7] [--rounds 7] [--reps 20]

the tree arm: beside the plain step and the linear verify steps of --k, one TREE step per n -- spec_tree_prepare + input_embedding
+ prefill_paged of n nodes per sequence with the tree set (a binary tree in heap order) + rmsnorm + linear over the batch * n rows
+ spec_verify_tree + kv_tree_commit; the tree drafter's launch is timed on its own (ngram_tree_ms).

Same build, same process, same weights; the arms alternate inside every round (plain, k = 2, 4, 7, plain, ...) and the median
round of each arm is reported with its min and max.  A verify step emits 1 .. k + 1 tokens for its time, a plain step one: the
break-even is verify_ms / plain_ms emitted tokens per verify step, i.e. that minus one accepted drafts.  Prints one JSON line
(and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the flagship benchmark's weights and engine construction)

EPS, V_PAGE = 1e-5, 128


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps   # ms


def run_batch(llmie, cfg, weights, B, ks, ctx, rounds, reps, trees=()):
    H, V, L, KVH, HS = cfg["head_num"] * cfg["head_size"], cfg["vocab_size"], cfg["num_layers"], cfg["kv_head_num"], cfg["head_size"]
    kmax = max(ks)
    max_pages = (ctx + max([kmax + 1] + list(trees)) + V_PAGE - 1) // V_PAGE
    num_pages = B * max_pages
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    ecfg = dict(cfg, max_seq_len=max_pages * V_PAGE, max_batch=B, rotary_dim=HS, rotary_base=10000.0, rms_eps=EPS, dtype=llmie.F16,
                wfmt=llmie.W_F16, int4_group=128, kv_fmt=llmie.KV_NATIVE, k_scale=1.0, v_scale=1.0)
    dec = llmie.Decoder(ecfg, weights["layers"])
    kp = torch.empty((L, num_pages, KVH, V_PAGE, HS), dtype=torch.float16, device="cuda").normal_(0, 0.5)
    vp = torch.empty((L, num_pages, KVH, V_PAGE, HS), dtype=torch.float16, device="cuda").normal_(0, 0.5)
    table = torch.randperm(num_pages, device="cuda").to(torch.int32).reshape(B, max_pages).contiguous()
    g = torch.Generator(device="cuda").manual_seed(B)
    params = llmie.sampling_params([dict(temperature=0.8, top_k=50, top_p=0.9, seed=b) for b in range(B)])
    seq, fin = i32([0] * B), torch.zeros(B, dtype=torch.uint8, device="cuda")

    # plain step
    x1 = torch.randn((B, H), generator=g, device="cuda").half()
    y1, logits1, out1 = torch.empty_like(x1), torch.empty((B, V), dtype=torch.float16, device="cuda"), i32([0] * B)
    ctx1 = i32([ctx + 1] * B)
    ws1 = torch.empty(llmie.sample_logits_workspace_bytes(B, V), dtype=torch.uint8, device="cuda")

    def plain():
        dec.forward_paged_ragged(x1, y1, kp, vp, table, ctx1)
        dec.lm_head_sample_params(y1, weights["final_norm"], weights["lm_head"], llmie.W_F16, logits1, params, seq, fin, out1, 7, -1, workspace=ws1)

    # verify steps
    arms = {}
    cached = i32([ctx] * B)
    for k in ks:
        T = B * (k + 1)
        ids = torch.randint(0, V, (T,), generator=g, device="cuda").to(torch.int32)
        drafts = ids.reshape(B, k + 1)[:, 1:].contiguous()
        xk, logits = torch.empty((T, H), dtype=torch.float16, device="cuda"), torch.empty((T, V), dtype=torch.float16, device="cuda")
        yk = torch.empty_like(xk)
        in_len = i32([k + 1] * B)
        ws = torch.empty(llmie.spec_verify_workspace_bytes(B, k, V), dtype=torch.uint8, device="cuda")
        outs = (torch.empty((B, k + 1), dtype=torch.int32, device="cuda"), i32([0] * B))

        def verify(k=k, ids=ids, drafts=drafts, xk=xk, yk=yk, logits=logits, in_len=in_len, ws=ws, outs=outs):
            llmie.input_embedding(ids, weights["embed"], xk)
            dec.prefill_paged(xk, yk, kp, vp, table, in_len, cached, k + 1)
            llmie.rmsnorm(yk, None, weights["final_norm"], EPS)
            llmie.linear(yk, weights["lm_head"], logits)
            llmie.spec_verify(logits, drafts, params, seq, fin, -1, draft_len=None, step=7, workspace=ws, out=outs)

        arms[k] = verify
    # tree steps: a binary tree in heap order per sequence (depth log2 n; every node live), the walk decided by random logits
    tree_arms = {}
    for n in trees:
        T = B * n
        t_ids = torch.randint(0, V, (B, n), generator=g, device="cuda").to(torch.int32)
        t_parent = i32([[-1] + [(i - 1) // 2 for i in range(1, n)]] * B)
        st = llmie.spec_tree_state(B, n)
        xt, t_logits = torch.empty((T, H), dtype=torch.float16, device="cuda"), torch.empty((T, V), dtype=torch.float16, device="cuda")
        yt = torch.empty_like(xt)
        t_in_len = i32([n] * B)
        t_ws = torch.empty(llmie.spec_verify_tree_workspace_bytes(B, n, V), dtype=torch.uint8, device="cuda")

        def tree_step(n=n, t_ids=t_ids, t_parent=t_parent, st=st, xt=xt, yt=yt, t_logits=t_logits, t_in_len=t_in_len, t_ws=t_ws):
            llmie.spec_tree_prepare(t_parent, None, out=(st.depth, st.anc))
            dec.set_tree(st.depth, st.anc)
            llmie.input_embedding(t_ids.view(-1), weights["embed"], xt)
            dec.prefill_paged(xt, yt, kp, vp, table, t_in_len, cached, n)
            dec.set_tree(None, None)
            llmie.rmsnorm(yt, None, weights["final_norm"], EPS)
            llmie.linear(yt, weights["lm_head"], t_logits)
            llmie.spec_verify_tree(t_logits, t_ids, t_parent, st.depth, st.anc, params, seq, fin, -1, step=7, workspace=t_ws,
                                   out=(st.tokens, st.count, st.path))
            llmie.kv_tree_commit(kp, vp, cached, st.path, st.count, block_table=table)

        tree_arms[n] = tree_step
    # the drafter alone, on rows of ctx tokens from an alphabet of 4 (matches of every n all over the row: the costly case)
    toks = torch.randint(0, 4, (B, ctx + 64), generator=g, device="cuda").to(torch.int32)
    tlen = i32([ctx] * B)
    dout = (torch.empty((B, kmax + 1), dtype=torch.int32, device="cuda"), torch.empty((B, kmax), dtype=torch.int32, device="cuda"), i32([0] * B))

    def draft():
        llmie.ngram_draft(toks, tlen, kmax, max_n=3, min_n=1, out=dout)

    nmax = max(trees) if trees else 0
    tout = (torch.empty((B, max(nmax, 1)), dtype=torch.int32, device="cuda"), torch.empty((B, max(nmax, 1)), dtype=torch.int32, device="cuda"), i32([0] * B))

    def draft_tree():
        llmie.ngram_draft_tree(toks, tlen, nmax, min(kmax, 15), branches=8, max_n=3, min_n=1, out=tout)

    for _ in range(3):   # every shape of the timed window, warm
        plain()
        draft()
        for k in ks:
            arms[k]()
        for n in trees:
            tree_arms[n]()
        if trees:
            draft_tree()
    torch.cuda.synchronize()
    tp, tv, td, tt, tdt = [], {k: [] for k in ks}, [], {n: [] for n in trees}, []
    for _ in range(rounds):
        tp.append(timed(plain, reps))
        for k in ks:
            tv[k].append(timed(arms[k], reps))
        for n in trees:
            tt[n].append(timed(tree_arms[n], reps))
        td.append(timed(draft, reps))
        if trees:
            tdt.append(timed(draft_tree, reps))
    mp = statistics.median(tp)
    res = dict(batch=B, ctx=ctx, plain_ms=mp, plain_ms_min_max=[min(tp), max(tp)], ngram_ms=statistics.median(td), verify=[])
    for k in ks:
        mv = statistics.median(tv[k])
        # per-round ratios: the spread of the break-even itself (the arms of a round run back to back)
        ratios = [a / b for a, b in zip(tv[k], tp)]
        res["verify"].append(dict(k=k, rows=B * (k + 1), verify_ms=mv, verify_ms_min_max=[min(tv[k]), max(tv[k])], verify_over_plain=mv / mp,
                                  verify_over_plain_min_max=[min(ratios), max(ratios)], break_even_tokens_per_step=mv / mp,
                                  break_even_accepted_drafts=mv / mp - 1, speedup_if_all_accepted=(k + 1) * mp / mv))
    if trees:
        res["ngram_tree_ms"] = statistics.median(tdt)
        res["tree"] = []
        kref = max(ks)
        for n in trees:
            mt = statistics.median(tt[n])
            ratios = [a / b for a, b in zip(tt[n], tp)]
            lin = [a / b for a, b in zip(tt[n], tv[kref])]
            res["tree"].append(dict(n=n, rows=B * n, tree_ms=mt, tree_ms_min_max=[min(tt[n]), max(tt[n])], tree_over_plain=mt / mp,
                                    tree_over_plain_min_max=[min(ratios), max(ratios)], break_even_tokens_per_step=mt / mp,
                                    break_even_accepted_nodes=mt / mp - 1, linear_k=kref, tree_over_linear=statistics.median(lin),
                                    tree_over_linear_min_max=[min(lin), max(lin)]))
    dec.close()
    del kp, vp
    torch.cuda.empty_cache()
    return res


def run_sampled(llmie, B, ks, rounds, reps, V=32000):
    """the sampled-draft arm: spec_verify and spec_verify_sampled alone, alternating, device events around `reps` calls"""
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(100 + B)
    params = llmie.sampling_params([dict(temperature=0.8, top_k=50, top_p=0.9, seed=b) for b in range(B)])
    dparams = llmie.sampling_params([dict(temperature=1.0, top_k=50, seed=1000 + b) for b in range(B)])
    out = dict(batch=B, vocab=V, arms=[])
    for k in ks:
        T = B * (k + 1)
        logits = (torch.randn((T, V), generator=g, device="cuda") * 3).half()
        dlogits = (logits.reshape(B, k + 1, V)[:, :k].float() + torch.randn((B, k, V), generator=g, device="cuda")).half().contiguous()
        # the drafter's side of the contract: every draft is llmie_sample_logits' pick from its draft row (no history here)
        drafts = i32([0] * (B * k))
        dp_rows = llmie.sampling_params([dict(temperature=1.0, top_k=50, seed=1000 + b) for b in range(B) for _ in range(k)])
        llmie.sample_logits(dlogits.reshape(B * k, V), dp_rows, i32([0] * (B * k)), torch.zeros(B * k, dtype=torch.uint8, device="cuda"), drafts, 7, -1)
        # (one step for all rows is not the per-position step of the contract: this is a timing, the verdicts only need to vary)
        drafts = drafts.reshape(B, k).contiguous()
        seq, fin = i32([0] * B), torch.zeros(B, dtype=torch.uint8, device="cuda")
        outs = (torch.empty((B, k + 1), dtype=torch.int32, device="cuda"), i32([0] * B))
        acc = i32([0] * B)
        ws = torch.empty(llmie.spec_verify_sampled_workspace_bytes(B, k, V), dtype=torch.uint8, device="cuda")

        def exact():
            llmie.spec_verify(logits, drafts, params, seq, fin, -1, step=7, workspace=ws, out=outs)

        def sampled():
            llmie.spec_verify_sampled(logits, dlogits, drafts, params, dparams, seq, fin, -1, step=7, workspace=ws, out=outs, out_accepted=acc)

        for _ in range(3):
            exact()
            sampled()
        torch.cuda.synchronize()
        accepted = float(acc.float().mean().item())
        te, ts = [], []
        for _ in range(rounds):
            te.append(timed(exact, reps) * 1e3)
            ts.append(timed(sampled, reps) * 1e3)
        me, ms = statistics.median(te), statistics.median(ts)
        out["arms"].append(dict(k=k, rows=T, spec_verify_us=me, spec_verify_us_min_max=[min(te), max(te)], spec_verify_sampled_us=ms,
                                spec_verify_sampled_us_min_max=[min(ts), max(ts)], sampled_over_exact=ms / me,
                                accepted_drafts_per_sequence=accepted))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--k", type=int, nargs="*", default=[2, 4, 7])
    ap.add_argument("--ctx", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--layers", type=int, default=0, help="fewer layers than the model's 32 (a rehearsal; not a measurement)")
    ap.add_argument("--sampled", action="store_true", help="the sampled-draft arm: spec_verify_sampled beside spec_verify, the entries alone")
    ap.add_argument("--tree", type=int, nargs="*", default=[], help="the tree arm: node counts n (1 .. 64) of one tree step each")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("specbench: needs a GPU (a time measured anywhere else says nothing)")
    llmie = bench.load_llmie()
    if a.sampled:
        res = dict(bench="spec_verify_sampled", device=torch.cuda.get_device_name(0), rounds=a.rounds, reps=a.reps,
                   results=[run_sampled(llmie, B, a.k, a.rounds, a.reps) for B in a.batch])
        line = json.dumps(res)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    cfg = dict(bench.LLAMA2_7B)
    if a.layers:
        cfg["num_layers"] = a.layers
    weights = bench.build_weights(torch, cfg, 0)
    res = dict(bench="spec_decode", device=torch.cuda.get_device_name(0), rounds=a.rounds, reps=a.reps, layers=cfg["num_layers"],
               results=[run_batch(llmie, cfg, weights, B, a.k, a.ctx, a.rounds, a.reps, a.tree) for B in a.batch])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
