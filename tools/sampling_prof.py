"""Device time of the per-request sampler (llmie_sample_logits), one configuration per process so that a
`rocprofv3 --kernel-trace --stats` run attributes every sample_params_kernel launch to it (tools/sampling_prof.sh runs them).

    python tools/sampling_prof.py <all|greedy|top_p|tail|ext_mask|ext_all|ext_top> <batch> [iters]

all: temperature 0.8, top_k 50, top_p 0.9, min_p 0.02, the three penalties over a 64-id history;  greedy: temperature 0;
top_p: top_p 0.9 alone;  tail: the existing top-4 tail (llmie_topk round 1 + round 2, llmie_sampling) on the same rows.
ext_*: llmie_sample_logits_ext on the parameters of "all" -- ext_mask: an allowed-token mask per row (half the tokens) alone;
ext_all: the mask, 300 bias entries per row and top_n = 20;  ext_top: top_n = 20 alone.
V = 32000, fp16 logits."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

CONFIGS = {
    "all": dict(temperature=0.8, top_k=50, top_p=0.9, min_p=0.02, repetition_penalty=1.1, presence_penalty=0.1,
                frequency_penalty=0.05),
    "greedy": dict(temperature=0.0),
    "top_p": dict(top_p=0.9),
}


def main():
    kind, bs = sys.argv[1], int(sys.argv[2])
    iters = int(sys.argv[3]) if len(sys.argv) > 3 else 50
    llmie = g._load()
    V = 32000
    rng = np.random.default_rng(0)
    logits = torch.from_numpy((rng.standard_normal((bs, V)) * 3).astype(np.float16)).cuda()
    seq = torch.zeros(bs, dtype=torch.int32, device="cuda")
    fin = torch.zeros(bs, dtype=torch.uint8, device="cuda")
    out = torch.empty(bs, dtype=torch.int32, device="cuda")
    if kind == "tail":
        K = 4
        tid = torch.empty((bs, 8, K), dtype=torch.int32, device="cuda")
        tv = torch.empty((bs, 8, K), dtype=torch.float16, device="cuda")
        ids = torch.empty((bs, K), dtype=torch.int32, device="cuda")
        vals = torch.empty((bs, K), dtype=torch.float16, device="cuda")
        for i in range(iters):
            llmie.topk(logits, tid, tv, ids, vals)
            llmie.sampling(ids, vals, seq, fin, out, i, 2, V)
    else:
        ext = None
        if kind.startswith("ext_"):
            masks = rng.random((bs, V)) < 0.5 if kind in ("ext_mask", "ext_all") else None
            bias = [[(int(t), float(v)) for t, v in zip(rng.integers(0, V, 300), rng.standard_normal(300))]
                    for _ in range(bs)] if kind == "ext_all" else None
            ext = llmie.sampling_ext(bs, V, masks=masks, bias=bias, top_n=0 if kind == "ext_mask" else 20)
            kind = "all"
        params = llmie.sampling_params([dict(CONFIGS[kind], seed=b) for b in range(bs)])
        hist = torch.from_numpy(rng.integers(0, V, (bs, 64)).astype(np.int32)).cuda()
        hlen = torch.full((bs,), 64, dtype=torch.int32, device="cuda")
        lp = torch.empty(bs, dtype=torch.float32, device="cuda")
        ws = torch.empty(llmie.sample_logits_workspace_bytes(bs, V), dtype=torch.uint8, device="cuda")
        for i in range(iters):
            llmie.sample_logits(logits, params, seq, fin, out, i, 2, history=hist, history_len=hlen, out_logprob=lp, workspace=ws,
                                ext=ext)
    torch.cuda.synchronize()
    print(sys.argv[1], bs, "ok", out[:4].tolist())


if __name__ == "__main__":
    main()
