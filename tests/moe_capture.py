"""Run by tests/test_moe_engine_gpu.py in a FRESH process: one decode step of an engine with experts is recorded into a graph (the
first launches this process makes of the moe sequence: nothing on it may allocate or read back).  Expert ids, weights, the tile list
and the tile count live in device memory, so the SAME graph must serve other hidden rows that route differently: each replay is
compared bit for bit with the eager call.  Six rows take the grouped route, three the GEMV route.  Prints one JSON line."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tests.conftest import load_llmie  # noqa: E402
import moe_engine_cases as me  # noqa: E402

llmie = load_llmie()
DEV, F16 = me.DEV, me.F16
hs, E, k, step = 64, 8, 2, 131
w = me.layer_weights(hs, 1, E, seed=17)
dec = me.moe_engine(llmie, w, (True,), hs, k, max_tokens=me.MAX_BATCH)
probe = me.make_engine(llmie, w, hs, zero_down=True)   # its output is the residual stream in front of the FFN norm
g = torch.Generator().manual_seed(8)
equal, routes_differ = [], []
for bs in (6, 3):
    k0 = (torch.randn((1, bs, 2, me.MAX_SEQ, hs), generator=g) * 0.5).to(DEV).to(F16)
    v0 = (torch.randn((1, bs, 2, me.MAX_SEQ, hs), generator=g) * 0.5).to(DEV).to(F16)
    xs = [torch.randn((bs, me.H), generator=g).to(DEV).to(F16) for _ in range(2)]
    step_dev = torch.tensor([step], dtype=torch.int32, device=DEV)
    x, y, kc, vc = xs[0].clone(), torch.zeros_like(xs[0]), k0.clone(), v0.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.graph(graph, stream=s):
        dec.forward(x, y, kc, vc, -1, step_dev=step_dev)
    ids = []
    for i, xi in enumerate(xs):
        x.copy_(xi), kc.copy_(k0), vc.copy_(v0)
        graph.replay()
        torch.cuda.synchronize()
        want = dec.forward(xi, torch.zeros_like(xi), k0.clone(), v0.clone(), -1, step_dev=step_dev)
        torch.cuda.synchronize()
        if bs == 6 or i == 1:
            equal.append(bool(torch.equal(y, want)) and float(want.float().abs().sum()) > 0)
        r = probe.forward(xi, torch.zeros_like(xi), k0.clone(), v0.clone(), -1, step_dev=step_dev)
        llmie.rmsnorm(r, torch.empty_like(r), torch.from_numpy(w[0]["ffn_norm"]).to(DEV), 1e-5)
        ids.append(llmie.moe_route(r, torch.from_numpy(w[0]["router"]).to(DEV), k)[0].cpu())
    routes_differ.append(not torch.equal(ids[0], ids[1]))
dec.close()
probe.close()
print(json.dumps(dict(equal=equal, routes_differ=routes_differ)))
