"""Run by tests/test_moe_mxfp4_engine_gpu.py in a FRESH process: one decode step of an engine with MXFP4 experts and the gpt-oss
epilogue is recorded into a graph (the first launches this process makes of the moe sequence: nothing on it may allocate or read
back).  The SAME graph must serve other hidden rows that route differently: each replay is compared bit for bit with the eager call.
Six rows on an engine attached under LLMIE_MOE_FORCE_GROUPED take the grouped route, three rows on a second engine the GEMV route.
Prints one JSON line."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tests.conftest import load_llmie  # noqa: E402
import moe_engine_cases as me  # noqa: E402
import mxfp4_cases as mx  # noqa: E402

llmie = load_llmie()
DEV, F16 = me.DEV, me.F16
hs, E, k, step = 64, 8, 2, 131
w = me.layer_weights(hs, 1, E, seed=17)
rng = np.random.default_rng(3)
d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
gq, gs = mx.quantize(w[0]["e_gate_up"].reshape(E * 2 * me.IE, me.H))
dq, ds = mx.quantize(w[0]["e_down"].reshape(E * me.H, me.IE))
router_bias = d((0.5 * rng.standard_normal(E)).astype(np.float16))
ex = llmie.MoeExperts(d(w[0]["router"]), d(gq.reshape(E, 2 * me.IE, me.H // 2)), d(dq.reshape(E, me.H, me.IE // 2)),
                      gate_up_scale=d(gs.reshape(E, 2 * me.IE, me.H // 32)), down_scale=d(ds.reshape(E, me.H, me.IE // 32)), router_bias=router_bias,
                      gate_up_bias=d((0.25 * rng.standard_normal((E, 2 * me.IE))).astype(np.float16)),
                      down_bias=d((0.5 * rng.standard_normal((E, me.H))).astype(np.float16)), act=llmie.MOE_ACT_SWIGLU_CLAMPED, alpha=1.702, limit=7.0)
probe = me.make_engine(llmie, w, hs, zero_down=True)   # its output is the residual stream in front of the FFN norm
g = torch.Generator().manual_seed(8)
equal, routes_differ = [], []
for bs, flags in ((6, llmie.MOE_FORCE_GROUPED), (3, 0)):
    dec = me.make_engine(llmie, w, hs)
    dec.moe_attach([ex], k, flags=flags, max_tokens=me.MAX_BATCH)
    assert ("route=grouped" if bs == 6 else "route=gemv") in llmie.moe_ffn_plan_ex(bs, me.H, me.IE, E, k, flags, llmie.W_MXFP4, 1)
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
        ids.append(llmie.moe_route_ex(r, ex, k)[0].cpu())
    routes_differ.append(not torch.equal(ids[0], ids[1]))
    dec.close()
probe.close()
print(json.dumps(dict(equal=equal, routes_differ=routes_differ)))
