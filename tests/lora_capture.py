"""Run by tests/test_lora_engine_gpu.py in a FRESH process: one decode step of an engine with an adapter table attached is recorded
into a graph (the first launches this process makes of the lora sequence: nothing on it may allocate).  The slot table and the
per-sequence slot array live in device memory, so the SAME graph must serve a new adapter mix and a slot reloaded with another
adapter: each replay is compared bit for bit with the eager call.  Prints one JSON line."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tests.conftest import load_llmie  # noqa: E402
import lora_engine_cases as lc  # noqa: E402

llmie = load_llmie()
DEV, F16 = lc.DEV, lc.F16
hs, bs, step = 64, 4, 131
base, ads = lc.base_weights(hs), lc.adapters(hs)
dec, table, seq_slot = lc.lora_engine(llmie, base, ads, hs, False, max_tokens=lc.MAX_BATCH)
g = torch.Generator().manual_seed(8)
k0 = (torch.randn((lc.LAYERS, bs, lc.KVH, lc.MAX_SEQ, hs), generator=g) * 0.5).to(DEV).to(F16)
v0 = (torch.randn((lc.LAYERS, bs, lc.KVH, lc.MAX_SEQ, hs), generator=g) * 0.5).to(DEV).to(F16)
x = torch.randn((bs, lc.NH * hs), generator=g).to(DEV).to(F16)
step_dev = torch.tensor([step], dtype=torch.int32, device=DEV)
seq_slot[:bs] = torch.tensor([1, -1, 0, 2], dtype=torch.int32, device=DEV)

y, kc, vc = torch.zeros_like(x), k0.clone(), v0.clone()
torch.cuda.synchronize()
graph = torch.cuda.CUDAGraph()
s = torch.cuda.Stream()
with torch.cuda.graph(graph, stream=s):
    dec.forward(x, y, kc, vc, -1, step_dev=step_dev)


def replay():
    kc.copy_(k0), vc.copy_(v0)
    graph.replay()
    torch.cuda.synchronize()
    return y.clone()


def eager():
    out = dec.forward(x, torch.zeros_like(x), k0.clone(), v0.clone(), -1, step_dev=step_dev)
    torch.cuda.synchronize()
    return out


got = [replay()]
want = [eager()]
seq_slot[:bs] = torch.tensor([2, 0, -1, 1], dtype=torch.int32, device=DEV)   # a new adapter mix
got.append(replay())
want.append(eager())
lc.load_slot(llmie, table, 2, ads[0])                                        # a live slot reloaded with another adapter
torch.cuda.synchronize()
got.append(replay())
want.append(eager())
dec.close()
print(json.dumps(dict(equal=[bool(torch.equal(a, b)) for a, b in zip(got, want)],
                      distinct=[not torch.equal(got[0], got[1]), not torch.equal(got[1], got[2])])))
