"""Run by tests/test_score_tokens_gpu.py in a FRESH process: the very first llmie_score_tokens call this process makes (RMSNorm copy,
tile kernel, merge kernel) is recorded into a hipGraph.  An allocation or a synchronisation while the stream is capturing is an
error, so the capture succeeds only if the call does neither.  The graph is replayed twice and compared with the eager call.
Prints one JSON line."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.conftest import load_llmie  # noqa: E402

llmie = load_llmie()
DEV = "cuda"
rows, H, V = 130, 512, 1003
rng = np.random.default_rng(11)
x = torch.from_numpy(rng.standard_normal((rows, H)).astype(np.float16)).to(DEV)
w = torch.from_numpy((rng.standard_normal((V, H)) * (1.2 / np.sqrt(H))).astype(np.float16)).to(DEV)
gamma = torch.from_numpy((1.0 + 0.1 * rng.uniform(-1, 1, H)).astype(np.float16)).to(DEV)
bias = torch.from_numpy((0.5 * rng.standard_normal(V)).astype(np.float16)).to(DEV)
targets = torch.from_numpy(rng.integers(0, V, rows).astype(np.int32)).to(DEV)
ws = torch.empty(llmie.score_tokens_workspace_bytes(rows, H, V), dtype=torch.uint8, device=DEV)
lp, lse, alp = (torch.zeros(rows, dtype=torch.float32, device=DEV) for _ in range(3))
am = torch.zeros(rows, dtype=torch.int32, device=DEV)


def call(o_lp, o_lse, o_am, o_alp):
    rc = llmie.lib().llmie_score_tokens(x.data_ptr(), gamma.data_ptr(), 1e-5, w.data_ptr(), bias.data_ptr(), targets.data_ptr(),
                                        o_lp.data_ptr(), o_lse.data_ptr(), o_am.data_ptr(), o_alp.data_ptr(), rows, H, V, ws.data_ptr(),
                                        ws.numel(), llmie.F16, torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError(llmie.lib().llmie_last_error().decode())


torch.cuda.synchronize()
graph = torch.cuda.CUDAGraph()
s = torch.cuda.Stream()
with torch.cuda.graph(graph, stream=s):   # FIRST launches of this process, under capture
    call(lp, lse, am, alp)
graph.replay()
torch.cuda.synchronize()
first = [t.clone() for t in (lp, lse, am, alp)]
for t in (lp, lse, am, alp):
    t.zero_()
graph.replay()
torch.cuda.synchronize()
second = [t.clone() for t in (lp, lse, am, alp)]

eager = [torch.zeros(rows, dtype=torch.float32, device=DEV), torch.zeros(rows, dtype=torch.float32, device=DEV),
         torch.zeros(rows, dtype=torch.int32, device=DEV), torch.zeros(rows, dtype=torch.float32, device=DEV)]
call(*eager)
torch.cuda.synchronize()
print(json.dumps(dict(replay1_equal=[bool(torch.equal(a, b)) for a, b in zip(first, eager)],
                      replay2_equal=[bool(torch.equal(a, b)) for a, b in zip(second, eager)],
                      finite=bool(torch.isfinite(eager[0]).all() and torch.isfinite(eager[1]).all()),
                      logprob_min=float(eager[0].min().item()))))
