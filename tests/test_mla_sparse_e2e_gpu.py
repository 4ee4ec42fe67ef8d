"""The sparse decode step end to end on the GPU: mla_index_topk's selection feeds mla_decode_sparse.  With ctx <= top_k the step is the
dense one, bit for bit; with ctx > top_k it is the float64 attention over the float64 reference's OWN top-k set -- on inputs whose
64th / 65th reference logits lie further apart than twice the logit bound B_max of tests/test_mla_sparse_gpu.py (the seed is picked by
that criterion, the gap asserted), so that the selection is unique.  Attention bound: 2^-10 max_j |row_j| + 2^-10 |ref|."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV, SCALE, EPS, SEED = "cuda:0", 1.0 / 6.0, 2.0 ** -10, 2


@pytest.mark.parametrize("ctx,top_k", [(200, 256), (700, 64)])
def test_index_then_sparse_decode(llmie, ctx, top_k):
    llmie.build()
    rng, S, heads = np.random.default_rng(SEED), 768, 16
    q_idx = rng.standard_normal((64, 128)).astype(np.float16)
    k_idx = rng.standard_normal((S, 128)).astype(np.float16)
    w_idx = (rng.standard_normal(64) / 8).astype(np.float32)
    q_lat = rng.standard_normal((1, heads, 576)).astype(np.float16)
    rows = (0.5 * rng.standard_normal((S, 576))).astype(np.float16)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    cache, lengths = d(rows[None, None]), torch.tensor([ctx], dtype=torch.int32, device=DEV)
    sel, cnt = torch.full((1, top_k), -7, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    llmie.mla_index_topk(d(q_idx[None]), d(w_idx[None]), d(k_idx[None, None]), 0, lengths, sel, cnt, llmie.mla_index_workspace(1, S))
    o_lat = torch.full((1, heads, 512), 777.0, dtype=torch.float16, device=DEV)
    llmie.mla_decode_sparse(d(q_lat), cache, 0, lengths, sel, cnt, SCALE, o_lat, llmie.mla_workspace(1, heads, top_k))
    if ctx <= top_k:
        dense = llmie.mla_decode(d(q_lat), cache, 0, lengths, SCALE, torch.full_like(o_lat, 777.0), llmie.mla_workspace(1, heads, S))
        assert int(cnt) == ctx and torch.equal(o_lat, dense)
        return
    q64, k64, w64 = q_idx.astype(np.float64), k_idx[:ctx].astype(np.float64), w_idx.astype(np.float64)
    ref = np.maximum(k64 @ q64.T, 0) @ w64
    b_max = (2.0 ** -15 * (np.abs(k64) @ np.abs(q64).T) @ np.abs(w64)).max()
    order = np.sort(ref)
    assert order[-top_k] - order[-top_k - 1] > 2 * b_max, "the seed no longer separates the top_k-th from the next logit"
    want = np.sort(np.argsort(ref)[-top_k:])
    assert int(cnt) == top_k and (sel[0].cpu().numpy() == want).all()
    picked = rows[want].astype(np.float64)
    s = SCALE * q_lat[0].astype(np.float64) @ picked.T
    p = np.exp(s - s.max(-1, keepdims=True))
    o = (p / p.sum(-1, keepdims=True)) @ picked[:, :512]
    ratio = (np.abs(o_lat[0].double().cpu().numpy() - o) / (EPS * np.abs(picked[:, :512]).max(0) + EPS * np.abs(o))).max()
    print("sparse step ctx %d top_k %d: worst error / bound %.3f" % (ctx, top_k, ratio))
    assert ratio <= 1.0
