"""MLA decode attention on the GPU against a float64 reference in the UN-absorbed form (k_t = W_UK c_t || k_pe_t, v_t = W_UV c_t,
plain softmax), computed from the cache rows AS STORED by mla_kv_append, so that a wrong append and a wrong attention fail
differently.  The appended row is checked first against float64 RMSNorm / RoPE (2 fp16 ulps for c, 2 eps (|x| + |partner|) for k_pe).

Bound for o_lat and the composed output, derived: P is rounded to fp16 before the PV MFMA (2^-11 per weight, the weights sum to 1),
the output is rounded to fp16 (2^-11), and a factor 2 for the fp32 accumulation order: |err| <= 2^-10 max_t |v_t| + 2^-10 |ref| per
element (v_t = c_t for o_lat).  Inputs: latents 0.5 N(0, 1), logits of standard deviation ~2, a dominant key at ctx - 1 (head 0) and
at the first row of the last tile (head 1), a decoy row of 1e4 at slot ctx (dense) and in every page outside the block table (paged).

Measured on an MI355X, worst error / bound: 16 heads 0.356 (ctx 547), 32 heads 0.506 (ctx 128), ctx 1 exact; ragged batch 0.478
(dense = paged); chain 0.226 (o_lat) / 0.265 (out).  The ragged case is batch 4: three live contexts and one sequence at ctx_len 0.
"""
import functools
import re
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV, EPS, L, LAYER, SCALE, RMS_EPS, SENTINEL = "cuda:0", 2.0 ** -10, 2, 1, 1.0 / 6.0, 1e-6, 777.0


@pytest.fixture(scope="module")
def mla(llmie):
    llmie.build()
    m = re.search(r"tile(\d+) chunk(\d+)", llmie.mla_decode_plan(1, 16, 128)[0])
    return types.SimpleNamespace(lib=llmie, T=int(m[1]), C=int(m[2]))


def rope64(x, tab, pos):
    c, s, x0, x1 = tab[pos, :, 0], tab[pos, :, 1], x[..., :32], x[..., 32:]
    return np.concatenate([x0 * c - x1 * s, x1 * c + x0 * s], -1)


@functools.lru_cache(maxsize=None)
def make_case(llmie, T, heads, ctxs):
    """inputs of one call (numpy, fp16 values) and what the float64 algebra expects of the appended rows"""
    rng = np.random.default_rng(1000 * heads + sum(ctxs))
    f16 = lambda a: a.astype(np.float16)
    c = types.SimpleNamespace(heads=heads, ctxs=ctxs, B=len(ctxs), S=max(128, -(-max(ctxs) // 128) * 128))
    c.tab = llmie.rope_table(c.S, 64, 64, 10000.0)
    c.kv_b = f16(rng.standard_normal((heads, 256, 512)) / np.sqrt(128))
    c.q = f16(rng.standard_normal((c.B, heads, 192)))
    c.gamma = f16(1 + 0.1 * rng.uniform(-1, 1, 512))
    c.cache = f16(0.5 * rng.standard_normal((L, c.B, c.S, 576)))
    c.kv_a = f16(0.5 * rng.standard_normal((c.B, 576)))
    W, q = c.kv_b.astype(np.float64), c.q.astype(np.float64)
    q_abs = np.einsum("hnc,bhn->bhc", W[:, :128], q[:, :, :128])
    c.q_rot = np.stack([rope64(q[b, :, 128:], c.tab, max(ctx - 1, 0)) for b, ctx in enumerate(ctxs)])
    c.q_lat = f16(np.concatenate([q_abs, c.q_rot], -1))
    for b, ctx in enumerate(ctxs):
        if ctx < 1:
            continue
        unit = q_abs[b] / np.linalg.norm(q_abs[b], axis=-1, keepdims=True)
        c.kv_a[b, :512] = f16(8 * unit[0])                                 # the appended key: head 0's direction (RMSNorm sets its length)
        c.cache[LAYER, b, (ctx - 1) // T * T, :512] = f16(22.6 * unit[1])  # first row of the last tile: head 1's
        if ctx < c.S:
            c.cache[LAYER, b, ctx] = 1e4
    a = c.kv_a.astype(np.float64)
    lat, pe = a[:, :512], a[:, 512:]
    c.row_c = lat / np.sqrt((lat ** 2).mean(-1, keepdims=True) + RMS_EPS) * c.gamma.astype(np.float64)
    c.row_pe = np.stack([rope64(pe[b], c.tab, max(ctx - 1, 0)) for b, ctx in enumerate(ctxs)])
    c.pe_tol = 2 * EPS * (np.abs(pe) + np.abs(np.concatenate([pe[:, 32:], pe[:, :32]], -1)))
    return c


def reference(c, b, rows):
    """(o_lat, its bound, out, its bound) of sequence b from its stored rows [ctx, 576], float64, un-absorbed"""
    W, q, lat, pe = c.kv_b.astype(np.float64), c.q[b].astype(np.float64), rows[:, :512], rows[:, 512:]
    k_nope, v = np.einsum("tc,hnc->htn", lat, W[:, :128]), np.einsum("tc,hvc->htv", lat, W[:, 128:])
    logits = SCALE * (np.einsum("hn,htn->ht", q[:, :128], k_nope) + c.q_rot[b] @ pe.T)
    p = np.exp(logits - logits.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    o_lat, out = p @ lat, np.einsum("ht,htv->hv", p, v)
    return (o_lat, EPS * np.abs(lat).max(0) + EPS * np.abs(o_lat), out, EPS * np.abs(v).max(1) + EPS * np.abs(out))


def run(mla, c, paged, chain=False, only=None):
    """append + (absorb) + decode (+ out project) on the device; only = b: the batch-1 call of sequence b.  Checks the cache, returns
    (rows as stored [B, S, 576] float64, o_lat, out or None)"""
    llmie, sl = mla.lib, slice(None) if only is None else slice(only, only + 1)
    ctxs = c.ctxs[sl] if only is None else (c.ctxs[only],)
    B, d = len(ctxs), lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    dense, ctx_len, tab = d(c.cache[:, sl]), d(np.asarray(ctxs, np.int32)), d(c.tab)
    cache, table, kw = dense, None, {}
    if paged:   # shuffled table, two spare pages, decoys wherever no row lives
        mp = c.S // 128
        table = torch.randperm(B * mp + 2, generator=torch.Generator().manual_seed(B))[:B * mp].reshape(B, mp).to(DEV)
        cache = torch.full((L, B * mp + 2, 128, 576), 1e4, dtype=torch.float16, device=DEV)
        cache[:, table.flatten()] = dense.view(L, B * mp, 128, 576)
        table, kw = table.int().contiguous(), dict(block_table=table.int().contiguous(), max_seq_len=c.S)
    before = cache.clone()
    llmie.mla_kv_append(d(c.kv_a[sl]), d(c.gamma), RMS_EPS, tab, cache, LAYER, ctx_len, **kw)
    stored = (cache[LAYER, table.flatten().long()].view(B, c.S, 576) if paged else cache[LAYER]).double().cpu().numpy()
    patched = cache.clone()
    for b, ctx in enumerate(ctxs):   # the appended row, then: nothing else changed (dead sequences, decoys and spare pages included)
        if ctx >= 1:
            g = b if only is None else only
            err_c, err_pe = np.abs(stored[b, ctx - 1, :512] - c.row_c[g]), np.abs(stored[b, ctx - 1, 512:] - c.row_pe[g])
            assert (err_c <= 2 * EPS * np.abs(c.row_c[g]) + 2.0 ** -24).all(), "appended c of sequence %d: %g" % (b, err_c.max())
            assert (err_pe <= c.pe_tol[g] + 2.0 ** -24).all(), "appended k_pe of sequence %d: %g" % (b, err_pe.max())
            at = (int(table[b, (ctx - 1) // 128]), (ctx - 1) % 128) if paged else (b, ctx - 1)
            patched[LAYER, at[0], at[1]] = before[LAYER, at[0], at[1]]
    assert torch.equal(patched, before), "the append changed something outside the appended rows"
    q_lat = d(c.q_lat[sl])
    if chain:
        q_lat = llmie.mla_q_absorb(d(c.q[sl]), d(c.kv_b), tab, torch.full_like(q_lat, SENTINEL), ctx_len, c.S)
    o_lat = torch.full((B, c.heads, 512), SENTINEL, dtype=torch.float16, device=DEV)
    llmie.mla_decode(q_lat, cache, LAYER, ctx_len, SCALE, o_lat, llmie.mla_workspace(B, c.heads, c.S), **kw)
    out = llmie.mla_out_project(o_lat, d(c.kv_b), torch.empty((B, c.heads * 128), dtype=torch.float16, device=DEV)) if chain else None
    torch.cuda.synchronize()
    return stored, o_lat, out


def check(what, got, ref, bound):
    ratio = (np.abs(got.double().cpu().numpy().reshape(ref.shape) - ref) / bound).max()
    print("%s: worst error / bound %.3f" % (what, ratio))
    assert ratio <= 1.0, what


CONTEXTS = ("1", "T-1", "T", "T+1", "128", "129", "C", "C+1", "2*C+T+3")


@pytest.mark.parametrize("expr", CONTEXTS)
@pytest.mark.parametrize("heads", [16, 32])
def test_decode_dense_and_paged(mla, heads, expr):
    ctx = eval(expr, {"T": mla.T, "C": mla.C})
    c = make_case(mla.lib, mla.T, heads, (ctx,))
    stored, o_dense, _ = run(mla, c, paged=False)
    o_lat, bound, _, _ = reference(c, 0, stored[0, :ctx])
    check("heads %d ctx %d (%s) dense" % (heads, ctx, expr), o_dense[0], o_lat, bound)
    stored_p, o_paged, _ = run(mla, c, paged=True)
    assert np.array_equal(stored_p[0, :ctx], stored[0, :ctx]) and torch.equal(o_paged, o_dense), "paged differs from dense"


@pytest.mark.parametrize("paged", [False, True])
def test_ragged_batch_rows_equal_the_batch_1_calls(mla, paged):
    ctxs = (mla.C + 1, 0, mla.T - 1, 2 * mla.C + mla.T + 3)
    c = make_case(mla.lib, mla.T, 32, ctxs)
    stored, o, _ = run(mla, c, paged)
    assert (o[1] == SENTINEL).all(), "the sequence at ctx_len 0 was written"
    for b in (0, 2, 3):
        o_lat, bound, _, _ = reference(c, b, stored[b, :ctxs[b]])
        check("ragged row %d ctx %d paged=%s" % (b, ctxs[b], paged), o[b], o_lat, bound)
        assert torch.equal(run(mla, c, paged, only=b)[1][0], o[b]), "row %d differs from its batch-1 call" % b


def test_chain_absorb_decode_out_project(mla):
    ctx = mla.C + 1
    c = make_case(mla.lib, mla.T, 16, (ctx,))
    stored, o, out = run(mla, c, paged=False, chain=True)
    o_lat, bound, ref_out, out_bound = reference(c, 0, stored[0, :ctx])
    check("chain o_lat", o[0], o_lat, bound)
    check("chain out", out[0], ref_out, out_bound)
