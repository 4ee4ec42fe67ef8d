"""Tree attention in prefill (csrc/prefill.hip: the TREE instantiations of prefill_rope_append_kernel and prefill_flash_kernel) with
inputs that can fail.  Cases, planted rows and the float64 reference come from tests/spec_tree_attn_cases.py; tests/
test_spec_tree_cpu.py shows on the CPU that every owner holds its mass and that the planted defects -- a sibling let through, a
depth-for-index RoPE position, a 32-bit shift, the self bit dropped -- are rejected by the same comparison.

Each case runs Decoder.prefill and Decoder.prefill_paged (shuffled block table, spare pages) with the tree set, on a model whose QKV
weight columns ARE the nodes' q / k / v rows.  Per pass, first the caches: the appended rows of EVERY layer -- K rotated at
history + depth, stored at history + index -- against the CPU rows, every other byte unchanged; then the attention against the
float64 reference computed from the rows AS STORED.  Bound: BOUNDS["rope"][F16] of tests/attn_cases.py.

Chain = plain, bit for bit: with the chain tree set, hidden_out and both caches equal the same call without a tree wherever that
call plans q64w4t1 (asserted from the plan text).
"""
import numpy as np
import pytest
import torch

import spec_tree_attn_cases as tc
from attn_cases import E4M3

pytestmark = pytest.mark.gpu
DEV, F16 = "cuda", torch.float16
PAGED, RAGGED, QK_NORM, TREE = 1, 2, 8192, 16384
_ENGINE = {}


def _engine(llmie, c):
    key = (c.L, c.kv, c.max_seq, c.bs)
    if _ENGINE.get("key") != key:
        if "dec" in _ENGINE:
            _ENGINE.pop("dec").close()
            _ENGINE.clear()
        QKV = (tc.NH + 2 * tc.KVH) * tc.HS
        z = lambda *shape: torch.zeros(shape, dtype=F16, device=DEV)
        layers = [dict(attn_norm=torch.ones(tc.H, dtype=F16, device=DEV), ffn_norm=torch.ones(tc.H, dtype=F16, device=DEV), qkv=dict(data=z(QKV, tc.H)),
                       o=dict(data=torch.eye(tc.H, dtype=F16, device=DEV) if l == c.layer else z(tc.H, tc.H)), gate_up=dict(data=z(2 * tc.INTER, tc.H)),
                       down=dict(data=(torch.randn((tc.H, tc.INTER), device=DEV) * 0.05).to(F16))) for l in range(c.L)]
        _ENGINE.update(key=key, layers=layers, dec=llmie.Decoder(c.config(llmie), layers))
    for l, lw in enumerate(_ENGINE["layers"]):
        wq = lw["qkv"]["data"]
        wq.zero_()
        wq[:, :c.T] = torch.from_numpy(np.ascontiguousarray(c.w[l].reshape(c.T, -1).T)).to(DEV).to(F16)
    dec = _ENGINE["dec"]
    dec.set_tree(None, None)
    if c.qkn:
        g = torch.from_numpy(c.gamma).to(DEV).to(F16)
        dec.set_qk_norm(g, g.clone(), tc.QK_EPS)
    else:
        dec.set_qk_norm(None, None)
    return dec


def _dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if t.dtype == torch.uint8 else t.to(F16)


def _pool(dense, perm, filler):
    L, bs, kvh, max_seq, hs = dense.shape
    mp = perm.shape[1]
    pool = filler.clone()
    pool[:, perm.flatten().long()] = dense.view(L, bs, kvh, mp, 128, hs).permute(0, 1, 3, 2, 4, 5).reshape(L, bs * mp, kvh, 128, hs)
    return pool


def _unpool(pool, perm, bs):
    L, _, kvh, _, hs = pool.shape
    mp = perm.shape[1]
    return pool[:, perm.flatten().long()].view(L, bs, mp, kvh, 128, hs).permute(0, 1, 3, 2, 4, 5).reshape(L, bs, kvh, mp * 128, hs)


def _check_caches(c, form, after, before):
    """the appended rows of every layer (K rotated at history + depth, stored at history + index), everything else unchanged -> the
    values the pass left"""
    seq, pos = torch.from_numpy(c.seq_of).to(DEV), torch.from_numpy(c.slot_of).to(DEV)
    vals = []
    for which, name, new in ((0, "K", c.k_new), (1, "V", c.v_new)):
        got, exp = after[which], before[which].clone()
        exp[:, seq, :, pos] = got[:, seq, :, pos]
        assert torch.equal(got, exp), "%s %s: %s cache changed outside the appended slots, first at %s" % (c.cid, form, name, (got != exp).nonzero()[0].tolist())
        for l in range(c.L):
            rows = got[l, seq, :, pos].cpu().numpy()
            what = "%s %s: appended %s rows of layer %d" % (c.cid, form, name, l)
            if c.scales is None:
                err = np.abs(rows.astype(np.float64) - new[l])
                tol = c.k_tol[l] if which == 0 else 0.0
                if not (err <= tol).all():
                    t, g, d = np.unravel_index(np.argmax(err - tol), err.shape)
                    raise AssertionError("%s: node %d of sequence %d (slot %d, rotated at %d) kv_head=%d dim=%d is %r, expected %r" % (
                        what, t % c.n, c.seq_of[t], c.slot_of[t], c.rpos_of[t], g, d, float(rows[t, g, d]), float(new[l][t, g, d])))
            else:   # the neighbouring code where the device's fp16 value fell on the other side of a rounding boundary (tests/test_prefill_attn_gpu.py)
                scale = c.scales[which]
                a, b = E4M3[rows].astype(np.float64) * scale, E4M3[new[l]].astype(np.float64) * scale
                assert (rows != new[l]).mean() < 0.02, "%s: codes differ in %.3f of the elements" % (what, (rows != new[l]).mean())
                tol = 0.126 * np.abs(b) + scale * 2.0 ** -9 + 2.0 ** -9 * np.abs(b).max(axis=-1, keepdims=True)
                assert (np.abs(a - b) <= tol).all(), "%s: worst excess %.3g" % (what, (np.abs(a - b) - tol).max())
        vals.append(c.deq(got.cpu().numpy(), which))
    return vals


def _passes(llmie, dec, c, x, before, lens, hist):
    """(layout, hidden_out, dense views of the caches after the pass) for the dense and the paged entry"""
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    out = torch.full_like(x, 9.0)
    kd, vd = before[0].clone(), before[1].clone()
    dec.prefill(x, out, kd, vd, lens, hist, c.n)
    torch.cuda.synchronize()
    yield "dense", out, (kd, vd)
    rng = np.random.default_rng(5)
    mp = c.max_seq // 128
    num_pages = c.bs * mp + 2
    perm = i32(rng.permutation(num_pages)[:c.bs * mp].reshape(c.bs, mp))
    shape = (c.L, num_pages, tc.KVH, 128, tc.HS)
    fill = lambda: torch.randint(0, 0x58, shape, device=DEV, dtype=torch.uint8) if c.scales else (torch.randn(shape, device=DEV) * 0.5).to(F16)
    fillers = (fill(), fill())
    kp, vp = _pool(before[0], perm, fillers[0]), _pool(before[1], perm, fillers[1])
    out = torch.full_like(x, 9.0)
    dec.prefill_paged(x, out, kp, vp, perm, lens, hist, c.n)
    torch.cuda.synchronize()
    after = (_unpool(kp, perm, c.bs), _unpool(vp, perm, c.bs))
    for name, pool, a, f in (("K", kp, after[0], fillers[0]), ("V", vp, after[1], fillers[1])):
        assert torch.equal(pool, _pool(a, perm, f)), "%s paged: %s pool changed outside the block table's pages" % (c.cid, name)
    yield "paged", out, after


@pytest.mark.parametrize("tree,kv,qkn", tc.CASES, ids=tc.CASE_IDS)
def test_tree_attention(llmie, tree, kv, qkn):
    c = tc.make_case(tree, kv, qkn)
    dec = _engine(llmie, c)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    lens, hist = i32(c.lens), i32(c.hist)
    depth = i32(np.tile(np.asarray(c.depth, np.int32), (c.bs, 1)))
    anc = torch.from_numpy(np.tile(tc.anc_i64(c.anc), (c.bs, 1))).to(DEV)
    # the prepare kernel gives the same arrays (its own test: tests/test_spec_verify_tree_gpu.py)
    d2, a2 = llmie.spec_tree_prepare(i32(np.tile(np.asarray(c.parent, np.int32), (c.bs, 1))), None if c.count is None else i32([c.count] * c.bs))
    assert torch.equal(d2, depth) and torch.equal(a2, anc)
    x = torch.zeros((c.T, tc.H), dtype=F16, device=DEV)
    x[torch.arange(c.T), torch.arange(c.T)] = tc.X_ONE_HOT
    before = (_dev(c.k0), _dev(c.v0))
    text, _ = llmie.decoder_prefill_layer_plan(c.config(llmie), c.T, c.bs, c.n, call_flags=TREE | RAGGED | (QK_NORM if qkn else 0))
    assert text is not None and "attn=q64w4t1" in text and text.endswith(" tree") and "rope_append=1" in text, text
    dec.set_tree(depth, anc)
    ratios = {}
    try:
        for layout, out, after in _passes(llmie, dec, c, x, before, lens, hist):
            kf, vf = _check_caches(c, layout, after, before)
            ref, mass = tc.reference(c, kf, vf, with_mass=True)
            tc.assert_mass(c, mass)
            attn = (out.double() - x.double()).cpu().numpy()
            ratios[layout] = tc.check_case([attn[s * c.n:(s + 1) * c.n] for s in range(c.bs)], c, layout, exp=ref)
    finally:
        dec.set_tree(None, None)
        dec.set_qk_norm(None, None)
    print("%s: error / bound dense %.3f paged %.3f" % (c.cid, ratios["dense"], ratios["paged"]))


@pytest.mark.parametrize("n", [1, 16, 64])
@pytest.mark.parametrize("kv", ["f16", "pow2"])
def test_chain_tree_equals_plain_bit_for_bit(llmie, n, kv):
    """random rows (nothing planted matters here): the chain tree selects the keys of the causal mask and rotates at the same rows,
    and the two-launch RoPE form is bit-identical to the fused one; batch 3 on histories 0, 37, 128, dense and paged"""
    parent = [-1] + list(range(n - 1))
    tc.TREES["chain%d" % n] = (parent, None)
    try:
        c = tc.make_case("chain%d" % n, kv, False)
    finally:
        del tc.TREES["chain%d" % n]
    dec = _engine(llmie, c)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    lens, hist = i32(c.lens), i32(c.hist)
    plain, _ = llmie.decoder_prefill_layer_plan(c.config(llmie), c.T, c.bs, c.n, call_flags=RAGGED)
    assert "attn=q64w4t1" in plain.split(" "), plain   # the shapes where the plain plan runs the form the tree form was cut from
    d, a = tc.chain_ref(n)
    depth, anc = i32(np.tile(np.asarray(d, np.int32), (c.bs, 1))), torch.from_numpy(np.tile(tc.anc_i64(a), (c.bs, 1))).to(DEV)
    x = torch.zeros((c.T, tc.H), dtype=F16, device=DEV)
    x[torch.arange(c.T), torch.arange(c.T)] = tc.X_ONE_HOT
    before = (_dev(c.k0), _dev(c.v0))
    runs = {}
    for with_tree in (True, False):
        dec.set_tree(depth, anc) if with_tree else dec.set_tree(None, None)
        try:
            runs[with_tree] = [(layout, out, after) for layout, out, after in _passes(llmie, dec, c, x, before, lens, hist)]
        finally:
            dec.set_tree(None, None)
    for (layout, o1, a1), (_, o0, a0) in zip(runs[True], runs[False]):
        assert torch.equal(o1, o0), "%s n=%d %s: hidden_out differs at %s" % (kv, n, layout, (o1 != o0).nonzero()[0].tolist())
        assert torch.equal(a1[0], a0[0]) and torch.equal(a1[1], a0[1]), "%s n=%d %s: the caches differ" % (kv, n, layout)
    assert not torch.equal(runs[True][0][1], torch.full_like(x, 9.0))


def test_set_tree_refusals(llmie):
    c = tc.make_case("chain2", "f16", False)
    dec = _engine(llmie, c)
    depth = torch.zeros((c.bs, 2), dtype=torch.int32, device=DEV)
    anc = torch.ones((c.bs, 2), dtype=torch.int64, device=DEV)
    lib, h = llmie.lib(), dec.handle
    err = lambda: lib.llmie_last_error().decode()
    p = lambda t: t.data_ptr()
    assert lib.llmie_decoder_set_tree(h, p(depth), None, 2) == -1 and "go together" in err()
    assert lib.llmie_decoder_set_tree(h, None, p(anc), 2) == -1 and "go together" in err()
    for stride in (0, 65, -1):
        assert lib.llmie_decoder_set_tree(h, p(depth), p(anc), stride) == -1 and "stride" in err()
    dec.set_window(64)
    assert lib.llmie_decoder_set_tree(h, p(depth), p(anc), 2) == -2 and "draft tree" in err()
    dec.set_window(None)
    sinks = torch.zeros((c.L, tc.NH), dtype=torch.float32, device=DEV)
    dec.set_head_sinks(sinks)
    assert lib.llmie_decoder_set_tree(h, p(depth), p(anc), 2) == -2 and "draft tree" in err()
    dec.set_head_sinks(None)
    dec.set_tree(depth, anc)
    try:
        with pytest.raises(llmie.LlmieError, match="draft tree"):
            dec.set_window(64)
        with pytest.raises(llmie.LlmieError, match="draft tree"):
            dec.set_head_sinks(sinks)
        # a call longer than the stride is refused, with nothing written
        x = torch.zeros((3, tc.H), dtype=F16, device=DEV)
        out = torch.full_like(x, 9.0)
        k, v = _dev(c.k0[:, :1]), _dev(c.v0[:, :1])
        k0 = k.clone()
        with pytest.raises(llmie.LlmieError, match="stride"):
            dec.prefill(x, out, k, v, torch.tensor([3], dtype=torch.int32, device=DEV), torch.tensor([0], dtype=torch.int32, device=DEV), 3)
        torch.cuda.synchronize()
        assert torch.equal(k, k0) and (out == 9.0).all()
    finally:
        dec.set_tree(None, None)
