"""Prefill attention (csrc/prefill.hip: the six instantiations of prefill_flash_kernel and the three producers of the K / V rows it
reads -- splitk_finalize_qkv_rope, prefill_rope_append_kernel, the QKV GEMM's fused epilogue) with inputs that can fail.

Cases, planted rows and the float64 reference come from tests/prefill_attn_cases.py; tests/test_prefill_attn_cases_cpu.py shows on
the CPU that the table reaches every form, that the bound used here is met by the oracle's composition of the same attention, and
that seeded defects are rejected by the same comparison.

The kernel has no entry of its own: each case runs Decoder.prefill and Decoder.prefill_paged (shuffled block table, spare pages,
random bytes wherever no row lives) on a model whose QKV weight columns ARE the tokens' q / k / v rows, o = identity and gate_up = 0,
so that hidden_out - hidden_in is the attention output.  Per pass, first the caches: the appended rows of EVERY layer against the
CPU rows (fp16: 2 eps (|x| + |partner|) for k, exact for v; e4m3: within one code, fewer than 2 % of the codes differing), every
other byte -- other slots, the slot past the context that holds a decoy, pages outside the block table -- unchanged.  Then the
attention, against the float64 reference computed from the rows AS STORED: a wrong append and a wrong attention fail differently.
"""
import numpy as np
import pytest
import torch

import prefill_attn_cases as pc

pytestmark = pytest.mark.gpu
DEV, F16 = "cuda", torch.float16
PAGED, RAGGED = 1, 2   # call flags of llmie_decoder_prefill_layer_plan (include/llmie.h)
_ENGINE = {}


def _engine(llmie, c):
    """one engine per (heads, layers, cache format, slab, batch), its weight tensors rewritten in place for every case (prefill reads
    the row-major originals)"""
    key = (c.nh, c.kvh, c.L, c.kv, c.max_seq, c.bs)
    if _ENGINE.get("key") != key:
        if "dec" in _ENGINE:
            _ENGINE.pop("dec").close()
            _ENGINE.clear()
        H, QKV = c.H, (c.nh + 2 * c.kvh) * pc.HS
        z = lambda *shape: torch.zeros(shape, dtype=F16, device=DEV)
        layers = [dict(attn_norm=torch.ones(H, dtype=F16, device=DEV), ffn_norm=torch.ones(H, dtype=F16, device=DEV), qkv=dict(data=z(QKV, H)),
                       # o = 0 in front of the measured layer (such a layer is the identity), o = identity in it
                       o=dict(data=torch.eye(H, dtype=F16, device=DEV) if l == c.layer else z(H, H)), gate_up=dict(data=z(2 * pc.INTER, H)),
                       down=dict(data=(torch.randn((H, pc.INTER), device=DEV) * 0.05).to(F16))) for l in range(c.L)]
        _ENGINE.update(key=key, layers=layers, dec=llmie.Decoder(c.config(llmie), layers))
    for l, lw in enumerate(_ENGINE["layers"]):
        wq = lw["qkv"]["data"]
        wq.zero_()
        wq[:, :c.T] = torch.from_numpy(np.ascontiguousarray(c.w[l].reshape(c.T, -1).T)).to(DEV).to(F16)
    return _ENGINE["dec"]


def _dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if t.dtype == torch.uint8 else t.to(F16)


def _pool(dense, perm, filler):
    """dense [L, bs, kvh, max_seq, hs] (max_seq a multiple of 128) -> pool [L, num_pages, kvh, 128, hs] under the block table perm
    [bs, max_pages]; pages outside the table hold `filler`"""
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
    """`after`, `before`: dense views [L, bs, kvh, max_seq, hs] of both caches (K, V) behind / in front of the pass -> the values the
    pass left, as numpy"""
    seq, pos = torch.from_numpy(c.seq_of).to(DEV), torch.from_numpy(c.pos_of).to(DEV)
    vals = []
    for which, name, new in ((0, "K", c.k_new), (1, "V", c.v_new)):
        got, exp = after[which], before[which].clone()
        exp[:, seq, :, pos] = got[:, seq, :, pos]
        if not torch.equal(got, exp):
            raise AssertionError("%s: %s cache changed outside the appended slots, first at [layer, sequence, kv_head, slot, dim] = %s" % (
                _words(c, form), name, (got != exp).nonzero()[0].tolist()))
        for l in range(c.L):
            rows = got[l, seq, :, pos].cpu().numpy()                 # [T, kvh, hs] as stored
            what = "%s: appended %s rows of layer %d" % (_words(c, form), name, l)
            if c.scales is None:
                err = np.abs(rows.astype(np.float64) - new[l])
                tol = c.k_tol[l] if which == 0 else 0.0
                if not (err <= tol).all():
                    t, g, d = np.unravel_index(np.argmax(err - tol), err.shape)
                    raise AssertionError("%s: packed token %d (sequence %d, slot %d) kv_head=%d dim=%d is %r, expected %r" % (
                        what, t, c.seq_of[t], c.pos_of[t], g, d, float(rows[t, g, d]), float(new[l][t, g, d])))
            else:
                # the neighbouring code where the device's fp16 value fell on the other side of a rounding boundary (one e4m3 step =
                # 2^-3 relative; + two fp16 ulps at the row's magnitude: near zero that difference spans several of the small codes)
                scale = c.scales[which]
                a, b = pc.E4M3[rows].astype(np.float64) * scale, pc.E4M3[new[l]].astype(np.float64) * scale
                assert (rows != new[l]).mean() < 0.02, "%s: codes differ in %.3f of the elements" % (what, (rows != new[l]).mean())
                tol = 0.126 * np.abs(b) + scale * 2.0 ** -9 + 2.0 ** -9 * np.abs(b).max(axis=-1, keepdims=True)
                assert (np.abs(a - b) <= tol).all(), "%s: worst excess %.3g" % (what, (np.abs(a - b) - tol).max())
        vals.append(c.deq(got.cpu().numpy(), which))
    return vals


def _words(c, form):
    return "case=%s form=%s" % (c.cid, form)


@pytest.mark.parametrize("entry", pc.TABLE, ids=pc.IDS)
def test_prefill_attention(llmie, entry):
    """Bound: the fp16 attention bound (3e-3, 2e-3) plus one fp16 ulp of |x| on the one element per row that the residual add rounds
    again.  Measured on an MI355X, largest error / bound per form, dense = paged to three digits: q64w4t1 0.484 (fp16 cache) / 0.483
    (e4m3), q128w4t2 0.483 / 0.484, q128w8t1 0.483 / 0.483 -- all of it the rounding of 64 + attention at the residual's element (half an
    ulp of 64 is 0.484 of the bound there).  Away from that element: q64w4t1 0.119 / 0.112, q128w4t2 0.104 / 0.112, q128w8t1 0.116 /
    0.120, which is what the oracle's composition reaches on the CPU (0.119: the fp16 rounding of the output)."""
    c = pc.build(entry)
    dec = _engine(llmie, c)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    lens, hist = i32(c.lens), i32(c.hist)
    x = torch.zeros((c.T, c.H), dtype=F16, device=DEV)
    x[torch.arange(c.T), torch.arange(c.T)] = pc.X_ONE_HOT
    before = (_dev(c.k0), _dev(c.v0))
    ratios = {}
    for layout in ("dense", "paged"):
        text, _ = llmie.decoder_prefill_layer_plan(c.config(llmie), c.T, c.bs, c.max_q_len,
                                                   call_flags=(PAGED if layout == "paged" else 0) | (RAGGED if c.bs > 1 else 0))
        assert text is not None and all(w in text.split(" ") for w in c.plan_words()), (c.cid, text)
        form = "%s %s kv=%s producer=%s" % (layout, c.form, c.kv, c.producer)
        out = torch.full_like(x, 9.0)
        if layout == "dense":
            kd, vd = before[0].clone(), before[1].clone()
            dec.prefill(x, out, kd, vd, lens, hist, c.max_q_len)
            torch.cuda.synchronize()
            after = (kd, vd)
        else:
            rng = np.random.default_rng(5)
            mp = c.max_seq // 128
            num_pages = c.bs * mp + 2
            perm = i32(rng.permutation(num_pages)[:c.bs * mp].reshape(c.bs, mp))
            shape = (c.L, num_pages, c.kvh, 128, pc.HS)
            fill = lambda: torch.randint(0, 0x58, shape, device=DEV, dtype=torch.uint8) if c.scales else (torch.randn(shape, device=DEV) * 0.5).to(F16)
            fillers = (fill(), fill())
            kp, vp = _pool(before[0], perm, fillers[0]), _pool(before[1], perm, fillers[1])
            dec.prefill_paged(x, out, kp, vp, perm, lens, hist, c.max_q_len)
            torch.cuda.synchronize()
            after = (_unpool(kp, perm, c.bs), _unpool(vp, perm, c.bs))
            for name, pool, a, f in (("K", kp, after[0], fillers[0]), ("V", vp, after[1], fillers[1])):   # nothing outside the table's pages
                assert torch.equal(pool, _pool(a, perm, f)), "%s: %s pool changed outside the block table's pages" % (_words(c, form), name)
        kf, vf = _check_caches(c, form, after, before)
        ref, mass = pc.reference(c, kf, vf, with_mass=True)
        pc.assert_mass(c, mass)
        attn = (out.double() - x.double()).cpu().numpy()
        per_seq = [attn[c.cum[s]:c.cum[s + 1]] for s in range(c.bs)]
        ratios[layout] = (pc.check_case(per_seq, c, form, exp=ref), pc.attention_ratio(per_seq, c, ref))
    print("%s: %s producer=%s error / bound dense %.3f paged %.3f (away from the residual's element: %.3f, %.3f)" % (
        c.cid, c.form, c.producer, ratios["dense"][0], ratios["paged"][0], ratios["dense"][1], ratios["paged"][1]))
