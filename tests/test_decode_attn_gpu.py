"""Decode attention (csrc/attention_decode.hip: the split-KV kernel, its merge kernel, the in-launch ticket merge, the generic
kernel) on every geometry it dispatches, at the steps where it changes behaviour, with inputs that can fail.

Cases, planted rows and the float64 reference come from tests/attn_cases.py; tests/test_decode_attn_cases_cpu.py shows on the
CPU that the bounds used here are met by the project's C oracle and that seeded defects are rejected by the same comparison.

    activations / cache   head_size            tokens per chunk         128-token pages per chunk
    fp16 / fp16           32 / 64 / 128 / 256   512 / 256 / 128 / 64     4 / 2 / 1 / 1
    fp32 / fp32           32 / 64 / 128 / 256   256 / 128 / 64 / 32      2 / 1 / 1 / 1

Every case id names dtype, head size, head ratio and step(s).  Each runs the public forms -- llmie_decoder_mha (host step; the
device-step form once per geometry), llmie_decoder_mha_rope with the separate merge kernel and with tickets,
llmie_decoder_mha_ragged dense and paged with the sequences at different steps -- and compares the output with the float64
reference and BOTH caches with their inputs: the appended row equal to the rounded new k / v, every other slot (other layers
and unmapped pool pages included) bit-identical.  Outputs start at 9 and the workspace is filled with NaN: nothing may depend
on what a buffer held before.

    fp16 / e4m3           64 / 128              512 / 256 (x 1, 2, 8 chunks per workgroup at batch 2, 16, 64)    4 / 2

The e4m3-cache form has no unit entry: it runs through a one-layer Decoder with o = identity and gate_up = 0, so that
hidden_out - x is the attention output (test_decode_attention_e4m3_cache_through_the_engine).
"""
import numpy as np
import pytest
import torch

import attn_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda"
TT = {ac.F16: torch.float16, ac.F32: torch.float32}
UNIFORM, RAGGED, GENERIC = ac.uniform_cases(), ac.ragged_cases(), ac.generic_cases()


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(TT[dtype])


class _Inputs:
    def __init__(self, llmie, c):
        self.c = c
        self.qkv, self.kc, self.vc = _dev(c.qkv, c.dtype), _dev(c.kc, c.dtype), _dev(c.vc, c.dtype)
        self.bias = None if c.bias is None else _dev(c.bias, c.dtype)
        self.tab = None if c.tab is None else _dev(c.tab)
        self.ws = torch.full((max(1, llmie.decoder_mha_workspace_bytes(c.bs, c.nh, c.hs, c.max_seq) // 4),), float("nan"),
                             device=DEV)

    def out(self):
        return torch.full((self.c.bs, self.c.nh * self.c.hs), 9.0, dtype=TT[self.c.dtype], device=DEV)


def _check_new_rows(c, form, name, rows, new, tol):
    err = np.abs(rows.double().cpu().numpy() - new)
    if not (err <= tol).all():
        b, g, d = np.unravel_index(np.argmax(err - tol), err.shape)
        raise AssertionError("%s: appended %s row of b=%d kv_head=%d dim=%d is %r, expected %r (+- %.3g)" % (
            c.describe(form), name, b, g, d, float(rows[b, g, d]), float(new[b, g, d]), float(tol[b, g, d])))


def _check_caches(c, form, kd, vd, kin, vin):
    for name, got, inp, new, tol in (("K", kd, kin, c.k_new, c.k_tol), ("V", vd, vin, c.v_new, c.v_tol)):
        exp = inp.clone()
        for b, s in enumerate(c.steps):
            exp[c.layer, b, :, s - 1] = got[c.layer, b, :, s - 1]
        if not torch.equal(got, exp):
            where = (got != exp).nonzero()[0].tolist()
            raise AssertionError("%s: %s cache changed outside the appended slot, first at [layer, b, kv_head, t, d] = %s" % (
                c.describe(form), name, where))
        rows = torch.stack([got[c.layer, b, :, s - 1] for b, s in enumerate(c.steps)])
        _check_new_rows(c, form, name, rows, new, tol)


def _run(llmie, c, x, form, call, bounds):
    kd, vd, out = x.kc.clone(), x.vc.clone(), x.out()
    call(kd, vd, out)
    torch.cuda.synchronize()
    r = ac.check(out.double().cpu().numpy(), c, form, bounds)
    _check_caches(c, form, kd, vd, x.kc, x.vc)
    return r


# ------------------------------------------------------------------------------------------------- the batch at one position
@pytest.mark.parametrize("cid,dtype,geo,step,logit", UNIFORM, ids=[u[0] for u in UNIFORM])
def test_decode_attention_uniform(llmie, cid, dtype, geo, step, logit):
    C = ac.chunk_len(dtype, geo[0])
    # plain entry
    c = ac.build_uniform(dtype, geo, step, logit)
    x = _Inputs(llmie, c)
    b = ac.BOUNDS["plain"][dtype]
    rs = [_run(llmie, c, x, "decoder_mha(host step)",
               lambda kd, vd, out: llmie.decoder_mha(x.qkv, x.bias, kd, vd, out, c.layer, c.nh, c.kvh, step, x.ws), b)]
    # the split kernel answered (not the generic one, which takes no workspace): partials exist exactly when there are >= 2 chunks
    assert bool(torch.isfinite(x.ws).any()) == (step > C), c.describe("decoder_mha(host step)") + ": workspace use"
    if step == 17 * C + 1:   # once per geometry (and in the logit-40 cases): the position read on the device
        sd = torch.tensor([step], dtype=torch.int32, device=DEV)
        rs.append(_run(llmie, c, x, "decoder_mha(device step)",
                       lambda kd, vd, out: llmie.decoder_mha(x.qkv, x.bias, kd, vd, out, c.layer, c.nh, c.kvh, -1, x.ws,
                                                             step_dev=sd), b))
    # RoPE fused in front: separate merge kernel, then the in-launch merge
    c = ac.build_uniform(dtype, geo, step, logit, rope=True)
    x = _Inputs(llmie, c)
    b = ac.BOUNDS["rope"][dtype]
    rs.append(_run(llmie, c, x, "decoder_mha_rope(tickets=None)",
                   lambda kd, vd, out: llmie.decoder_mha_rope(x.qkv, x.bias, kd, vd, out, c.layer, c.nh, c.kvh, step, x.ws,
                                                              x.tab, c.rot, None), b))
    tickets = torch.zeros(c.bs * c.kvh, dtype=torch.int32, device=DEV)
    rs.append(_run(llmie, c, x, "decoder_mha_rope(tickets)",
                   lambda kd, vd, out: llmie.decoder_mha_rope(x.qkv, x.bias, kd, vd, out, c.layer, c.nh, c.kvh, step, x.ws,
                                                              x.tab, c.rot, tickets), b))
    assert int(tickets.abs().sum()) == 0, c.describe("decoder_mha_rope(tickets)") + ": tickets not back to zero"
    print("%s: error / bound per form %s" % (cid, ["%.3f" % r for r in rs]))


# ------------------------------------------------------------------------------------- the sequences at different positions
def _pool(dense, perm, filler):
    """dense [L, bs, kvh, max_seq, hs] -> pool [L, num_pages, kvh, 128, hs] under the block table perm [bs, max_pages]; rows past
    max_seq and unmapped pages hold `filler`"""
    L, bs, kvh, max_seq, hs = dense.shape
    max_pages = perm.shape[1]
    padded = torch.full((L, bs, kvh, max_pages * 128, hs), 0.25, dtype=dense.dtype, device=DEV)
    padded[:, :, :, :max_seq] = dense
    pages = padded.view(L, bs, kvh, max_pages, 128, hs).permute(0, 1, 3, 2, 4, 5).reshape(L, bs * max_pages, kvh, 128, hs)
    pool = filler.clone()
    pool[:, perm.flatten().long()] = pages
    return pool


@pytest.mark.parametrize("cid,dtype,geo,steps", RAGGED, ids=[r[0] for r in RAGGED])
def test_decode_attention_ragged_dense_and_paged(llmie, cid, dtype, geo, steps):
    c = ac.build_ragged(dtype, geo, steps)
    x = _Inputs(llmie, c)
    b = ac.BOUNDS["rope"][dtype]
    ctx = torch.tensor(steps, dtype=torch.int32, device=DEV)
    r1 = _run(llmie, c, x, "decoder_mha_ragged(dense)",
              lambda kd, vd, out: llmie.decoder_mha_ragged(x.qkv, x.bias, kd, vd, out, c.layer, c.nh, c.kvh, ctx, x.ws, x.tab,
                                                           c.rot, c.max_seq), b)
    # paged: the same rows behind a shuffled block table, in pools with two spare pages and random bytes wherever no row lives
    form = "decoder_mha_ragged(paged)"
    rng = np.random.default_rng(5)
    max_pages = -(-c.max_seq // 128)
    num_pages = c.bs * max_pages + 2
    perm = _dev(rng.permutation(num_pages)[:c.bs * max_pages].astype(np.int32).reshape(c.bs, max_pages))
    filler = (torch.randn((c.L, num_pages, c.kvh, 128, c.hs), device=DEV) * 0.5).to(TT[dtype])
    kp, vp, out = _pool(x.kc, perm, filler), _pool(x.vc, perm, filler), x.out()
    llmie.decoder_mha_ragged(x.qkv, x.bias, kp, vp, out, c.layer, c.nh, c.kvh, ctx, x.ws, x.tab, c.rot, c.max_seq,
                             block_table=perm)
    torch.cuda.synchronize()
    r2 = ac.check(out.double().cpu().numpy(), c, form, b)
    for name, pool, inp, new, tol in (("K", kp, x.kc, c.k_new, c.k_tol), ("V", vp, x.vc, c.v_new, c.v_tol)):
        rows = torch.stack([pool[c.layer, int(perm[i, (s - 1) // 128]), :, (s - 1) % 128] for i, s in enumerate(steps)])
        exp = inp.clone()
        for i, s in enumerate(steps):
            exp[c.layer, i, :, s - 1] = rows[i]
        assert torch.equal(pool, _pool(exp, perm, filler)), "%s: %s pool changed outside the appended slots" % (c.describe(form), name)
        _check_new_rows(c, form, name, rows, new, tol)
    print("%s: error / bound dense %.3f paged %.3f" % (cid, r1, r2))


# ---------------------------------------------------------------------------------------------------------- the generic kernel
@pytest.mark.parametrize("cid,dtype,g,step", GENERIC, ids=[g[0] for g in GENERIC])
def test_decode_attention_generic_kernel(llmie, cid, dtype, g, step):
    c = ac.build_generic(dtype, g, step)
    x = _Inputs(llmie, c)
    b = ac.BOUNDS["plain"][dtype]
    sd = torch.tensor([step], dtype=torch.int32, device=DEV)
    r1 = _run(llmie, c, x, "decoder_mha(host step, generic)",
              lambda kd, vd, out: llmie.decoder_mha(x.qkv, x.bias, kd, vd, out, 0, c.nh, c.kvh, step, x.ws), b)
    r2 = _run(llmie, c, x, "decoder_mha(device step, generic)",
              lambda kd, vd, out: llmie.decoder_mha(x.qkv, x.bias, kd, vd, out, 0, c.nh, c.kvh, -1, x.ws, step_dev=sd), b)
    print("%s: error / bound %.3f %.3f" % (cid, r1, r2))


@pytest.mark.parametrize("dtype", [ac.F16, ac.F32])
def test_forms_the_generic_kernel_does_not_have_are_errors(llmie, dtype):
    """head ratio 3: fused RoPE, the in-launch merge and ragged batches exist in the split kernel only -- an error, and nothing
    written, rather than an answer without them"""
    c = ac.build_generic(dtype, ac.GENERIC[0], 257)
    x = _Inputs(llmie, c)
    tab = _dev(ac.rope_table(c.max_seq, c.hs, c.hs))
    kd, vd, out = x.kc.clone(), x.vc.clone(), x.out()
    tickets = torch.zeros(c.bs * c.kvh, dtype=torch.int32, device=DEV)
    with pytest.raises(llmie.LlmieError):
        llmie.decoder_mha_rope(x.qkv, x.bias, kd, vd, out, 0, c.nh, c.kvh, 257, x.ws, tab, c.hs, None)
    with pytest.raises(llmie.LlmieError):
        llmie.decoder_mha_rope(x.qkv, x.bias, kd, vd, out, 0, c.nh, c.kvh, 257, x.ws, None, 0, tickets)
    with pytest.raises(llmie.LlmieError):
        llmie.decoder_mha_ragged(x.qkv, x.bias, kd, vd, out, 0, c.nh, c.kvh, torch.tensor([257, 5], dtype=torch.int32, device=DEV),
                                 x.ws, tab, c.hs, c.max_seq)
    torch.cuda.synchronize()
    assert torch.equal(kd, x.kc) and torch.equal(vd, x.vc) and bool((out == 9.0).all())


# ---------------------------------------------------------------------------------- fp16 activations over an e4m3 KV cache
E4M3 = ac.e4m3_cases()
_ENGINE = {}


def _e4m3_engine(llmie, c, hs, ratio, bs, sc):
    key = (hs, ratio, bs, sc)
    if _ENGINE.get("key") != key:
        if "dec" in _ENGINE:
            _ENGINE.pop("dec").close()
        w, H = c.weights, c.nh * c.hs
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(torch.float16)
        layer = dict(attn_norm=d(w["attn_norm"]), ffn_norm=d(w["ffn_norm"]), qkv=dict(data=d(w["qkv"])),
                     o=dict(data=torch.eye(H, dtype=torch.float16, device=DEV)),
                     gate_up=dict(data=torch.zeros((2 * w["I"], H), dtype=torch.float16, device=DEV)), down=dict(data=d(w["down"])))
        cfg = dict(head_num=c.nh, kv_head_num=c.kvh, head_size=hs, inter_size=w["I"], num_layers=1, vocab_size=100,
                   max_seq_len=c.max_seq, max_batch=bs, rotary_dim=hs, rotary_base=10000.0, rms_eps=1e-5, dtype=llmie.F16,
                   wfmt=llmie.W_F16, int4_group=128, kv_fmt=llmie.KV_FP8, k_scale=c.scales[0], v_scale=c.scales[1])
        _ENGINE.update(key=key, dec=llmie.Decoder(cfg, [layer]))
    return _ENGINE["dec"]


@pytest.mark.parametrize("cid,hs,ratio,bs,sc,step", E4M3, ids=[e[0] for e in E4M3])
def test_decode_attention_e4m3_cache_through_the_engine(llmie, cid, hs, ratio, bs, sc, step):
    """Bound: the fp16 attention bound (3e-3, 2e-3) plus one fp16 ulp of |x| for the residual add.  The CPU composition of the same
    step (oracle kernels, fp16 roundings where the device rounds) reaches at most 0.23 of that bound against the float64 reference
    over these cases (tests/test_decode_attn_cases_cpu.py measures and asserts it), so the bound stands as it is."""
    c = ac.make_case_e4m3(hs, ratio, bs, sc, step)
    dec = _e4m3_engine(llmie, c, hs, ratio, bs, sc)
    form = "Decoder.forward(e4m3 cache, batch %d, %d chunks per workgroup, %s scales)" % (bs, c.cpw, sc)
    kin, vin = torch.from_numpy(c.kq).to(DEV), torch.from_numpy(c.vq).to(DEV)
    kd, vd = kin.clone(), vin.clone()
    xd = torch.from_numpy(c.x).to(DEV).to(torch.float16)
    out = dec.forward(xd, torch.full_like(xd, 9.0), kd, vd, step)
    torch.cuda.synchronize()
    # caches: every slot but step - 1 keeps its byte; the appended rows are e4m3(new k, v / scale) of the CPU composition, up to the
    # neighbouring code where the device's fp16 value fell on the other side of a rounding boundary (one e4m3 step = 2^-3 relative)
    rows = {}
    for name, got, inp, want, scale in (("K", kd, kin, c.k_codes_new, c.scales[0]), ("V", vd, vin, c.v_codes_new, c.scales[1])):
        exp = inp.clone()
        exp[0, :, :, step - 1] = got[0, :, :, step - 1]
        assert torch.equal(got, exp), "%s: %s cache changed outside the appended slot" % (c.describe(form), name)
        rows[name] = got[0, :, :, step - 1].cpu().numpy()
        a, b = ac.E4M3[rows[name]].astype(np.float64) * scale, ac.E4M3[want].astype(np.float64) * scale
        assert (rows[name] != want).mean() < 0.02, "%s: appended %s codes differ in %.3f of the elements" % (
            c.describe(form), name, (rows[name] != want).mean())
        # (+ two fp16 ulps at the row's magnitude: the batch paths rotate k in fp32 straight from the projection's partial sums,
        # the composition from its fp16 image, and near zero that difference spans several of the small codes)
        tol = 0.126 * np.abs(b) + scale * 2.0 ** -9 + 2.0 ** -9 * np.abs(b).max(axis=-1, keepdims=True)
        assert (np.abs(a - b) <= tol).all(), "%s: appended %s row, worst excess %.3g" % (c.describe(form), name, (np.abs(a - b) - tol).max())
    # the attention output: reference on the de-quantised cache INCLUDING the appended rows as the device stored them
    ac.finish_e4m3(c, rows["K"], rows["V"])
    attn = out.double().cpu().numpy() - c.x.astype(np.float64)
    r = ac.check(attn, c, form, ac.BOUNDS["rope"][ac.F16], extra_atol=ac.e4m3_extra_atol(c))
    print("%s: error / bound %.3f" % (cid, r))
