"""Cases and reference of the _ex mixture-of-experts entries: MXFP4 experts, router / expert biases, clamped SwiGLU (numpy only; read by
test_moe_mxfp4_cpu.py and test_moe_mxfp4_gpu.py).  Wraps moe_cases (shapes, router operands with exactly known logits, bounds) and
mxfp4_cases (the quantiser and the exact value of every code).

Expert weights: drawn as moe_cases.build draws them; every block of 32 along K is multiplied by 2^d, d in 0 .. 3 (neighbouring blocks of
a row differ by up to 8 x, so a scale taken from the wrong block or row shows), the whole divided by 4, rounded to fp16 and quantised
with mxfp4_cases.quantize on the flattened [E * 2 Ie, H] and [E * H, Ie] matrices -- the layout include/llmie.h states.
The reference computes in float64 on mxfp4_cases.dequantize of the codes (the exact weights), with moe_cases.route on logits + router
bias and ffn() below, which restates the arithmetic of llmie_moe_ffn_ex.  Bounds as in moe_cases: twice the error of the restatement
with the two fp16 roundings (a_j, y) against the unrounded one.

  CASES       every shape of moe_cases.CASES with MXFP4 experts, no bias, plain SwiGLU;
  "lo", "hi"  the ends of the pinned exponent range on the down matrix: every down block at e in -23 .. -20 (the weights are fp16
              subnormals; k = 1, no residual; gate/up x 8 so that y is an fp16 normal) and at e in 10 .. 13 (gate/up / 64 keeps the
              reference's |y| below 3e4, asserted by test_moe_mxfp4_cpu.py);
  EPI_CASES   r1_e8, r4_e8, r17_e128, r100_counts, r300_counts_rt4 with all three biases and the clamped act (alpha 1.702, limit 1.0),
              each on fp16 and on MXFP4 experts.  The router bias is an integer multiple of the logits' unit (moe_cases: 2^(-2 - s)),
              so logits + bias are exact in fp32 and ties stay exact ties.
"""
import numpy as np

import moe_cases as mc
import mxfp4_cases as mx

ACT_SWIGLU, ACT_CLAMPED = 0, 1
ALPHA, LIMIT = 1.702, 1.0


def _case(base, fmt="mxfp4", epi=False, end=None, id=None):
    return dict(id=id or "%s_%s%s" % (base["id"], fmt, "_epi" if epi else ""), base=base, fmt=fmt, epi=epi, end=end,
                rows=base["rows"], H=base["H"], Ie=base["Ie"], E=base["E"], k=base["k"], flags=base["flags"])


CASES = [_case(c) for c in mc.CASES]
END_CASES = [_case(mc._c("mx4_lo", 4, 256, 192, 8, 1, resid=False), end="lo", id="lo"),
             _case(mc._c("mx4_hi", 4, 256, 192, 8, 1, resid=False), end="hi", id="hi")]
EPI_IDS = ["r1_e8", "r4_e8", "r17_e128", "r100_counts", "r300_counts_rt4"]
EPI_CASES = [_case(mc.BY_ID[i], fmt, epi=True) for i in EPI_IDS for fmt in ("f16", "mxfp4")]
ALL_CASES = CASES + END_CASES + EPI_CASES
BY_ID = {c["id"]: c for c in ALL_CASES}
# the base shapes on which test_moe_mxfp4_cpu.py holds the quantisation mutants away from the reference
MUTANT_IDS = ["r1_e1", "r4_e8", "r5_h2112", "r16_i2112", "r17_e128", "r100_counts", "r2_h4160"]


def _quantise(w16, rng, gain):
    """fp16 [N, K] as drawn -> (the fp16 matrix that is quantised, codes [N, K/2], scale bytes [N, K/32])"""
    N, K = w16.shape
    d = rng.integers(0, 4, (N, K // mx.BLOCK))
    w = (w16.astype(np.float64) * np.repeat(2.0 ** d, mx.BLOCK, axis=1) * (gain / 4.0)).astype(np.float16)
    q, s = mx.quantize(w)
    return w, q, s


def build(case):
    """operands of a case in storage types.  x, router, resid: moe_cases.  fp16 experts: gate_up / down fp16 [E, ..].  MXFP4 experts:
    gate_up_q / down_q uint8 codes [E, 2 Ie, H / 2] / [E, H, Ie / 2], gate_up_s / down_s e8m0 bytes, gate_up16 / down16 the fp16
    matrices they were quantised from.  gate_up64 / down64: the exact weights the reference multiplies.  Biases: fp16 or None"""
    base = case["base"]
    b = mc.build(base)
    E, H, Ie = case["E"], case["H"], case["Ie"]
    out = dict(case=case, x=b["x"], router=b["router"], resid=b["resid"], router_bias=None, gate_up_bias=None, down_bias=None,
               act=ACT_CLAMPED if case["epi"] else ACT_SWIGLU, alpha=ALPHA if case["epi"] else 0.0, limit=LIMIT if case["epi"] else 0.0)
    if case["fmt"] == "f16":
        out.update(gate_up=b["gate_up"], down=b["down"], gate_up64=b["gate_up"].astype(np.float64), down64=b["down"].astype(np.float64))
    else:
        rng = mc._rng(base, "mxfp4")
        gain = {None: 1.0, "lo": 8.0, "hi": 1.0 / 64}[case["end"]]
        g16, gq, gs = _quantise(b["gate_up"].reshape(E * 2 * Ie, H), rng, gain)
        d16, dq, ds = _quantise(b["down"].reshape(E * H, Ie), rng, 1.0)
        if case["end"]:
            ebase = mx.E_MIN if case["end"] == "lo" else mx.E_MAX - 3
            ds = (ebase + (np.arange(E * H)[:, None] + np.arange(Ie // mx.BLOCK)[None, :]) % 4 + 127).astype(np.uint8)
        out.update(gate_up_q=gq.reshape(E, 2 * Ie, H // 2), gate_up_s=gs.reshape(E, 2 * Ie, H // mx.BLOCK), down_q=dq.reshape(E, H, Ie // 2),
                   down_s=ds.reshape(E, H, Ie // mx.BLOCK), gate_up16=g16.reshape(E, 2 * Ie, H), down16=d16.reshape(E, H, Ie),
                   gate_up64=mx.dequantize(gq, gs).reshape(E, 2 * Ie, H), down64=mx.dequantize(dq, ds).reshape(E, H, Ie))
    if case["epi"]:
        rng = mc._rng(base, "epilogue")
        s = 2 if base["kind"] == "designed" else 3 + int(round(np.log2(H) / 2))
        top = 1 if base["kind"] == "designed" else 64
        rb = rng.integers(-top, top + 1, E) * 2.0 ** (-2 - s)
        out["router_bias"], out["logit_unit"] = rb.astype(np.float16), 2.0 ** (-2 - s)
        assert np.array_equal(out["router_bias"].astype(np.float64), rb) and (rb != 0).any()
        out["gate_up_bias"] = (rng.standard_normal((E, 2 * Ie)) * 0.25).astype(np.float16)
        out["down_bias"] = (rng.standard_normal((E, H)) * 0.5).astype(np.float16)
    return out


def biased_logits(b):
    r = mc.logits(b["x"], b["router"])
    return r if b["router_bias"] is None else r + b["router_bias"].astype(np.float64)[None, :]


def _f16(a):
    return a.astype(np.float16).astype(np.float64)


def ffn(b, experts, weights, rounded, gate_up=None, down=None, mutant=None, stats=None):
    """y [rows, H] float64 of the built case b under the given routing, the arithmetic of llmie_moe_ffn_ex restated.  rounded: with
    its two fp16 roundings (a_j, y).  gate_up / down: other weights than the exact ones (the quantisation mutants).  mutant: one of
    no_clamp, no_plus1, alpha1, no_gate_up_bias, no_down_bias.  stats: a dict that receives clamp_share"""
    gate_up = b["gate_up64"] if gate_up is None else gate_up
    down = b["down64"] if down is None else down
    x = b["x"].astype(np.float64)
    rows, H = x.shape
    k = experts.shape[1]
    Ie = down.shape[2]
    alpha = 1.0 if mutant == "alpha1" else b["alpha"]
    d = np.zeros((rows, k, H))
    clamped = total = 0
    for e in np.unique(experts):
        m, j = np.nonzero(experts == e)
        t = x[m] @ gate_up[e].T
        g, u = t[:, :Ie], t[:, Ie:]
        if b["gate_up_bias"] is not None and mutant != "no_gate_up_bias":
            gb = b["gate_up_bias"][e].astype(np.float64)
            g, u = g + gb[None, :Ie], u + gb[None, Ie:]
        if b["act"] == ACT_CLAMPED:
            clamped += int(((g > b["limit"]) | (np.abs(u) > b["limit"])).sum())
            total += g.size
            if mutant != "no_clamp":
                g, u = np.minimum(g, b["limit"]), np.clip(u, -b["limit"], b["limit"])
            a = (u + (0.0 if mutant == "no_plus1" else 1.0)) * g / (1.0 + np.exp(-alpha * g))
        else:
            a = g / (1.0 + np.exp(-g)) * u
        if rounded:
            a = _f16(a)
        dj = a @ down[e].T
        if b["down_bias"] is not None and mutant != "no_down_bias":
            dj = dj + b["down_bias"][e].astype(np.float64)[None, :]
        d[m, j] = dj
    y = np.zeros((rows, H))
    for j in range(k):   # rank order
        y = y + weights[:, j:j + 1] * d[:, j]
    if b["resid"] is not None:
        y = y + b["resid"].astype(np.float64)
    if stats is not None:
        stats["clamp_share"] = clamped / total if total else None
    return _f16(y) if rounded else y


def reference(b):
    """everything a test needs of a built case, computed once: routing (under the router bias), the float64 output, the fp16-rounded
    one, the bounds and the clamp share"""
    c = b["case"]
    experts, weights, r = mc.route(b["x"], b["router"], c["k"], c["flags"], r=biased_logits(b))
    stats = {}
    y64 = ffn(b, experts, weights, rounded=False, stats=stats)
    y16 = ffn(b, experts, weights, rounded=True)
    return dict(experts=experts, weights=weights, logits=r, y64=y64, y16=y16, bounds=mc.bounds(y64, y16), clamp_share=stats["clamp_share"])


def distance_in_bounds(y, ref):
    """how many bounds y lies from the float64 reference: the smaller of the two ratios (a mutant has to leave BOTH by the factor)"""
    bd = ref["bounds"]
    return min(float(np.abs(y - ref["y64"]).max()) / bd["max_abs"], mc.rel_frobenius(y, ref["y64"]) / bd["rel"])


def weight_mutants(b):
    """name -> (gate_up, down) float64: what a kernel that misreads the format would multiply"""
    c = b["case"]
    E, H, Ie = c["E"], c["H"], c["Ie"]
    gq, gs = b["gate_up_q"].reshape(E * 2 * Ie, -1), b["gate_up_s"].reshape(E * 2 * Ie, -1)
    dq, ds = b["down_q"].reshape(E * H, -1), b["down_s"].reshape(E * H, -1)

    def deq(gq, gs, dq, ds):
        return mx.dequantize(gq, gs).reshape(E, 2 * Ie, H), mx.dequantize(dq, ds).reshape(E, H, Ie)

    swap = lambda q: ((q >> 4) | (q << 4)).astype(np.uint8)
    return dict(swapped_nibbles=deq(swap(gq), gs, swap(dq), ds),
                scales_rolled_along_k=deq(gq, np.roll(gs, 1, axis=1), dq, np.roll(ds, 1, axis=1)),
                scales_rolled_by_a_row=deq(gq, np.roll(gs, 1, axis=0), dq, np.roll(ds, 1, axis=0)),
                unquantised=(b["gate_up16"].astype(np.float64), b["down16"].astype(np.float64)))


GEMV_DEFAULT_ROWS_MXFP4 = 16   # include/llmie.h: MXFP4 experts take the gemv route up to 16 rows (fp16: moe_cases.GEMV_DEFAULT_ROWS)


def expected_plan(case):
    """(route, rt, tiles) of the default plan by the thresholds include/llmie.h states for the case's expert format"""
    rows, H, Ie, E, k = (case[n] for n in ("rows", "H", "Ie", "E", "k"))
    gemv = case["fmt"] == "mxfp4" and rows <= GEMV_DEFAULT_ROWS_MXFP4 and H <= 16384 and Ie <= 16384
    return mc.expected_plan(rows, H, Ie, E, k, force="gemv" if gemv else None)


EPI_MUTANTS = ["no_clamp", "no_plus1", "alpha1", "no_gate_up_bias", "no_down_bias"]
