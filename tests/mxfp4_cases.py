"""MXFP4 (OCP microscaling 4-bit) weights: a numpy restatement of the quantiser and de-quantiser of include/llmie.h, and projection
cases whose one correct answer is known to the bit (numpy only; read by test_mxfp4_cpu.py and test_mxfp4_linear_gpu.py).

An e2m1 code times a power of two is an exactly known number, so the method of exact_linear_cases.py carries over:

Integer cases (dense): x[m, k] = i * 2^j(m) with |i| <= 3, codes drawn over all 16 values, block exponents e(n, b) = en(n) + d(n, b) + c
with d in 0..3 (blocks of one row differ by factors up to 8), en cycling over 8 octaves from row to row and one common shift c that
puts the largest |y| just below 65504.  In units of 2^(j(m) + en(n) + c - 1) a weight is the integer 2 * magnitude * 2^d <= 96, so
every product and every partial sum is an integer below 2^24 units (K = 8224: 8224 * 3 * 96 = 2.37e6): exact in fp32 in any order,
through a dot2 or an MFMA, with the block's 2^e applied to the weight or to the block's partial sum.  The result is the fp16
round-to-nearest-even of an exactly known number.
  "plain"  large sums, the single rounding is exercised where K is large (conditions() asserts it from K = 2048 and 64 outputs);
  "epi"    bias + residual, |acc + bias + residual| <= 2048 units: exact whether a route rounds before or after the add.
Probe cases (sparse): activation rows of one or two non-zeros +-7 * 2^jx at the k edges of the routes (first / last k, both sides of
every 32-element block boundary near the start, the middle and the end of the row, of the 128-k groups a wave of the MFMA kernel
takes and of the 1024-k round of its eight waves, of the 2048-k parts and strides of the GEMV's waves), every code on every probed column, block
exponents at the ends of the pinned range: "lo" e in -23 .. -20 (the weights are fp16 subnormals), "hi" e in 10 .. 13, "mid" around 0.
"""
import numpy as np

import exact_linear_cases as X

MAG = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
E_MIN, E_MAX = -23, 13          # pinned range of block exponents: every weight is an fp16 number
BLOCK = 32


# ---------------------------------------------------------------- the format, restated
def unpack(wq):
    """uint8 [N, K/2] -> codes [N, K] (low nibble = even k)"""
    wq = np.asarray(wq, np.uint8)
    out = np.empty((wq.shape[0], wq.shape[1] * 2), np.uint8)
    out[:, 0::2], out[:, 1::2] = wq & 0xF, wq >> 4
    return out


def pack(codes):
    return X._pack4(np.asarray(codes, np.uint8))


def dequantize(wq, scale):
    """exact real value of every weight, float64 [N, K]; NaN for a 0xFF block"""
    codes = unpack(wq)
    mag = MAG[codes & 7] * np.where(codes & 8, -1.0, 1.0)
    sc = np.asarray(scale, np.uint8)
    two_e = np.where(sc == 0xFF, np.nan, 2.0 ** (sc.astype(np.float64) - 127))
    return mag * np.repeat(two_e, BLOCK, axis=1)


def dequantize_f16(wq, scale):
    """what llmie_dequantize_mxfp4 writes: the round-to-nearest-even fp16 of the exact value, 0x7E00 for a 0xFF block, -0 kept"""
    with np.errstate(over="ignore", invalid="ignore"):
        h = dequantize(wq, scale).astype(np.float16)
    bits = h.view(np.uint16).copy()
    bits[np.repeat(np.asarray(scale, np.uint8) == 0xFF, BLOCK, axis=1)] = 0x7E00
    return bits.view(np.float16)


def quantize(w):
    """fp16 [N, K] -> (wq uint8 [N, K/2], scale uint8 [N, K/32]); the codes of a block with a non-finite element are zeros here
    (unspecified in the library)"""
    w = np.asarray(w, np.float16)
    N, K = w.shape
    assert K % BLOCK == 0
    a = np.abs(w.astype(np.float64)).reshape(N, K // BLOCK, BLOCK)
    with np.errstate(invalid="ignore"):
        bad = ~np.isfinite(a).all(axis=2)
        amax = np.where(bad, 1.0, a.max(axis=2))
    zero = amax == 0
    e = np.clip(np.floor(np.log2(np.where(zero, 1.0, amax))) - 2, E_MIN, E_MAX)   # log2 of an fp16 number: exact enough, floor is safe
    e = np.where(zero, 0, e)
    r = np.where(bad[:, :, None], 0.0, a) / 2.0 ** e[:, :, None]                   # exact
    code = ((r > 0.25).astype(np.uint8) + (r >= 0.75) + (r > 1.25) + (r >= 1.75) + (r > 2.5) + (r >= 3.5) + (r > 5.0)).astype(np.uint8)
    sign = ((w.view(np.uint16) >> 15) & 1).astype(np.uint8).reshape(N, K // BLOCK, BLOCK)
    code = np.where(bad[:, :, None], 0, code | (sign << 3)).astype(np.uint8)
    scale = np.where(bad, 0xFF, e + 127).astype(np.uint8)
    return pack(code.reshape(N, K)), scale


def quantiser_inputs(N, K, seed=0):
    """fp16 [N, K] whose blocks meet every rule of the quantiser: exact ties, values in (6, 8) * 2^e, an all-zero block, -0, fp16
    subnormals, 65504, and -- last two blocks -- one block with inf and one with NaN.  (expected scale bytes only there)"""
    rng = np.random.default_rng(seed)
    nb = N * K // BLOCK
    w = np.zeros((nb, BLOCK), np.float64)
    ties = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 0.25 + 2 ** -9, 0.75 - 2 ** -9, 5 + 2 ** -7, 5 - 2 ** -7])
    for b in range(nb):
        kind = b % 8
        e = int(rng.integers(-12, 12))
        sg = rng.choice(np.array([1.0, -1.0]), BLOCK)
        if kind == 0:      # exact ties and their neighbours under an amax of 4 .. 6 * 2^e
            v = np.resize(ties, BLOCK)
            v[0] = rng.choice(np.array([4.0, 5.0, 6.0, 7.0]))
        elif kind == 1:    # values in (6, 8): saturation
            v = rng.uniform(6, 8, BLOCK)
            v[1:8] = rng.uniform(0, 6, 7)
        elif kind == 2:    # all zero, with -0
            v, e = np.zeros(BLOCK), 0
        elif kind == 3:    # fp16 subnormals: the clamp at e = -23
            v, e = rng.integers(0, 64, BLOCK).astype(np.float64), -24
            if b % 16 == 3:
                v = np.zeros(BLOCK)
                v[5] = 1.0                                  # amax = 2^-24
        elif kind == 4:    # the top: amax = 65504
            v, e = rng.uniform(0, 65504, BLOCK), 0
            v[7] = 65504.0
        else:
            v = rng.uniform(0, 8, BLOCK) * rng.choice(np.array([1.0, 0.25, 0.01]), BLOCK)
            v[3] = rng.uniform(4, 8)
        w[b] = sg * v * 2.0 ** e
    with np.errstate(over="ignore"):
        h = w.astype(np.float16)
    h = h.reshape(N, K).copy()
    bits = h.view(np.uint16)
    zb = [b for b in range(nb) if b % 8 == 2]
    for b in zb:
        bits.reshape(nb, BLOCK)[b, 1::3] = 0x8000          # -0 inside the all-zero block
    special = np.zeros(nb, bool)
    if nb >= 3:
        hb = h.reshape(nb, BLOCK)
        hb[nb - 1, 4] = np.float16(np.nan)
        hb[nb - 2, 9] = np.float16(-np.inf)
        special[[nb - 1, nb - 2]] = True
    return h, special.reshape(N, K // BLOCK)


# ---------------------------------------------------------------- exact projection cases
def _c(id, route, M, K, N, ws="auto", kind="int", **kw):
    return dict(id=id, fmt="mxfp4", route=route, M=M, K=K, N=N, ws=ws, kind=kind, entry="linear", group=0, xoff=0, **kw)


def route_of(M, ws="auto"):
    if M <= 8:
        return "mxfp4_gemv"
    if M <= 64:
        return "mxfp4_mfma"
    if M < 192 or ws is None:
        return "mxfp4_chunks"
    # N = 256, K = 4096 below: the fp16 GEMM on the image runs 128 x 128 tiles, past 192 rows its partly filled 256-row grid
    return "image_prefill+tiles128" if M <= 192 else "image_prefill+tiles256_part"


CASES = [_c("mx4_m%d_k%d_n%d" % (M, K, N), route_of(M), M, K, N) for M in (1, 3, 8) for K in (32, 96, 4128) for N in (1, 17, 1003)]
CASES += [_c("mx4_m%d_k%d_n%d" % (M, K, N), route_of(M), M, K, N) for M in (9, 16, 17, 64) for K in (32, 64, 2080) for N in (16, 17, 1000)]
# up to 4 rows the GEMV splits a weight row over four waves from K = 8192 (4128: two, below: one); more rows: one wave
CASES += [_c("mx4_m%d_k8224_n17" % M, route_of(M), M, 8224, 17) for M in (3, 5)]
CASES += [_c("mx4_m%d_k4096_n48" % M, route_of(M), M, 4096, 48) for M in (65, 130)]
CASES += [_c("mx4_m%d_k4096_n256" % M, route_of(M), M, 4096, 256) for M in (192, 300)]
CASES += [_c("mx4_m%d_k4096_n256_nows" % M, route_of(M, None), M, 4096, 256, ws=None) for M in (192, 300)]

_PROBE_SHAPES = [(8, 4128, 17), (8, 96, 17), (8, 8224, 17), (17, 2080, 17), (64, 2080, 16), (65, 4096, 48), (192, 4096, 256)]
PROBES = []
for _M, _K, _N in _PROBE_SHAPES:
    _rots = -(-len(X.edge_ks(_K)) // (2 * _M))
    for _rot in range(_rots):
        PROBES.append(_c("mx4_probe_m%d_k%d_mid_r%d" % (_M, _K, _rot), route_of(_M), _M, _K, _N, kind="probe", ebase=-2, rot=_rot))
    for _name, _eb in (("lo", E_MIN), ("hi", E_MAX - 3)):
        PROBES.append(_c("mx4_probe_m%d_k%d_%s" % (_M, _K, _name), route_of(_M), _M, _K, _N, kind="probe", ebase=_eb, rot=0))


def epilogues(case):
    return ("plain",) if case["kind"] == "probe" else ("plain", "epi")


def build(case, epi, check=True):
    out = _build_probe(case) if case["kind"] == "probe" else _build_int(case, epi)
    out.update(case=case, epi=epi)
    if check:
        conditions(out)
    return out


def _build_int(case, epi):
    rng = X._rng(case, epi)
    M, K, N = case["M"], case["K"], case["N"]
    nb = K // BLOCK
    xi, jm = X._activations_int(case, epi, rng)
    codes = rng.integers(0, 16, (N, K)).astype(np.uint8)
    d = rng.integers(0, 4, (N, nb))
    en = -(np.arange(N) * 3 % X.E_SPAN)
    # weight in units of 2^(en - 1): (2 * magnitude) * 2^d, an integer <= 96
    wi = (2 * MAG[codes & 7] * np.where(codes & 8, -1, 1)).astype(np.int64) * 2 ** np.repeat(d, BLOCK, axis=1)
    S = xi.astype(np.float64) @ wi.astype(np.float64).T
    T, bi, ri = S, None, None
    if epi == "epi":
        jtop = jm.max()
        bi = rng.integers(-4, 5, N)
        T = T + bi[None, :] * 2.0 ** (jtop - jm)[:, None]
        ri = rng.integers(-600, 601, (M, N)).astype(np.float64)
        ri = np.clip(ri, -2048 - T, 2048 - T)
        assert np.abs(ri).max() <= 2048
        T = T + ri
    big = np.abs(T)                                     # the shift keeps the output and the epilogue operands below 65504
    if epi == "epi":
        big = np.maximum(big, np.maximum(np.abs(ri), np.abs(bi)[None, :] * 2.0 ** (jtop - jm)[:, None]))
    top = (big * 2.0 ** (jm[:, None] + en[None, :] - 1)).max()
    c = int(np.floor(np.log2(X.F16_MAX / top))) if top > 0 else 0
    c = min(c, E_MAX - 3)                               # (a tiny case could otherwise leave the pinned range at the top)
    en = en + c
    U = jm[:, None] + en[None, :] - 1
    x = (xi * 2.0 ** jm[:, None]).astype(np.float16)
    assert np.array_equal(x.astype(np.float64), xi * 2.0 ** jm[:, None])
    e = en[:, None] + d
    scale = (e + 127).astype(np.uint8)
    out = dict(x=x, xi=xi, jm=jm, wi=wi, en=en, e=e, S=S, T=T, U=U, exact=T * 2.0 ** U, expected=(T * 2.0 ** U + 0.0).astype(np.float16),
               w=pack(codes), codes=codes, scale=scale, deq=wi * 2.0 ** (en[:, None] - 1), bias=None, residual=None)
    if bi is not None:
        out["bias"] = (bi * 2.0 ** (jm.max() + en - 1)).astype(np.float16)
    if ri is not None:
        out["residual"] = (ri * 2.0 ** U).astype(np.float16)
    return out


def _build_probe(case):
    rng = X._rng(case, "probe")
    M, K, N, ebase, rot = case["M"], case["K"], case["N"], case["ebase"], case["rot"]
    nb = K // BLOCK
    ks = X.edge_ks(K)
    ks = ks[:len(ks) // 2 * 2]
    # x = +-7 * 2^jx: the smallest product 3.5 * 2^(jx + ebase) sits at 3.5 * 2^-14 ("lo": jx = 9), the largest sum of two
    # 2 * 42 * 2^(jx + ebase + 3) at 43008 ("hi": jx = -4); every sum or difference is a multiple of the smallest product
    jx = -14 - ebase if ebase < -14 else (-4 if ebase + 3 == E_MAX else 0)
    x = np.zeros((M, K), np.float64)
    hit = []
    for m in range(M):
        k1, k2 = ks[(2 * (m + rot * M)) % len(ks)], ks[(2 * (m + rot * M) + 1) % len(ks)]
        x[m, k1] = 7 * 2.0 ** jx
        hit.append(k1)
        if m % 3 != 2:
            x[m, k2] = 7 * 2.0 ** jx * (1 if m % 4 < 2 else -1)
            hit.append(k2)
    hit = sorted(set(hit))
    codes = rng.integers(0, 16, (N, K)).astype(np.uint8)
    for i, k in enumerate(hit):                          # every code meets every probed k within 16 weight rows
        codes[:, k] = np.resize(np.roll(np.arange(16, dtype=np.uint8), 5 * i), N)
    e = ebase + (np.arange(N)[:, None] + np.arange(nb)[None, :]) % 4
    scale = (e + 127).astype(np.uint8)
    w = pack(codes)
    deq = dequantize(w, scale)
    exact = x @ deq.T
    return dict(x=x.astype(np.float16), w=w, codes=codes, scale=scale, e=e, deq=deq, bias=None, residual=None, exact=exact,
                expected=(exact + 0.0).astype(np.float16), hit=hit)


def conditions(b):
    """the conditions of the module docstring, asserted (not measured) for a built case"""
    case, epi = b["case"], b["epi"]
    assert b["e"].min() >= E_MIN and b["e"].max() <= E_MAX, "%s: a block exponent leaves the pinned range" % case["id"]
    assert np.array_equal(dequantize(b["w"], b["scale"]), b["deq"])
    assert np.array_equal(dequantize_f16(b["w"], b["scale"]).astype(np.float64), b["deq"]), "a weight is no fp16 number"
    assert X._normal16(b["x"]) and X._normal16(b["exact"]), "%s: operand or output outside fp16's normal range" % case["id"]
    assert np.abs(b["exact"]).max() <= X.F16_MAX
    assert np.array_equal(b["expected"].astype(np.float64) != 0, b["exact"] != 0)
    for name in ("bias", "residual"):
        if b[name] is not None:
            assert X._normal16(b[name]), name
    if case["kind"] == "probe":
        # one or two products per output, both multiples of the smallest product and at most 2 * 42 * 8 of it: exact in fp32
        assert ((b["x"] != 0).sum(axis=1) <= 2).all() and ((b["x"] != 0).sum(axis=1) >= 1).all()
        if case["N"] >= 16:
            for k in b["hit"]:
                assert len(set(b["codes"][:, k].tolist())) == 16, "a code misses a probed k"
        unit = 3.5 * 2.0 ** (np.log2(np.abs(b["x"][b["x"] != 0].astype(np.float64)).min() / 7) + case["ebase"])
        q = b["exact"] / unit
        assert np.array_equal(q, np.round(q)) and np.abs(q).max() < 2 ** 24
        return
    # integer cases: every term and partial sum is an integer of the output's unit, the sum of |terms| below 2^24 units
    row = np.abs(b["xi"]).sum(axis=1).max()
    assert np.abs(b["wi"]).max() <= 96 and np.abs(b["xi"]).max() <= (3 if epi == "epi" or case["M"] < 4 else 64)
    assert row * np.abs(b["wi"]).max() < 2 ** 24, "%s: %d * %d terms overflow 2^24 units" % (case["id"], row, np.abs(b["wi"]).max())
    if case["K"] * case["N"] >= 512:
        assert len(np.unique(b["codes"])) == 16
    if epi == "plain":
        if case["K"] >= 2048 and case["M"] * case["N"] >= 64:
            assert (b["expected"].astype(np.float64) != b["exact"]).any(), "%s: no output is rounded" % case["id"]
    else:
        assert np.abs(b["T"]).max() <= 2048
