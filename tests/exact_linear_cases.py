"""Projection cases whose one correct answer is known to the bit (numpy only; read by test_exact_linear_cpu.py and _gpu.py).

Every operand is a small integer times a power of two: activations x[m, k] = 2^j(m) * i (|i| <= 3; int4: <= 31), weight codes taken as
integers over the whole code range of their format, scales 2^e that differ from row to row and token to token by factors of 2 .. 128
and from group to group of an int4 row by 2 .. 8.  Every
product and every partial sum of such a projection is an integer multiple of the output's unit 2^U(m, n) below 2^24 of it, so it is
exact in fp32 in any order, under split-K, through an MFMA or a dot2; the result is the fp16 round-to-nearest-even of an exactly known
number, computed here as a float64 matmul over the integers (exact: every sum is far below 2^53) rounded once.  The tests demand
equality of bits.

Integer cases (dense), in two magnitudes:
  "plain"  large codes: |y| runs far past 2048 units, so the single rounding is exercised (the builder asserts it);
  "epi"    bias + residual: |acc + bias + residual| <= 2048 units, so the answer is exact whether a route rounds before or after the add.
Rows from the end of x: all positive (worst case of an offset start term such as -1152 * sum(x)), all zero, one outlier 2^6 times the
rest (plain; fp8 has none: its +-448 u marks every aligned run of 32).  fp8 activations are u(m) * {0, +-112, +-224, +-448} with
+-448 u first in every aligned run of 32 k, so amax / 448 == u(m) for the token and for every K slice of any launch, x / s == x * (1 / s)
on the grid; "runs" cases scale whole 2048-k regions of a row by 1, 1/4, 1/2, 1/8 so that K slices differ in amax and stay exact.

Probe cases (sparse; fp16 and fp8 weights): every finite e4m3 code (-0 and the subnormals included, the two NaN codes left out) or
random normal fp16 patterns plus +-0, 65504 and 2^-14, against activation rows of one or two non-zeros 7 * 2^j at the k edges of the
routes (first / last k, both sides of 8 .. 2048-element boundaries, the tail): each output is one or two exact products.

Conditions asserted for every case (conditions(), called by build()): operands and non-zero expected outputs normal, |y| <= 65504,
the sum of |terms| of every output below 2^24 units including the offset terms a route adds (offsets(), read from the kernels), the
code range of the format fully used.  The exponent ranges (j over 0..5, e over 0..7, one common shift per case) are the widest for
which 2^24-unit sums of K = 11008 dense terms still fit fp16's normal range at both ends.
"""
import zlib

import numpy as np

F16_MAX = 65504.0
J_SPAN, E_SPAN = 6, 8           # activation rows cycle over 2^0..2^5, weight rows over 2^0..2^-7 (before the case's common shift)
EPI_TERMS = 12                  # non-zeros per activation row of an "epi" case: 12 * 128 < 2048


def e4m3_table():
    """value of every OCP e4m3fn code (float64); NaN at 0x7f / 0xff"""
    b = np.arange(256)
    sgn, ex, mant = b >> 7, (b >> 3) & 0xF, b & 7
    v = np.where(ex == 0, (mant / 8.0) * 2.0 ** -6, (1 + mant / 8.0) * 2.0 ** (ex.astype(np.float64) - 7))
    v = np.where(sgn == 1, -v, v)
    v[[0x7F, 0xFF]] = np.nan
    return v


E4M3 = e4m3_table()
E4M3_FINITE = np.array([c for c in range(256) if c not in (0x7F, 0xFF)], np.uint8)
_E4M3_OF_INT = {int(E4M3[c]): c for c in range(0x7F) if E4M3[c] == int(E4M3[c]) and c != 0}
_E4M3_OF_INT.update({-k: c | 0x80 for k, c in list(_E4M3_OF_INT.items())})
_E4M3_OF_INT[0] = 0


def e4m3_codes_of_ints(a):
    lut = np.zeros(31, np.uint8)
    for v in range(-15, 16):
        lut[v + 15] = _E4M3_OF_INT[v]
    return lut[a + 15]


# Offset terms the routes add on top of x . w, as (elements of one fp32 chain that carries them, bound of the coefficients of one
# element).  gemm_kernels.cuh chunk_dot<8>: the chain of a thread multiplies 1152 + w (<= 1279) and starts at -1152 * sum(x) over its
# slice of ceil(K / 16 / 256) chunks of 16; chunk_dot<4>: a 32-weight chunk multiplies 1024 + n (<= 1039) or (1024 + 16 n) / 16 and
# starts at -(1032 | 1152 / 16) * x.  Every other route subtracts its offset in fp16, exactly, before the multiply (dequant8,
# dequant_i8x8, off8 / off72 of gemm_kernels.cuh and pk_gemm.cuh): no offset term reaches an accumulator.
def offsets(case):
    if case["route"] == "gemv_ksplit" and case["fmt"] == "int8":
        return 16 * -(-case["K"] // (16 * 256)), 1152 + 1279
    if case["route"] in ("gemv_ksplit", "int4_chunks") and case["fmt"] == "int4":
        return 32, 1032 + 1039
    return 0, 0


def _rng(case, epi):
    return np.random.default_rng(zlib.crc32(("%s/%s" % (case["id"], epi)).encode()))


def _pack4(nib):
    return (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8)


def edge_ks(K):
    """k positions at the edges of the routes: first / last, both sides of every 8 .. 2048 boundary nearest the start, the middle and the
    end of the row, the tail"""
    ks = [0, K - 1, K - 2, 1]
    for b in (8, 16, 32, 64, 128, 256, 512, 1024, 2048):
        for at in (b, (K // 2) // b * b, (K - 1) // b * b):
            ks += [at - 1, at]
    out = []
    for k in ks:
        if 0 <= k < K and k not in out:
            out.append(k)
    return out


def _activations_int(case, epi, rng):
    """(xi integers [M, K], jm exponents [M]): x = xi * 2^jm"""
    M, K = case["M"], case["K"]
    jm = np.arange(M) % J_SPAN
    if case["fmt"] == "fp8":
        jm = jm + 4                                      # x = u * 16 * {0, 7, 14, 28}
        if epi == "plain":
            xi = rng.choice(np.array([0, 7, 14, 28, -7, -14, -28]), (M, K))
        else:
            xi = np.zeros((M, K), np.int64)
            xi[:, K - 1] = 7 * rng.choice(np.array([1, -1]), M)            # the last k counts (its weight is non-zero)
        xi[:, 0::32] = 28 * rng.choice(np.array([1, -1]), (M, len(range(0, K, 32))))
        if case.get("runs"):                             # whole 2048-k regions at 1, 1/4, 1/2, 1/8 of the row's scale
            assert epi == "plain"
            xi = xi * 8
            jm = jm - 3
            xi = xi // np.array([1, 4, 2, 8])[(np.arange(K) // 2048) % 4][None, :]
        xi[M - 1] = np.abs(xi[M - 1])
        if M >= 3:
            xi[M - 2] = 0
        return xi, jm
    if epi == "plain":
        # int4: |i| up to 31, so that a 128-k partial of one group (|n - 8| <= 8) passes 2048 units and would be rounded as fp16
        top = 31 if case["fmt"] == "int4" else 3
        xi = rng.integers(-top, top + 1, (M, K))
        xi[M - 1] = rng.integers(1, top + 1, K)
        if M >= 4:
            xi[M - 3] = rng.integers(-1, 2, K)
            xi[M - 3, rng.integers(0, K)] = 64
    else:
        xi = np.zeros((M, K), np.int64)
        for m in range(M):
            ks = np.concatenate([[0, K - 1], rng.choice(np.arange(1, K - 1), EPI_TERMS - 2, replace=False)])
            xi[m, ks] = rng.choice(np.array([1, -1]), EPI_TERMS)
        xi[M - 1] = np.abs(xi[M - 1])
    if M >= 3:
        xi[M - 2] = 0
    return xi, jm


def _weights_int(case, epi, rng):
    """(wi integers [N, K] in units of 2^en[n], en [N], codes dict): w[n, k] = wi * 2^en"""
    N, K, fmt = case["N"], case["K"], case["fmt"]
    en = -(np.arange(N) * 3 % E_SPAN)
    if fmt == "int8":
        q = rng.integers(-128, 128, (N, K)).astype(np.int8)
        return q.astype(np.int64), en, dict(q=q)
    if fmt == "int4":
        nib = rng.integers(0, 16, (N, K)).astype(np.uint8)
        G = K // case["group"]
        d = rng.integers(0, 4, (N, G))                                     # group scales 2^(en + d): a span of 8 per row
        return (nib.astype(np.int64) - 8) * 2 ** np.repeat(d, case["group"], axis=1), en, dict(nib=nib, d=d)
    if fmt == "fp8":
        if epi == "plain":
            wi = rng.integers(-15, 16, (N, K))
        else:                                            # sparse +-1: |acc| <= 28 * (hits of 64 non-zeros per row) stays small
            wi = np.zeros((N, K), np.int64)
            for n in range(N):
                ks = rng.choice(K, min(64, K // 8), replace=False)
                wi[n, ks] = rng.choice(np.array([1, -1]), len(ks))
            wi[:, [0, K - 1]] = rng.choice(np.array([1, -1]), (N, 2))
        return wi, en, dict(q=e4m3_codes_of_ints(wi))
    wi = rng.integers(-255, 256, (N, K)) if epi == "plain" else rng.integers(-128, 128, (N, K))
    return wi, en, {}


def build(case, epi, check=True):
    """operands in the format's storage + the exact expected fp16 output of case (a dict of CASES) in magnitude "plain" or "epi"
    ("epi": with bias and residual; the in-place form uses the same operands)"""
    if case["kind"] == "probe":
        assert epi == "plain"
        out = _build_probe(case)
    else:
        out = _build_int(case, epi)
    out.update(case=case, epi=epi)
    if check:
        conditions(out)
    return out


def _build_int(case, epi):
    rng = _rng(case, epi)
    M, K, N, fmt = case["M"], case["K"], case["N"], case["fmt"]
    xi, jm = _activations_int(case, epi, rng)
    wi, en, codes = _weights_int(case, epi, rng)
    S = xi.astype(np.float64) @ wi.astype(np.float64).T                     # exact: integers far below 2^53
    T, bi, ri = S, None, None
    if epi == "epi":
        jtop = jm.max()
        if case["entry"] != "packed":                                      # the packed entry has no bias
            bi = rng.integers(-4, 5, N)
            T = T + bi[None, :] * 2.0 ** (jtop - jm)[:, None]               # bias[n] = bi * 2^(jtop + en): whole units of every row
        ri = rng.integers(-600, 601, (M, N)).astype(np.float64)
        ri = np.clip(ri, -2048 - T, 2048 - T)                               # |acc + bias + residual| <= 2048 units
        assert np.abs(ri).max() <= 2048
        T = T + ri
    # one common shift of the weight scales puts the largest |y| just below 65504
    top = np.abs(T * 2.0 ** (jm[:, None] + en[None, :])).max()
    c = int(np.floor(np.log2(F16_MAX / top)))
    en = en + c
    U = jm[:, None] + en[None, :]
    x = (xi * 2.0 ** jm[:, None]).astype(np.float16)
    assert np.array_equal(x.astype(np.float64), xi * 2.0 ** jm[:, None])
    out = dict(x=x, xi=xi, jm=jm, wi=wi, en=en, S=S, T=T, U=U, expected=(T * 2.0 ** U + 0.0).astype(np.float16), exact=T * 2.0 ** U,
               bias=None, residual=None)
    if fmt == "f16":
        out.update(w=(wi * 2.0 ** en[:, None]).astype(np.float16), scale=None, deq=wi * 2.0 ** en[:, None])
    elif fmt == "int8":
        out.update(w=codes["q"], scale=(2.0 ** en).astype(np.float16), deq=wi * 2.0 ** en[:, None])
    elif fmt == "int4":
        out.update(w=_pack4(codes["nib"]), nib=codes["nib"], scale=(2.0 ** (en[:, None] + codes["d"])).astype(np.float16),
                   deq=wi * 2.0 ** en[:, None])
    else:
        out.update(w=codes["q"], scale=(2.0 ** en).astype(np.float32), deq=wi * 2.0 ** en[:, None])
    if bi is not None:
        out["bias"] = (bi * 2.0 ** (jm.max() + en)).astype(np.float16)
    if ri is not None:
        out["residual"] = (ri * 2.0 ** U).astype(np.float16)
    return out


def _build_probe(case):
    rng = _rng(case, "probe")
    M, K, N, fmt = case["M"], case["K"], case["N"], case["fmt"]
    ks = edge_ks(K)
    x = np.zeros((M, K), np.float64)
    ks = ks[:len(ks) // 2 * 2]                           # even positions: "A" columns, odd positions: "B" columns (disjoint)
    hit_a, hit_b = [], []
    for m in range(M):                                   # rows take the edges in turn, two per row: 2 M edges where M is small
        k1, k2 = ks[(2 * m) % len(ks)], ks[(2 * m + 1) % len(ks)]
        # fp8: both non-zeros 7 * 2^j (the row's amax: code 448).  fp16: 7 / 16 on the A column (meets 65504), 7 or 14 on the B column
        # (meets 2^-14): with weight exponents 2^-2 .. 2^1 the two products' units differ by at most 2^8, 14 + 8 + 1 < 24 bits
        j = m % 8 - 4
        x[m, k1] = 7 * 2.0 ** (j if fmt == "fp8" else -4)
        if m % 3 != 2:
            x[m, k2] = 7 * 2.0 ** (j if fmt == "fp8" else m % 2) * (1 if m % 4 < 2 else -1)
            hit_b.append(k2)
        hit_a.append(k1)
    hit_a, hit_b = sorted(set(hit_a)), sorted(set(hit_b))
    hit = sorted(hit_a + hit_b)
    if fmt == "fp8":
        q = E4M3_FINITE[rng.integers(0, len(E4M3_FINITE), (N, K))]
        for i, k in enumerate(hit):                      # every finite code meets every probed k within 254 weight rows
            if N >= len(E4M3_FINITE):
                q[:, k] = np.resize(np.roll(E4M3_FINITE, 37 * i), N)
        e = np.arange(N) % 4
        scale = (2.0 ** -e).astype(np.float32)
        deq = E4M3[q] * scale[:, None].astype(np.float64)
        w = q
    else:
        # random normal fp16 patterns, and the edges of the format on the probed columns of the first rows, one product per output there:
        # +-65504 on A against +-0 on B, +-0 on A against +-2^-14 on B, 1 + 2^-10 on both
        bits = (rng.integers(0, 2, (N, K)) << 15) | (rng.integers(13, 17, (N, K)) << 10) | rng.integers(0, 1024, (N, K))
        w = bits.astype(np.uint16).view(np.float16)
        sp_a = np.array([0x7BFF, 0xFBFF, 0x0000, 0x8000, 0x3C01], np.uint16).view(np.float16)
        sp_b = np.array([0x0000, 0x8000, 0x0400, 0x8400, 0x3C01], np.uint16).view(np.float16)
        for n in range(min(N, len(sp_a))):
            w[n, hit_a], w[n, hit_b] = sp_a[n], sp_b[n]
        scale, deq = None, w.astype(np.float64)
    exact = x @ deq.T                                    # one or two exact products per output
    return dict(x=x.astype(np.float16), w=w, scale=scale, deq=deq, bias=None, residual=None, exact=exact,
                expected=(exact + 0.0).astype(np.float16), hit=hit)


def _normal16(a):
    a = np.abs(np.asarray(a, np.float64))
    a = a[a != 0]
    return a.size == 0 or (a.min() >= 2.0 ** -14 and a.max() <= F16_MAX)


def conditions(b):
    """the conditions of the module docstring, asserted (not measured) for a built case"""
    case, epi = b["case"], b["epi"]
    fmt = case["fmt"]
    assert _normal16(b["x"]) and _normal16(b["exact"]), "%s: operand or output outside fp16's normal range" % case["id"]
    assert np.array_equal(b["expected"].astype(np.float64) != 0, b["exact"] != 0)
    if b["scale"] is not None:
        s = np.abs(b["scale"].astype(np.float64))
        assert s.min() >= (2.0 ** -14 if b["scale"].dtype == np.float16 else 2.0 ** -126) and s.max() <= F16_MAX
    if fmt == "f16":
        assert _normal16(b["w"])
    for name in ("bias", "residual"):
        if b[name] is not None:
            assert _normal16(b[name]), name
    if case["kind"] == "probe":
        # each output: two products 7 * 2^j * w of at most 14 significant bits whose units differ by at most 2^14 (e4m3: 2^-9 .. 2^5
        # of a 4-bit mantissa) or 2^7 (fp16 patterns of eight exponents; the specials meet one product or an equal partner)
        cols = b["w"][:, b["hit"]]
        if fmt == "fp8":
            if case["N"] >= len(E4M3_FINITE):
                for i in range(len(b["hit"])):
                    assert set(cols[:, i].tolist()) == set(E4M3_FINITE.tolist()), "a finite e4m3 code misses a probed k"
            assert not np.isin(b["w"], [0x7F, 0xFF]).any()
        else:
            v = cols.view(np.uint16)
            assert all((v == p).any() for p in (0x0000, 0x8000, 0x7BFF, 0xFBFF, 0x0400, 0x8400)), "an fp16 edge pattern misses the probed k"
            e = (b["w"].view(np.uint16) >> 10) & 31
            assert (e != 31).all() and ((e != 0) | ((b["w"].view(np.uint16) & 0x7FFF) == 0)).all(), "a weight is not normal or zero"
        return
    # integer cases: sum of |terms| in units of 2^U, the cheap bound (largest row of |xi|) * (largest |wi|)
    row = np.abs(b["xi"]).sum(axis=1).max()
    assert row * np.abs(b["wi"]).max() < 2 ** 24, "%s: %d * %d terms overflow 2^24 units" % (case["id"], row, np.abs(b["wi"]).max())
    n_el, coef = offsets(case)
    assert n_el * np.abs(b["xi"]).max() * coef < 2 ** 24, "%s: the route's offset terms overflow 2^24 units" % case["id"]
    if epi == "plain":
        assert np.abs(b["T"]).max() > 4 * 2048, "%s: no output is rounded" % case["id"]
        if fmt == "int8":
            assert len(np.unique(b["w"])) == 256
        if fmt == "int4":
            assert len(np.unique(b["nib"])) == 16
        if fmt == "fp8":
            assert len(np.unique(b["w"])) == 31
    else:
        assert np.abs(b["T"]).max() <= 2048
    assert np.abs(b["exact"]).max() <= F16_MAX


def _c(id, fmt, route, M, K, N, group=0, ws="auto", xoff=0, entry="linear", kind="int", **kw):
    return dict(id=id, fmt=fmt, route=route, M=M, K=K, N=N, group=group, ws=ws, xoff=xoff, entry=entry, kind=kind, **kw)


# ---- fp16 weights: every route llmie_linear reaches without SwiGLU.  plan: llmie_gemm256_tiles of the shape (tiles256 forms) ----
F16 = [
    _c("f16_gemv", "f16", "gemv_ksplit", 5, 4096, 1000),
    _c("f16_gemv_k11008", "f16", "gemv_ksplit", 2, 11008, 1000),
    _c("f16_gemv_lds", "f16", "gemv_lds", 3, 10240, 504),                   # K past the K-split register budget of 3 rows
    _c("f16_skinny_nows", "f16", "skinny", 40, 4096, 1000, ws=None),
    _c("f16_skinny_k1056", "f16", "skinny", 33, 1056, 1000),                # K % 128 != 0: no split-K form
    _c("f16_splitk0_m20", "f16", "splitk", 20, 4096, 1000),
    _c("f16_splitk2_m50", "f16", "splitk", 50, 4096, 1000),
    _c("f16_splitk1_m100", "f16", "splitk", 100, 4096, 1000),
    _c("f16_splitk1_m150", "f16", "splitk", 150, 4096, 1000),               # two passes: 128 + 22 rows
    _c("f16_splitk_k11008", "f16", "splitk", 20, 11008, 1000),
    _c("f16_passes_m200", "f16", "splitk_passes", 200, 4096, 1000),
    _c("f16_midtiles_m400", "f16", "tiles256_part", 400, 1024, 1000),
    _c("f16_midtiles_nows", "f16", "tiles256_part", 250, 4096, 1000, ws=None),
    _c("f16_tiles128_nows", "f16", "tiles128", 100, 4096, 1000, ws=None),
    _c("f16_tiles128_k1088", "f16", "tiles128", 150, 1088, 1000, ws=None),
    _c("f16_generic_k1001", "f16", "generic", 70, 1001, 1000),
    _c("f16_generic_xoff", "f16", "generic", 130, 1024, 1000, xoff=1),
    _c("f16_tiles256_narrow", "f16", "tiles256", 2048, 512, 4096, plan="8p 128x32@0"),
    _c("f16_tiles256_wide", "f16", "tiles256", 4096, 256, 4096, plan="8p 256x16@0"),
    _c("f16_tiles256_two", "f16", "tiles256", 4096, 256, 4352, plan="8p 256x16@0 128x2@4096"),
]
WQ = [
    _c("i8_gemv", "int8", "gemv_ksplit", 7, 4096, 1000),
    _c("i8_gemv_k11008", "int8", "gemv_ksplit", 2, 11008, 1000),
    _c("i8_skinny_nows", "int8", "int8_skinny", 40, 4096, 1000, ws=None),
    _c("i8_skinny_k1088", "int8", "int8_skinny", 40, 1088, 1000),
    _c("i8_splitk_m100", "int8", "int8_splitk", 100, 4096, 1000),
    _c("i8_splitk_m150", "int8", "int8_splitk", 150, 4096, 1000),
    _c("i8_splitk_k11008", "int8", "int8_splitk", 20, 11008, 1000),
    _c("i8_midpasses", "int8", "int8_splitk_passes", 200, 11008, 1000),
    _c("i8_image_m300", "int8", "image_prefill+tiles256_part", 300, 4096, 1000),
    _c("i8_image_k1152", "int8", "image_last+tiles128", 100, 1152, 1000),
    _c("i8_g8p", "int8", "g8p", 2048, 512, 4096, plan="8p 128x32@0"),
    _c("i4_gemv", "int4", "gemv_ksplit", 3, 4096, 1000, group=128),
    _c("i4_gemv_g32", "int4", "gemv_ksplit", 3, 4096, 1000, group=32),
    _c("i4_splitk_m50", "int4", "int4_splitk", 50, 4096, 1000, group=128),
    _c("i4_splitk_m150", "int4", "int4_splitk", 150, 4096, 1000, group=128),
    _c("i4_splitk_k11008", "int4", "int4_splitk", 50, 11008, 1000, group=128),
    _c("i4_chunks_g64", "int4", "int4_chunks", 20, 4096, 1000, group=64),
    _c("i4_chunks_nows", "int4", "int4_chunks", 40, 1024, 1000, group=128, ws=None),
    _c("i4_chunks_k1152", "int4", "int4_chunks", 20, 1152, 1000, group=128),
    _c("i4_image_m300", "int4", "image_prefill+tiles256_part", 300, 4096, 1000, group=128),
    _c("i4_image_g64", "int4", "image_prefill+tiles256_part", 200, 4096, 1000, group=64),
]
# ---- llmie_linear_fp8: the form follows from the shape (linear.hip, plan_linear_fp8): M <= 8 and ksplit_eligible(M, K, 8) -> GEMV; tiled: M > 8,
# K % 128 == 0, N % 4 == 0 and (gemm256_fills(M, N) or, from 129 rows, the time model rounds * K / 128 * 1.15 < passes * (N K / 8.3e6 + 17))
# -> gemm256 e4m3; else split-K skinny in passes of 128 rows (K % 256 == 0).  rule: what the CPU test recomputes for the shape.
FP8 = [
    _c("fp8_gemv", "fp8", "fp8_gemv", 5, 4096, 1000),
    _c("fp8_gemv_k11008", "fp8", "fp8_gemv", 2, 11008, 1000),
    _c("fp8_splitk_m5_k11008", "fp8", "fp8_splitk", 5, 11008, 1000),         # M <= 8 past the GEMV's register budget: split-K
    _c("fp8_splitk_m20", "fp8", "fp8_splitk", 20, 4096, 1000),
    _c("fp8_splitk_m32", "fp8", "fp8_splitk", 32, 4096, 1000),
    _c("fp8_splitk_k11008", "fp8", "fp8_splitk", 20, 11008, 1000),
    _c("fp8_passes_m72", "fp8", "fp8_splitk", 72, 4096, 1000),
    _c("fp8_passes_m150", "fp8", "fp8_splitk", 150, 4096, 1000),
    _c("fp8_gemm256_fills", "fp8", "fp8_gemm256", 2048, 512, 4096, plan="8p 128x32@0"),
    _c("fp8_gemm256_part", "fp8", "fp8_gemm256", 400, 1152, 1000, plan="8p 128x8@0"),
]
PACKED = [_c("pk_%s_m%d_k%d" % (f, M, K), f, "packed", M, K, 1000, group=128 if f == "int4" else 0, entry="packed")
          for f in ("f16", "int8", "int4", "fp8") for M in (3, 16, 17, 32) for K in (4096, 11008)]
PACKED += [_c("pk_fp8_runs_m17_k11008", "fp8", "packed", 17, 11008, 1000, entry="packed", runs=True),
           _c("fp8_splitk_runs", "fp8", "fp8_splitk", 20, 11008, 1000, runs=True)]
CASES = F16 + WQ + FP8 + PACKED
PROBES = [dict(c, id=c["id"] + "_probe", kind="probe") for c in CASES if c["fmt"] in ("f16", "fp8") and not c.get("runs")
          and c["M"] <= 400]


def epilogues(case):
    """magnitudes / epilogue forms a case runs with: plain everywhere; bias + residual and the in-place residual on integer cases"""
    return ("plain",) if case["kind"] == "probe" or case.get("runs") else ("plain", "epi")
