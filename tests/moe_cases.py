"""Mixture-of-experts FFN cases and their reference (numpy only; read by test_moe_cpu.py, test_moe_route_gpu.py, test_moe_ffn_gpu.py).

Two restatements of the arithmetic include/llmie.h states for llmie_moe_route / llmie_moe_ffn:
  route() + ffn(rounded=False)  float64 throughout;
  ffn(rounded=True)             the same with the two fp16 roundings the arithmetic makes (a_j once, y once).
The bound of an accuracy test is twice the error of the second against the first (bounds()): it comes from the reference alone.

Router operands with exactly known logits (the method of exact_linear_cases.py): x[m, i] = 2^j(m) * integer (|integer| <= 3, j in
0 .. -2) and Wr[e, i] = 2^-s * integer (|integer| <= 3), so every product and every partial sum of a logit is an integer multiple
of 2^(j - s) below 2^24 of it: exact in fp32 in any order, through dot2 or an MFMA.  Selection, tie-breaks included, has one right
answer on the device and here.
  "ties"      random integers; the router rows of experts e with e % 8 in {0, 1, 2} of one block of 8 are copies of each other, so are
              those with e % 8 in {3, 4}: exact ties inside the selected set and across the k-th place in many rows (asserted per case
              by test_moe_cpu.py through tie_census()).
  "designed"  the routing is chosen first: row m's rank-j expert e gets the logit (k + 1 - j) / 4 (times the row's 2^j(m)) through one
              router coefficient +-1/4 at hidden position e % H (sign -1 for the experts of every second block of H, so e and e + H
              cannot both be chosen by one row); the other positions of x carry -1 / 0 / 1, so every other logit lies in
              [-1/4, 1/4], below the k-th selected one (2/4).  Gaps of 1/4 keep every selected weight a sizeable fraction.
              Distributions: "counts" leaves expert 0 without a pair and gives experts 1, 2, 3 exactly 16, 17 and 16 * 4 + 1 pairs;
              "one" sends every row to one expert.
Expert weights: gate_up ~ N(0, 1 / H), down ~ N(0, 1 / Ie), fp16; resid ~ N(0, 1) fp16 where a case has one.
"""
import zlib

import numpy as np

SOFTMAX_ALL = 1

# (E, k) of the issue; rows / H / Ie from its size lists, the smallest at which each kernel can go wrong: rows 1 .. 4 default to the
# GEMV route, 5 .. 16 reach it by force; 16 / 17 / 33 stand at and across the 16-pair tile; 300 rows x k / E >= 32 takes RT = 4.
# H = 2112 / Ie = 2112 (33 x 64): an odd number of 64-element steps, and 264 16-byte chunks per row = one past the 256 threads of a
# GEMV workgroup.  The last four cases reach the GEMV kernels' 4- and 8-chunk instantiations (K > 4096, K > 8192).
def _c(id, rows, H, Ie, E, k, kind="ties", dist=None, resid=True, flags=0):
    return dict(id=id, rows=rows, H=H, Ie=Ie, E=E, k=k, kind=kind, dist=dist, resid=resid, flags=flags)


CASES = [
    _c("r1_e1", 1, 64, 64, 1, 1),
    _c("r1_e8", 1, 256, 192, 8, 2, resid=False),
    _c("r2_e4", 2, 256, 192, 4, 1),
    _c("r4_e8", 4, 256, 192, 8, 2),
    _c("r5_h2112", 5, 2112, 64, 8, 2),
    _c("r16_i2112", 16, 64, 2112, 8, 2, resid=False),
    _c("r17_e128", 17, 256, 192, 128, 8),
    _c("r33_e128_all", 33, 256, 64, 128, 8, flags=SOFTMAX_ALL),
    _c("r100_counts", 100, 256, 192, 8, 2, kind="designed", dist="counts"),
    _c("r100_one", 100, 64, 64, 4, 1, kind="designed", dist="one"),
    _c("r300_counts_rt4", 300, 64, 192, 8, 2, kind="designed", dist="counts"),
    _c("r300_e128", 300, 256, 64, 128, 8, resid=False),
    _c("r16_e128_h64", 16, 64, 64, 128, 8, kind="designed", dist="spread"),
    _c("r2_h4160", 2, 4160, 64, 4, 1),
    _c("r2_i4160", 2, 64, 4160, 4, 1),
    _c("r1_h8256", 1, 8256, 64, 4, 1),
    _c("r1_i8256", 1, 64, 8256, 4, 1),
]
BY_ID = {c["id"]: c for c in CASES}
GEMV_MAX_ROWS, GEMV_DEFAULT_ROWS, RT4_PAIRS_PER_EXPERT = 16, 4, 32


def _rng(case, what):
    return np.random.default_rng(zlib.crc32(("%s/%s" % (case["id"], what)).encode()))


def tie_class(e):
    b, r = e // 8 * 8, e % 8
    return b if r in (0, 1, 2) else (b + 3 if r in (3, 4) else e)


def designed_assignment(case):
    """[rows, k] expert ids in rank order"""
    rows, E, k, H = case["rows"], case["E"], case["k"], case["H"]
    if case["dist"] == "one":
        assert k == 1
        return np.full((rows, 1), 2 % E, np.int64)
    if case["dist"] == "counts":
        assert k == 2 and E == 8 and rows >= 100
        first = [1] * 16 + [2] * 17 + [3] * 65
        first += [4 + i % 4 for i in range(rows - len(first))]
        second = [4 + (i * 3 + 1) % 4 for i in range(rows)]
        second = [s if s != f else 4 + (s - 4 + 1) % 4 for f, s in zip(first, second)]
        a = np.stack([np.array(first), np.array(second)], 1)
        # every second row swaps its ranks: an expert's pairs come from both ranks
        sw = np.arange(rows) % 2 == 1
        a[sw] = a[sw][:, ::-1]
        return a
    assert case["dist"] == "spread"
    rng = _rng(case, "assign")
    out = np.empty((rows, k), np.int64)
    for m in range(rows):
        while True:
            pick = rng.choice(E, k, replace=False)
            if len(set(int(p) % H for p in pick)) == k:   # e and e + H share a hidden position
                break
        out[m] = pick
    return out


def build(case):
    """operands of a case in storage types: x, router, gate_up, down fp16; resid fp16 or None"""
    rows, H, Ie, E, k = (case[n] for n in ("rows", "H", "Ie", "E", "k"))
    rng = _rng(case, "operands")
    jm = -(np.arange(rows) % 3)
    if case["kind"] == "ties":
        s = 3 + int(round(np.log2(H) / 2))
        xi = rng.integers(-3, 4, (rows, H))
        wi = rng.integers(-3, 4, (E, H))
        for e in range(E):
            wi[e] = wi[tie_class(e)]
    else:
        s = 2
        assign = designed_assignment(case)
        xi = rng.integers(-1, 2, (rows, H))
        wi = np.zeros((E, H), np.int64)
        for e in range(E):
            wi[e, e % H] = 1 if (e // H) % 2 == 0 else -1
        for m in range(rows):
            for j, e in enumerate(assign[m]):
                xi[m, e % H] = wi[e, e % H] * (k + 1 - j)
    assert np.abs(xi).max() <= 256 and np.abs(xi).sum(axis=1).max() * np.abs(wi).max() < 2 ** 24
    x = (xi * 2.0 ** jm[:, None]).astype(np.float16)
    router = (wi * 2.0 ** -s).astype(np.float16)
    assert np.array_equal(x.astype(np.float64), xi * 2.0 ** jm[:, None]) and np.array_equal(router.astype(np.float64), wi * 2.0 ** -s)
    gate_up = (rng.standard_normal((E, 2 * Ie, H)) / np.sqrt(H)).astype(np.float16)
    down = (rng.standard_normal((E, H, Ie)) / np.sqrt(Ie)).astype(np.float16)
    resid = rng.standard_normal((rows, H)).astype(np.float16) if case["resid"] else None
    return dict(case=case, x=x, router=router, gate_up=gate_up, down=down, resid=resid)


def logits(x, router):
    return x.astype(np.float64) @ router.astype(np.float64).T


def route(x, router, k, flags=0, r=None):
    """(expert ids [rows, k] int32, weights [rows, k] float64, logits [rows, E]): the k largest by (logit descending, id ascending), a
    NaN as -inf"""
    r = logits(x, router) if r is None else np.asarray(r, np.float64)
    rr = np.where(np.isnan(r), -np.inf, r)
    E = rr.shape[1]
    order = np.lexsort((np.broadcast_to(np.arange(E), rr.shape), -rr), axis=1)[:, :k]   # last key first: -logit, then the id
    sel = np.take_along_axis(rr, order, 1)
    with np.errstate(invalid="ignore"):
        num = np.exp(sel - sel[:, :1])
        den = np.exp(rr - sel[:, :1]).sum(axis=1, keepdims=True) if flags & SOFTMAX_ALL else num.sum(axis=1, keepdims=True)
    return order.astype(np.int32), num / den, r


def _f16(a):
    return a.astype(np.float16).astype(np.float64)


def ffn(b, experts, weights, rounded):
    """y [rows, H] float64 of the built case b under the given routing; rounded: with the fp16 roundings of the arithmetic (a_j, y)"""
    x = b["x"].astype(np.float64)
    rows, H = x.shape
    k = experts.shape[1]
    d = np.zeros((rows, k, H))
    for e in np.unique(experts):
        gu, dn = b["gate_up"][e].astype(np.float64), b["down"][e].astype(np.float64)
        Ie = dn.shape[1]
        m, j = np.nonzero(experts == e)
        t = x[m] @ gu.T
        a = t[:, :Ie] / (1.0 + np.exp(-t[:, :Ie])) * t[:, Ie:]
        if rounded:
            a = _f16(a)
        d[m, j] = a @ dn.T
    y = np.zeros((rows, H))
    for j in range(k):   # rank order
        y = y + weights[:, j:j + 1] * d[:, j]
    if b["resid"] is not None:
        y = y + b["resid"].astype(np.float64)
    return _f16(y) if rounded else y


def reference(b):
    """everything a test needs of a built case, computed once: routing, the float64 output, the fp16-rounded one and the bounds"""
    c = b["case"]
    experts, weights, r = route(b["x"], b["router"], c["k"], c["flags"])
    y64 = ffn(b, experts, weights, rounded=False)
    y16 = ffn(b, experts, weights, rounded=True)
    return dict(experts=experts, weights=weights, logits=r, y64=y64, y16=y16, bounds=bounds(y64, y16))


def rel_frobenius(got, exp):
    d = np.asarray(got, np.float64) - exp
    return float(np.sqrt((d * d).sum() / ((exp * exp).sum() + 1e-30)))


def bounds(y64, y16):
    """twice the error of the fp16-rounded restatement against the unrounded one: the largest element error and the relative
    Frobenius error.  The projection of an error on the signal is at most its relative Frobenius error (Cauchy-Schwarz), so the
    second bound holds for the projection too: a dropped or doubled expert weight gives a projection of the order of that weight."""
    return dict(max_abs=2.0 * float(np.abs(y16 - y64).max()), rel=2.0 * rel_frobenius(y16, y64))


def tie_census(r, k):
    """rows with an exact tie inside the selected set / across the k-th place"""
    E = r.shape[1]
    s = -np.sort(-r, axis=1)
    inside = (s[:, :k - 1] == s[:, 1:k]).any(axis=1) if k > 1 else np.zeros(len(r), bool)
    across = s[:, k - 1] == s[:, k] if k < E else np.zeros(len(r), bool)
    return int(inside.sum()), int(across.sum())


def pair_counts(experts, E):
    return np.bincount(experts.ravel(), minlength=E)


def tile_bound(rows, E, k, rt):
    pairs = rows * k
    return pairs // (16 * rt) + min(E, pairs)


def expected_plan(rows, H, Ie, E, k, flags=0, force=None):
    """(route, rt, tiles) by the thresholds include/llmie.h states"""
    gemv = force == "gemv" or (force is None and rows <= GEMV_DEFAULT_ROWS and H <= 16384 and Ie <= 16384)
    if gemv:
        return "gemv", 0, 0
    rt = 4 if rows * k // E >= RT4_PAIRS_PER_EXPERT else 1
    return "grouped", rt, tile_bound(rows, E, k, rt)
