"""The exact projection cases of tests/exact_linear_cases.py, checked without a GPU.

  * every case meets the conditions that make its arithmetic exact (exact_linear_cases.conditions);
  * every case id takes the route it names (llmie_linear_route; for llmie_linear_fp8 also by fp8_form() below, an independent
    restatement of plan_linear_fp8's rule that has to agree with the route query over the grid of test_linear_routes_cpu.py; the K
    split of the packed entry from its workspace query), and the cases name every route of the planner's vocabulary that is reachable
    without SwiGLU;
  * seeded defects, applied to a numpy restatement of the projection (project()), change at least one output bit in every case where
    they can be expressed (DEFECTS: which operands each needs).

Which of these defects the earlier recipe lets through (Gaussian x, Gaussian w / sqrt(K), the project's own quantisers, every element
within 2e-3 + 2e-3 |y| of the float64 reference; fp8: the statistical bound of test_linear_packed_fp8_matches_e4m3_emulation) is
computed by test_defects_the_gaussian_recipe_lets_through and printed; recorded, not asserted.  As computed (M 16, K 4096, N 256):
    let through:  nibble0_as_plus8 and int8_m128_clamped (the codes never occur), e4m3_neg_zero_as_nan (never occurs),
                  e4m3_subnormal_flushed, partial128_fp16 and slab_fp16 in all four formats
    caught:       nibble_not_offset, neighbour_group_scale, neighbour_row_scale, neighbour_token_scale, k_tail_dropped,
                  e4m3_448_as_240, wrong_slice_scale, residual_after_write
(The recipe does see a wrong scale or a dropped k where the defect is total, as here: every row, every group.  What it cannot see is
anything worth a few fp16 ulps, and any code its quantisers do not emit.)
"""
import numpy as np
import pytest

import exact_linear_cases as E

W_CODE = {"f16": 0, "int8": 1, "int4": 2, "fp8": 3}
X, W, SCALE, Y, BIAS, RESIDUAL, WORKSPACE = (0x10000000 * (i + 1) for i in range(7))
ALL = E.CASES + E.PROBES


@pytest.fixture(scope="module")
def built(llmie):
    llmie.build()
    return llmie


# ---------------------------------------------------------------- routes
def _route(lib, case, epi):
    fmt = W_CODE[case["fmt"]]
    if case["fmt"] == "fp8":   # (its own size query: the activation part, then the slabs)
        nbytes = lib.llmie_linear_fp8_workspace_bytes(case["M"], case["K"], case["N"])
    else:
        nbytes = lib.llmie_linear_workspace_bytes(fmt, case["M"], case["K"], case["N"]) if case["ws"] == "auto" else 0
    br = epi == "epi"
    r = lib.llmie_linear_route(fmt, X + 2 * case["xoff"], W, SCALE, Y, case["M"], case["K"], case["N"], 0, case["group"],
                               BIAS if br else None, RESIDUAL if br else None, WORKSPACE if nbytes else None, nbytes)
    return r.decode() if r is not None else "refused"


def fp8_form(M, K, N):
    """the form llmie_linear_fp8 runs for 16-byte aligned operands and a workspace of the queried size (linear.hip: plan_linear_fp8,
    ksplit_form, gemm256_fills, gemm256_narrow_rounds, gemm8p_fits), restated"""
    ceil = lambda a, b: -(-a // b)
    tm = ceil(M, 256)
    fills = tm * ceil(N, 256) >= 192 or tm * ceil(N, 128) >= 128
    tiled = M > 8 and K % 128 == 0 and N % 4 == 0
    if tiled and not fills:
        fits = (N + 512) * K < 2 ** 32
        rounds = ceil(tm * ceil(N, 128), 256)
        tiled = M > 128 and fits and rounds * (K // 128) * 1.15 < ceil(M, 128) * (N * K / 8.3e6 + 17.0)
    if not tiled and (K % 256 or K < 512):
        return "refused"
    xc = ceil(K // 16, 256)
    if M <= 8 and K % 16 == 0 and xc <= 3 and M * xc * 2 <= 16:
        return "fp8_gemv"
    return "fp8_gemm256" if tiled else "fp8_splitk"


@pytest.mark.parametrize("case", ALL, ids=[c["id"] for c in ALL])
def test_case_takes_the_route_it_names(built, case):
    lib = built.lib()
    if case["entry"] == "packed":
        # K 11008 is past the register-resident activation slice: the launch splits K over workgroups and needs slabs
        slabs = lib.llmie_linear_packed_workspace_bytes(W_CODE[case["fmt"]], case["M"], case["K"], case["N"])
        assert (slabs > 0) == (case["K"] == 11008)
    elif case["fmt"] == "fp8":
        assert fp8_form(case["M"], case["K"], case["N"]) == case["route"]
        for epi in E.epilogues(case):
            assert _route(lib, case, epi) == case["route"]
    else:
        for epi in E.epilogues(case):
            assert _route(lib, case, epi) == case["route"]
    if "plan" in case:
        assert built.gemm256_tiles("plain", {"f16": "f16", "int8": "int8", "fp8": "e4m3"}[case["fmt"]], case["M"], case["N"], case["K"]) == case["plan"]


def test_fp8_form_agrees_with_the_route_query(built):
    """over the aligned, workspace-given part of the grid of test_linear_routes_cpu.py; all four answers occur"""
    from collections import Counter
    import test_linear_routes_cpu as R
    lib, seen = built.lib(), Counter()
    for K, N in R.SHAPES:
        for M in R.MS:
            form = fp8_form(M, K, N)
            seen[form] += 1
            assert R._route_fp8(lib, M, K, N, "plain", "auto", 0) == form, (M, K, N)
    assert seen == {"fp8_gemm256": 174, "refused": 90, "fp8_splitk": 56, "fp8_gemv": 32}, seen


def test_fp8_workspace_query_sizes_the_slabs_of_every_split_k_case(built):
    """llmie_linear_fp8 runs split-K below the tiled sizes, also for M <= 8 where K is past the GEMV's register budget (3 .. 8 rows of
    K = 11008): the query has to count the slabs there, or the call is refused with the workspace the query itself sized"""
    q = built.lib().llmie_linear_fp8_workspace_bytes
    for M, K, N in [(c["M"], c["K"], c["N"]) for c in ALL if c["fmt"] == "fp8"] + [(m, 11008, 4096) for m in range(1, 10)]:
        form = fp8_form(M, K, N)
        assert form != "fp8_gemv" or q(M, K, N) == q(M, K, 0), (M, K, N)    # (the tiled sizes reserve slabs they do not use)
        if form == "fp8_splitk":
            assert q(M, K, N) >= q(M, K, 0) + 2 * min(M, 128) * N * 4      # at least two fp32 slabs of one pass


def test_cases_cover_the_vocabulary():
    named = {c["route"] for c in ALL}
    f16 = {"gemv_ksplit", "gemv_lds", "splitk", "splitk_passes", "skinny", "tiles256", "tiles256_part", "tiles128", "generic"}
    wq = {"g8p", "int8_splitk_passes", "int8_splitk", "int8_skinny", "int4_splitk", "int4_chunks", "gemv_ksplit",
          "image_prefill+tiles256_part", "image_last+tiles128"}
    fp8 = {"fp8_gemv", "fp8_splitk", "fp8_gemm256"}
    assert f16 | wq | fp8 | {"packed"} <= named, (f16 | wq | fp8) - named
    for fmt in ("int8", "int4"):     # both quantised formats on the GEMV, and on an fp16 image
        assert any(c["fmt"] == fmt and c["route"] == "gemv_ksplit" for c in ALL)
        assert any(c["fmt"] == fmt and c["route"].startswith("image_") for c in ALL)
    assert {c["group"] for c in ALL if c["fmt"] == "int4"} == {32, 64, 128}
    assert {c["plan"].split("@")[0] for c in E.F16 if "plan" in c} == {"8p 128x32", "8p 256x16"} and \
        any(" 128x" in c["plan"].split("@", 1)[1] for c in E.F16 if "plan" in c)    # narrow, wide, wide + narrow ranges


# ---------------------------------------------------------------- a numpy restatement of the projection, with seeded defects
def _to_e4m3(v):
    """round-to-nearest-even onto the e4m3 grid (saturating at 448), returned as values"""
    grid = E.E4M3[:0x7F]                                  # codes 0 .. 0x7e ascending
    a = np.minimum(np.abs(v), 448.0)
    hi = np.clip(np.searchsorted(grid, a), 1, len(grid) - 1)
    lo = hi - 1
    up = (a - grid[lo] > grid[hi] - a) | ((a - grid[lo] == grid[hi] - a) & (hi % 2 == 0))
    return np.sign(v) * np.where(up, grid[hi], grid[lo])


def project(b, defect=None, mi=None, ni=None, in_place=False, slices=1):
    """y (fp16) of the projection of a built case (or of operands in the same layout) on rows mi and weight rows ni, as the kernels
    define it: integer codes, scales, fp32-or-better accumulation, one rounding; `defect` names one of DEFECTS"""
    case = b["case"]
    fmt, K, group = case["fmt"], case["K"], case["group"]
    M, N = b["x"].shape[0], b["w"].shape[0]
    mi = np.arange(M) if mi is None else mi
    ni = np.arange(N) if ni is None else ni
    x = b["x"].astype(np.float64)[mi]
    table = E.E4M3.copy()
    if defect == "e4m3_subnormal_flushed":
        table[[c for c in range(256) if (c >> 3) & 0xF == 0]] = 0.0
    if defect == "e4m3_neg_zero_as_nan":
        table[0x80] = np.nan
    if defect == "e4m3_448_as_240":
        table[0x7E], table[0xFE] = 240.0, -240.0
    row_scale = np.ones(N) if b["scale"] is None or fmt == "int4" else b["scale"].astype(np.float64)
    if defect == "neighbour_row_scale":
        row_scale = np.roll(row_scale, 1)
    row_scale = row_scale[ni]
    if fmt == "f16":
        w = b["w"][ni].astype(np.float64)
    elif fmt == "int8":
        w = b["w"][ni].astype(np.float64)
        if defect == "int8_m128_clamped":
            w = np.maximum(w, -127)
    elif fmt == "int4":
        nib = np.stack([b["w"] & 0xF, b["w"] >> 4], axis=-1).reshape(N, K).astype(np.float64)
        w = nib - 8
        if defect == "nibble0_as_plus8":
            w[nib == 0] = 8
        if defect == "nibble_not_offset":
            w = nib
        sg = b["scale"].astype(np.float64)
        if defect == "neighbour_group_scale":
            sg = np.roll(sg, 1, axis=1)
        if defect == "neighbour_row_scale":
            sg = np.roll(sg, 1, axis=0)
        w = (w * np.repeat(sg, group, axis=1))[ni]
    else:
        w = table[b["w"][ni]]
    if defect == "slab_fp16":
        slices = max(slices, 4)                           # a split-K launch: four slabs
    bounds = [0, K] if slices == 1 else [0] + [K * s // slices // 64 * 64 for s in range(1, slices)] + [K]
    if defect == "k_tail_dropped":
        bounds[-1] = K - 1
    parts = []
    xs_all = []
    for s in range(len(bounds) - 1):
        k0, k1 = bounds[s], bounds[s + 1]
        xa = x[:, k0:k1]
        xs = np.ones(len(mi))
        if fmt == "fp8":                                  # per token (per slice of a K-split launch): scale amax / 448, codes on the grid
            amax = np.abs(b["x"].astype(np.float64)[:, k0:k1]).max(axis=1)
            xs = np.where(amax > 0, amax / 448.0, 1.0)
            if defect == "neighbour_token_scale":
                xs_use = np.roll(xs, 1)[mi]
            else:
                xs_use = xs[mi]
            xs = xs[mi]
            q = _to_e4m3(xa / xs[:, None])
            if defect in ("e4m3_448_as_240",):
                q = np.where(np.abs(q) == 448, np.sign(q) * 240, q)
            xa, xs = q, xs_use
        xs_all.append(xs)
        if defect == "partial128_fp16":
            p = np.zeros((len(mi), len(ni)))
            for kk in range(0, k1 - k0, 128):
                blk = (xa[:, kk:kk + 128] @ w[:, k0 + kk:min(k0 + kk + 128, k1)].T) * row_scale[None, :] * xs[:, None]
                p += blk.astype(np.float16).astype(np.float64)
            parts.append(p / (row_scale[None, :] * xs[:, None]))
        else:
            parts.append(xa @ w[:, k0:k1].T)
    if defect == "wrong_slice_scale":
        xs_all = xs_all[1:] + xs_all[:1]
    acc = np.zeros((len(mi), len(ni)))
    for p, xs in zip(parts, xs_all):
        slab = p * row_scale[None, :] * xs[:, None]
        if defect == "slab_fp16":
            slab = slab.astype(np.float16).astype(np.float64)
        acc += slab
    v = acc
    if b["bias"] is not None:
        v = v + b["bias"].astype(np.float64)[ni][None, :]
    if b["residual"] is not None:
        r = b["residual"].astype(np.float64)[np.ix_(mi, ni)]
        if defect == "residual_after_write":              # the residual element is read after another lane wrote the output over it
            assert in_place
            r = (v + r).astype(np.float16).astype(np.float64)
        v = v + r
    return (v + 0.0).astype(np.float16)                    # (+ 0.0: an exact zero is +0)


# defect -> (formats, kinds, magnitudes) it can be expressed in
DEFECTS = {
    "nibble0_as_plus8": (("int4",), ("int",), ("plain", "epi")),
    "nibble_not_offset": (("int4",), ("int",), ("plain", "epi")),
    "int8_m128_clamped": (("int8",), ("int",), ("plain", "epi")),
    "neighbour_group_scale": (("int4",), ("int",), ("plain", "epi")),
    "neighbour_row_scale": (("int8", "int4", "fp8"), ("int", "probe"), ("plain", "epi")),
    "neighbour_token_scale": (("fp8",), ("int", "probe"), ("plain", "epi")),
    "k_tail_dropped": (("f16", "int8", "int4", "fp8"), ("int", "probe"), ("plain", "epi")),
    "partial128_fp16": (("f16", "int8", "int4", "fp8"), ("int",), ("plain",)),     # a partial of at most 2048 units has nothing to round
    "slab_fp16": (("f16", "int8", "int4", "fp8"), ("int",), ("plain",)),
    "e4m3_subnormal_flushed": (("fp8",), ("probe",), ("plain",)),
    "e4m3_neg_zero_as_nan": (("fp8",), ("probe",), ("plain",)),
    "e4m3_448_as_240": (("fp8",), ("int", "probe"), ("plain", "epi")),
    "wrong_slice_scale": (("fp8",), ("runs",), ("plain",)),                        # needs K slices of different amax
    "residual_after_write": (("f16", "int8", "int4", "fp8"), ("int",), ("epi",)),
}


def _expressible(defect, case, epi):
    fmts, kinds, mags = DEFECTS[defect]
    kind = "runs" if case.get("runs") else case["kind"]
    if defect == "wrong_slice_scale":
        return kind == "runs"
    return case["fmt"] in fmts and (kind in kinds or (kind == "runs" and "int" in kinds)) and epi in mags


def _subset(case):
    """rows and weight rows a defect is judged on (outputs are independent: a bit that changes here changes in the case): the first and
    last rows (the all-positive, zero and outlier rows are last), the first 256 weight rows (every e4m3 code of a probe) and the last 16"""
    M, N = case["M"], case["N"]
    mi = np.arange(M) if M <= 24 else np.r_[0:12, M - 12:M]
    ni = np.arange(N) if N <= 272 else np.r_[0:256, N - 16:N]
    return mi, ni


@pytest.mark.parametrize("case", ALL, ids=[c["id"] for c in ALL])
def test_conditions_hold_and_every_seeded_defect_shows(case):
    for epi in E.epilogues(case):
        b = E.build(case, epi)                            # asserts the conditions
        mi, ni = _subset(case)
        exp = b["expected"][np.ix_(mi, ni)].view(np.uint16)
        sl = 4 if case.get("runs") else 1
        # the restatement itself, without a defect, is the exact answer (with and without a K split)
        assert np.array_equal(project(b, None, mi, ni, slices=sl).view(np.uint16), exp)
        for defect in DEFECTS:
            if _expressible(defect, case, epi):
                with np.errstate(all="ignore"):           # a defect may overflow fp16 or produce NaN: that is a changed bit
                    got = project(b, defect, mi, ni, in_place=True, slices=sl).view(np.uint16)
                assert (got != exp).any(), "%s %s: %s changes no output bit" % (case["id"], epi, defect)


# ---------------------------------------------------------------- what the earlier recipe sees of the same defects
def _gaussian(fmt, rng, M=16, K=4096, N=256):
    x = rng.standard_normal((M, K)).astype(np.float16)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float16).astype(np.float32)
    case = dict(id="gauss_" + fmt, fmt=fmt, K=K, group=128 if fmt == "int4" else 0, kind="int")
    res = rng.standard_normal((M, N)).astype(np.float16)
    if fmt == "f16":
        return dict(case=case, x=x, w=w.astype(np.float16), scale=None, bias=None, residual=res)
    if fmt == "int8":
        s = (np.abs(w).max(axis=1) / np.float32(127.0)).astype(np.float16)
        q = np.clip(np.rint(w / s.astype(np.float32)[:, None]), -127, 127).astype(np.int8)
        return dict(case=case, x=x, w=q, scale=s, bias=None, residual=res)
    if fmt == "int4":
        wg = w.reshape(N, K // 128, 128)
        s = (np.abs(wg).max(axis=2) / np.float32(7.0)).astype(np.float16)
        q = np.clip(np.rint(wg / s.astype(np.float32)[:, :, None]), -8, 7).astype(np.int32).reshape(N, K) + 8
        return dict(case=case, x=x, w=E._pack4(q.astype(np.uint8)), scale=s, bias=None, residual=res)
    s = (np.abs(w).max(axis=1) / np.float32(448.0)).astype(np.float32)
    v = _to_e4m3(w.astype(np.float64) / s[:, None])
    code_of = {float(E.E4M3[c]): c for c in range(0x7F)}
    q = np.vectorize(lambda t: code_of[abs(t)] | (0x80 if t < 0 else 0), otypes=[np.uint8])(v)
    return dict(case=case, x=x, w=q, scale=s, bias=None, residual=res)


def recipe_verdicts():
    """{(defect, format): True where the defect passes the Gaussian recipe}"""
    out = {}
    for fmt in ("f16", "int8", "int4", "fp8"):
        b = _gaussian(fmt, np.random.default_rng(7))
        for defect, (fmts, _, _) in DEFECTS.items():
            if fmt not in fmts:
                continue
            sl = 4 if defect in ("wrong_slice_scale", "slab_fp16") else 1     # (the reference is split like the defective launch)
            ref = project(b, None, slices=sl).astype(np.float64)
            with np.errstate(all="ignore"):
                got = project(b, defect, in_place=True, slices=sl).astype(np.float64)
                err = np.abs(got - ref)
            if fmt == "fp8":    # test_linear_packed_fp8_matches_e4m3_emulation's bound
                ok = (err <= 3e-3 + 3e-3 * np.abs(ref)).mean() > 0.9 and \
                    (np.linalg.norm(err, axis=1) / np.linalg.norm(ref, axis=1)).max() < 1e-2
            else:
                ok = bool((err <= 2e-3 + 2e-3 * np.abs(ref)).all())
            out[(defect, fmt)] = bool(ok)
    return out


def test_defects_the_gaussian_recipe_lets_through(capsys):
    v = recipe_verdicts()
    with capsys.disabled():
        print("\nseeded defects under the Gaussian recipe (2e-3 + 2e-3 |y|; fp8: the packed test's statistical bound):")
        for (defect, fmt), ok in sorted(v.items()):
            print("  %-24s %-5s %s" % (defect, fmt, "PASSES (not seen)" if ok else "caught"))
    assert len(v) >= len(DEFECTS)     # every defect was judged in at least one format; the verdicts themselves are recorded, not asserted
