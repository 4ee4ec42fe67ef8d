"""Host side of the mixture-of-experts entries and of their test cases (no GPU): exports and signatures; the float64 restatement of
tests/moe_cases.py pinned to the oracle's dense functions by the concatenation identity; every condition the cases claim; every
host refusal with its code and message; llmie_moe_ffn_plan against the stated thresholds and the tile bound; the workspace query."""
import ctypes as C
import os

import numpy as np
import pytest

import moe_cases as mc
import moe_engine_ref as er
import oracle as orc
from conftest import systematic_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
FAKE = 4096   # an aligned non-NULL "device pointer": every call below is refused before anything is dereferenced
FORCE_GEMV, FORCE_GROUPED = 2, 4

ROWS = (1, 2, 4, 5, 16, 17, 33, 100, 300)
HS = (64, 256, 2112)
IES = (64, 192, 2112)
EK = ((1, 1), (4, 1), (8, 2), (128, 8))


@pytest.fixture(scope="module")
def lib(llmie):
    llmie.build()
    return llmie.lib()


def _err(lib):
    return lib.llmie_last_error().decode()


def _fields(text):
    return dict(w.split("=") for w in text.split())


def test_exports_signatures_and_constants(lib, llmie):
    vp, i, sz, u = C.c_void_p, C.c_int, C.c_size_t, C.c_uint
    want = {
        "llmie_moe_workspace_bytes": [i, i, i, i, i],
        "llmie_moe_ffn_plan": [i, i, i, i, i, u],
        "llmie_moe_route": [vp, vp, i, i, i, i, u, vp, vp, i, vp],
        "llmie_moe_ffn": [vp, vp, vp, vp, vp, vp, i, i, i, i, i, u, vp, sz, i, vp],
    }
    for name, args in want.items():
        assert name in llmie.EXPORTS
        assert getattr(lib, name).argtypes == args, name
    assert lib.llmie_moe_workspace_bytes.restype is sz and lib.llmie_moe_ffn_plan.restype is C.c_char_p
    hdr = open(os.path.join(ROOT, "include", "llmie.h")).read()
    for name, v in (("MAX_EXPERTS", "128"), ("MAX_TOP_K", "8"), ("SOFTMAX_ALL", "1u"), ("FORCE_GEMV", "2u"), ("FORCE_GROUPED", "4u")):
        assert "#define LLMIE_MOE_%s %s" % (name, v) in hdr
    assert (llmie.MOE_MAX_EXPERTS, llmie.MOE_MAX_TOP_K) == (128, 8)
    assert (llmie.MOE_SOFTMAX_ALL, llmie.MOE_FORCE_GEMV, llmie.MOE_FORCE_GROUPED) == (mc.SOFTMAX_ALL, FORCE_GEMV, FORCE_GROUPED)
    assert "#define LLMIE_ABI_VERSION 3" in hdr and lib.llmie_abi_version() == 3
    for fn in ("moe_workspace", "moe_route", "moe_ffn", "moe_ffn_plan"):
        assert callable(getattr(llmie, fn))


# ---- the restatement against the oracle's dense functions ----
@pytest.mark.parametrize("cid", ["r1_e1", "r4_e8", "r17_e128", "r33_e128_all", "r100_counts"])
def test_restatement_equals_a_dense_ffn_of_the_selected_experts(cid):
    """a row's MoE FFN with its routing fixed = a dense FFN of inter size k * Ie: the selected gate rows stacked, then the selected up
    rows, and the down columns of expert e_j scaled by w_j.  oracle.linear / oracle.silu_and_mul compute in fp32: 1e-4 relative, the
    project's bar for fp32 kernels."""
    b = mc.build(mc.BY_ID[cid])
    ref = mc.reference(b)
    Ie, k = b["case"]["Ie"], b["case"]["k"]
    for m in sorted(set([0, b["case"]["rows"] // 2, b["case"]["rows"] - 1])):
        es, ws = ref["experts"][m], ref["weights"][m]
        gate = np.concatenate([b["gate_up"][e, :Ie] for e in es]).astype(np.float32)
        up = np.concatenate([b["gate_up"][e, Ie:] for e in es]).astype(np.float32)
        dn = np.concatenate([b["down"][e].astype(np.float64) * w for e, w in zip(es, ws)], axis=1).astype(np.float32)
        x = b["x"][m:m + 1].astype(np.float32)
        t = orc.linear(x, np.concatenate([gate, up]))
        a = orc.silu_and_mul(t.reshape(1, 2, k * Ie))
        y = orc.linear(a, dn)[0].astype(np.float64)
        if b["resid"] is not None:
            y = y + b["resid"][m].astype(np.float64)
        want = ref["y64"][m]
        assert np.abs(y - want).max() <= 1e-4 * max(1.0, np.abs(want).max()), (cid, m)
    if b["case"]["E"] == 1:   # the plain dense FFN: weight 1 exactly
        assert np.array_equal(ref["weights"], np.ones_like(ref["weights"])) and (ref["experts"] == 0).all()


def test_route_restatement_on_hand_made_logits():
    r = np.array([[1.0, 3.0, 3.0, -2.0, np.nan, 3.0], [np.nan] * 6, [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    ids, w, _ = mc.route(None, None, 3, r=r)
    assert ids.tolist() == [[1, 2, 5], [0, 1, 2], [0, 1, 2]]
    assert np.allclose(w[0], 1 / 3) and np.allclose(w[2], 1 / 3)
    ids, w, _ = mc.route(None, None, 2, r=r[:1])
    assert ids.tolist() == [[1, 2]] and np.allclose(w, 0.5)
    ids, w, _ = mc.route(None, None, 2, flags=mc.SOFTMAX_ALL, r=np.array([[0.0, np.log(2.0), np.log(5.0)]]))
    assert ids.tolist() == [[2, 1]] and np.allclose(w, [[5 / 8, 2 / 8]])


# ---- what the cases claim ----
def test_case_list_covers_the_size_lists():
    assert {c["rows"] for c in mc.CASES} == set(ROWS)
    assert {c["H"] for c in mc.CASES} >= set(HS) and {c["Ie"] for c in mc.CASES} >= set(IES)
    assert {(c["E"], c["k"]) for c in mc.CASES} == set(EK)
    for c in mc.CASES:
        assert c["H"] % 64 == 0 and c["Ie"] % 64 == 0
        assert c["Ie"] < 2112 or c["H"] <= 64      # 2112 and above only beside a small other dimension
        assert c["H"] < 2112 or c["Ie"] <= 64
    # both routes and both tile heights are reached by default, and forced GEMV has cases up to 16 rows
    plans = {mc.expected_plan(c["rows"], c["H"], c["Ie"], c["E"], c["k"])[:2] for c in mc.CASES}
    assert plans == {("gemv", 0), ("grouped", 1), ("grouped", 4)}
    assert max(c["rows"] for c in mc.CASES if c["rows"] <= mc.GEMV_MAX_ROWS) == 16


@pytest.mark.parametrize("case", mc.CASES, ids=[c["id"] for c in mc.CASES])
def test_case_conditions(case):
    b = mc.build(case)
    E, k, rows = case["E"], case["k"], case["rows"]
    ids, w, r = mc.route(b["x"], b["router"], k, case["flags"])
    # exact logits: every logit is a multiple of the row's unit, far below 2^24 of it, and the fp32 matmul reproduces it
    r32 = b["x"].astype(np.float32) @ b["router"].astype(np.float32).T
    assert np.array_equal(r32.astype(np.float64), r)
    assert ids.min() >= 0 and ids.max() < E and all(len(set(row)) == k for row in ids.tolist())
    if case["flags"] & mc.SOFTMAX_ALL:
        assert (w.sum(axis=1) <= 1 + 1e-12).all() and (E == k or (w.sum(axis=1) < 1).any())
    else:
        assert np.allclose(w.sum(axis=1), 1.0, atol=1e-12)
    assert (np.diff(w, axis=1) <= 0).all()   # rank order: non-increasing weights
    inside, across = mc.tie_census(r, k)
    counts = mc.pair_counts(ids, E)
    if case["kind"] == "ties" and rows >= 16 and E >= 4:
        assert across >= 1, "no exact tie across the k-th place"
        if k > 1:
            assert inside >= 1, "no exact tie inside the selected set"
        # a tie is resolved towards the lower id: ranks of equal logit are in ascending id order
        sel = np.take_along_axis(r, ids.astype(np.int64), 1)
        eq = sel[:, :-1] == sel[:, 1:]
        assert (ids[:, :-1][eq] < ids[:, 1:][eq]).all()
    if case["kind"] == "designed":
        assert np.array_equal(ids, mc.designed_assignment(case).astype(np.int32))
        assert inside == 0 and across == 0
    if case["dist"] == "counts":
        assert counts[0] == 0 and counts[1] == 16 and counts[2] == 17 and counts[3] == 16 * 4 + 1 and counts.sum() == rows * k
        ranks = [set(np.nonzero(ids == e)[1].tolist()) for e in (1, 2, 3)]
        assert all(rk == {0, 1} for rk in ranks)   # (row, rank) order inside an expert mixes the ranks
    if case["dist"] == "one":
        assert counts.max() == rows * k and (counts > 0).sum() == 1
    ref = mc.reference(b)
    assert ref["bounds"]["max_abs"] > 0 and 1e-5 < ref["bounds"]["rel"] < 4e-3   # two fp16 roundings: a few 2^-11
    # a dropped or doubled expert weight is far outside the bounds
    for scale in (0.0, 2.0):
        w2 = ref["weights"].copy()
        w2[:, -1] *= scale
        bad = mc.ffn(b, ref["experts"], w2, rounded=True)
        assert mc.rel_frobenius(bad, ref["y64"]) > 10 * ref["bounds"]["rel"]


# ---- host refusals: nothing is launched, no device is needed ----
def _ffn(lib, **kw):
    a = dict(x=FAKE, router=FAKE, gate_up=FAKE, down=FAKE, resid=None, y=FAKE, rows=5, H=256, Ie=192, E=8, k=2, flags=0, ws=FAKE * 16,
             ws_bytes=1 << 40, dtype=1)
    a.update(kw)
    return lib.llmie_moe_ffn(a["x"], a["router"], a["gate_up"], a["down"], a["resid"], a["y"], a["rows"], a["H"], a["Ie"], a["E"], a["k"],
                             a["flags"], a["ws"], a["ws_bytes"], a["dtype"], None)


FFN_REFUSALS = [
    (dict(x=None), INVALID, "NULL pointer"), (dict(router=None), INVALID, "NULL pointer"), (dict(gate_up=None), INVALID, "NULL pointer"),
    (dict(down=None), INVALID, "NULL pointer"), (dict(y=None), INVALID, "NULL pointer"),
    (dict(rows=0), INVALID, "non-positive size"), (dict(H=0), INVALID, "non-positive size"), (dict(Ie=-64), INVALID, "non-positive size"),
    (dict(E=0), INVALID, "non-positive size"), (dict(k=0), INVALID, "non-positive size"),
    (dict(flags=FORCE_GEMV | FORCE_GROUPED), INVALID, "together"), (dict(flags=64), INVALID, "unknown flags"),
    (dict(E=129), UNSUPPORTED, "129 experts above LLMIE_MOE_MAX_EXPERTS (128)"),
    (dict(E=4, k=5), UNSUPPORTED, "top_k=5 above the 4 experts"),
    (dict(E=16, k=9), UNSUPPORTED, "top_k=9 above LLMIE_MOE_MAX_TOP_K (8)"),
    (dict(H=96), UNSUPPORTED, "hidden=96 is not a multiple of 64"),
    (dict(Ie=200), UNSUPPORTED, "inter=200 is not a multiple of 64"),
    (dict(dtype=0), UNSUPPORTED, "fp16 activations only"),
    (dict(x=FAKE + 8), UNSUPPORTED, "not 16-byte aligned"), (dict(down=FAKE + 2), UNSUPPORTED, "not 16-byte aligned"),
    (dict(resid=FAKE + 4), UNSUPPORTED, "not 16-byte aligned"),
    (dict(rows=17, flags=FORCE_GEMV), UNSUPPORTED, "LLMIE_MOE_FORCE_GEMV with 17 rows"),
    (dict(ws=None), WORKSPACE, "workspace"), (dict(ws=FAKE * 16 + 16), WORKSPACE, "256-byte aligned"),
]


@pytest.mark.parametrize("kw,rc,msg", FFN_REFUSALS)
def test_ffn_refusals(lib, kw, rc, msg):
    assert _ffn(lib, **kw) == rc, kw
    assert _err(lib).startswith("moe_ffn:") and msg in _err(lib), _err(lib)


def test_ffn_workspace_short_by_one_byte(lib):
    for flags in (0, FORCE_GEMV, FORCE_GROUPED):
        need = int(_fields(lib.llmie_moe_ffn_plan(5, 256, 192, 8, 2, flags).decode())["ws"])
        assert _ffn(lib, flags=flags, ws_bytes=need - 1) == WORKSPACE and str(need) in _err(lib)


def test_route_refusals(lib):
    def go(**kw):
        a = dict(x=FAKE, router=FAKE, rows=5, H=256, E=8, k=2, flags=0, eo=FAKE, wo=FAKE, dtype=1)
        a.update(kw)
        return lib.llmie_moe_route(a["x"], a["router"], a["rows"], a["H"], a["E"], a["k"], a["flags"], a["eo"], a["wo"], a["dtype"], None)
    for kw, rc, msg in ((dict(x=None), INVALID, "NULL pointer"), (dict(eo=None), INVALID, "NULL pointer"), (dict(wo=None), INVALID, "NULL pointer"),
                        (dict(rows=-1), INVALID, "non-positive size"), (dict(E=129), UNSUPPORTED, "LLMIE_MOE_MAX_EXPERTS"),
                        (dict(k=9, E=16), UNSUPPORTED, "LLMIE_MOE_MAX_TOP_K"), (dict(k=3, E=2), UNSUPPORTED, "above the 2 experts"),
                        (dict(H=96), UNSUPPORTED, "multiple of 64"), (dict(dtype=0), UNSUPPORTED, "fp16 activations only"),
                        (dict(router=FAKE + 8), UNSUPPORTED, "not 16-byte aligned")):
        assert go(**kw) == rc, kw
        assert _err(lib).startswith("moe_route:") and msg in _err(lib), _err(lib)


def test_plan_query_refusals(lib):
    for args, msg in (((5, 256, 192, 129, 2, 0), "LLMIE_MOE_MAX_EXPERTS"), ((5, 96, 192, 8, 2, 0), "hidden=96"), ((0, 256, 192, 8, 2, 0), "non-positive"),
                      ((17, 256, 192, 8, 2, FORCE_GEMV), "FORCE_GEMV with 17 rows"), ((5, 256, 192, 8, 2, 6), "together")):
        assert lib.llmie_moe_ffn_plan(*args) is None
        assert _err(lib).startswith("moe_ffn_plan:") and msg in _err(lib), _err(lib)
    for args in ((0, 256, 192, 8, 2), (5, 96, 192, 8, 2), (5, 256, 100, 8, 2), (5, 256, 192, 129, 2), (5, 256, 192, 8, 9), (5, 256, 192, 2, 3)):
        assert lib.llmie_moe_workspace_bytes(*args) == 0


# ---- the planner ----
def test_plan_follows_the_thresholds_and_the_tile_bound(lib):
    seen = set()
    for rows in ROWS:
        for H in HS:
            for Ie in IES:
                for E, k in EK:
                    for flags, force in ((0, None), (FORCE_GEMV, "gemv"), (FORCE_GROUPED, "grouped")):
                        text = lib.llmie_moe_ffn_plan(rows, H, Ie, E, k, flags)
                        if force == "gemv" and rows > mc.GEMV_MAX_ROWS:
                            assert text is None and "LLMIE_MOE_FORCE_GEMV" in _err(lib)
                            continue
                        f = _fields(text.decode())
                        route, rt, tiles = mc.expected_plan(rows, H, Ie, E, k, force=force)
                        assert (f["route"], int(f["rt"]), int(f["tiles"])) == (route, rt, tiles), (rows, H, Ie, E, k, flags, f)
                        pairs = rows * k
                        assert int(f["route_grid"]) == (rows + 3) // 4
                        if route == "gemv":
                            assert f["gate_up_grid"] == "%dx%d" % (Ie // 16, pairs) and f["down_grid"] == "%dx%d" % (H // 16, rows)
                            assert f["plan_grid"] == "0" and f["combine_grid"] == "0x0"
                        else:
                            assert tiles == pairs // (16 * rt) + min(E, pairs)
                            assert f["gate_up_grid"] == "%dx%d" % (tiles, Ie // 64) and f["down_grid"] == "%dx%d" % (tiles, H // 64)
                            assert f["plan_grid"] == "1" and f["combine_grid"] == "%dx%d" % (rows, -(-(H // 4) // 256))
                            # the bound holds for every distribution of the pairs over the experts: sum of ceil(n_e / T) over
                            # the non-empty experts <= pairs / T + non-empty experts
                            T = 16 * rt
                            worst = min(E, pairs) - 1 + -(-(pairs - (min(E, pairs) - 1)) // T)   # one pair on all but one expert
                            assert worst <= tiles and -(-pairs // T) <= tiles
                        seen.add((route, rt))
    assert seen == {("gemv", 0), ("grouped", 1), ("grouped", 4)}
    # the thresholds themselves, at their edges
    f = lambda *a: _fields(lib.llmie_moe_ffn_plan(*a).decode())
    assert f(4, 256, 192, 8, 2, 0)["route"] == "gemv" and f(5, 256, 192, 8, 2, 0)["route"] == "grouped"
    assert f(127, 256, 192, 8, 2, 0)["rt"] == "1" and f(128, 256, 192, 8, 2, 0)["rt"] == "4"      # 254 // 8 = 31, 256 // 8 = 32
    assert f(4, 16448, 64, 4, 1, 0)["route"] == "grouped" and f(4, 16384, 64, 4, 1, 0)["route"] == "gemv"
    assert lib.llmie_moe_ffn_plan(4, 16448, 64, 4, 1, FORCE_GEMV) is None and "above 16384" in _err(lib)


def test_workspace_is_monotone_and_covers_every_smaller_call(lib):
    for H, Ie, (E, k) in ((256, 192, (8, 2)), (64, 2112, (128, 8)), (2112, 64, (4, 1)), (64, 64, (1, 1))):
        prev = 0
        sizes = {}
        for rows in range(1, 301):
            n = lib.llmie_moe_workspace_bytes(rows, H, Ie, E, k)
            assert n >= prev > -1 and n % 256 == 0 and n > 0
            prev = sizes[rows] = n
        for max_rows in (1, 4, 5, 16, 17, 127, 128, 300):
            for rows in range(1, max_rows + 1):
                for flags in (0, FORCE_GEMV, FORCE_GROUPED):
                    text = lib.llmie_moe_ffn_plan(rows, H, Ie, E, k, flags)
                    if text is not None:
                        assert int(_fields(text.decode())["ws"]) <= sizes[max_rows], (H, Ie, E, k, max_rows, rows, flags)


@pytest.mark.parametrize("case", er.CASES, ids=[c["id"] for c in er.CASES])
def test_engine_case_reference_meets_the_stability_cap(case):
    """from the reference alone (oracle kernels + the numpy expert FFN, float and fp16-rounded evaluations): at most 10 % of the case's
    rows have an unstable routing, the two evaluations agree within the bar on the stable rows (else the bar could not be asked of a
    device), and an engine that ran dense FFNs instead of its experts would lie at least 10 bars away"""
    b, y16, y64, stable = er.reference(case)
    rows = er.n_rows(case)
    assert y16.shape == (rows, er.H) and np.isfinite(y16).all()
    assert (~stable).sum() <= 0.1 * rows, (case["id"], int((~stable).sum()), rows)
    own = max(systematic_error(y16[m], y64[m])[0] for m in np.nonzero(stable)[0])
    assert own <= 1e-2, (case["id"], own)
    apart = systematic_error(er.dense_twin(b)[stable], y16[stable])[0]
    assert apart >= 10 * 2e-2, (case["id"], apart)


def test_engine_case_list_covers_the_issue():
    ids = {(c["kind"], c["cache"], c["E"], c["k"]) for c in er.CASES}
    for E, k in ((8, 2), (4, 1)):
        assert {("decode", c, E, k) for c in ("dense", "paged", "ragged", "e4m3")} <= ids
        assert {("prefill", c, E, k) for c in ("dense", "paged")} <= ids
        assert {sum(c["lens"]) for c in er.CASES if c["kind"] == "prefill" and c["E"] == E} == {5, 33, 130, 168}
    assert any(c["hist"] and max(c["hist"]) > 128 for c in er.CASES if c["kind"] == "prefill")
    assert any(c["sparse"] == (True, False, True) for c in er.CASES) and any(c["window"] for c in er.CASES)
    assert {len(c["sparse"]) for c in er.CASES} >= {2, 3}


def test_engine_entries_on_the_host(lib, llmie):
    import test_decoder_plan_cpu as dp
    vp, i, sz, u = C.c_void_p, C.c_int, C.c_size_t, C.c_uint
    want = {"llmie_decoder_moe_workspace_bytes": [vp, i, i, i, i], "llmie_decoder_moe_attach": [vp, vp, i, i, i, u, vp, sz],
            "llmie_decoder_moe_detach": [vp]}
    for name, args in want.items():
        assert name in llmie.EXPORTS and getattr(lib, name).argtypes == args, name
    assert lib.llmie_decoder_moe_workspace_bytes.restype is sz
    assert callable(llmie.Decoder.moe_attach) and callable(llmie.Decoder.moe_detach)
    assert [f[0] for f in llmie.MoeLayer._fields_] == ["router", "gate_up", "down"]
    cfg = dp._config(llmie, dp.W_F16, 128, (32, 32, 128, 11008), 8, 0)   # hidden 4096, max_batch 8
    assert lib.llmie_decoder_moe_workspace_bytes(C.byref(cfg), 2048, 14336, 8, 2) == lib.llmie_moe_workspace_bytes(2048, 4096, 14336, 8, 2) > 0
    assert lib.llmie_decoder_moe_workspace_bytes(C.byref(cfg), 3, 14336, 8, 2) == lib.llmie_moe_workspace_bytes(8, 4096, 14336, 8, 2)   # max_batch rows at least
    assert lib.llmie_decoder_moe_workspace_bytes(C.byref(cfg), 0, 14336, 8, 2) == 0
    assert lib.llmie_decoder_moe_workspace_bytes(C.byref(cfg), 8, 14336, 129, 2) == 0
    assert lib.llmie_decoder_moe_attach(None, FAKE, 192, 8, 2, 0, FAKE * 16, 1 << 30) == INVALID
    assert _err(lib).startswith("decoder_moe_attach:") and "NULL pointer" in _err(lib)
    assert lib.llmie_decoder_moe_detach(None) == INVALID and "NULL decoder" in _err(lib)
    # the plan queries answer for an engine without experts: their recordings are reproduced
    import test_prefill_layer_plan_cpu as pl
    assert dp.recording(llmie, lib) == dp._fixture()
    assert pl.recording(llmie, pl.ctypes_plan(lib, lib.llmie_decoder_prefill_layer_plan)) == pl._fixture()
    hdr = open(os.path.join(ROOT, "include", "llmie.h")).read()
    assert "LLMIE_OP_CHAIN, /* ABI 3" in hdr and hdr.count("LLMIE_OP_") >= 13   # LLMIE_OP_COUNT's list is as it was


def test_no_environment_switch():
    assert "getenv" not in open(os.path.join(ROOT, "llm-inference-engine_amd", "csrc", "moe.hip")).read()
