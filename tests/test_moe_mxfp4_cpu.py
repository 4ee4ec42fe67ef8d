"""Host side of the _ex mixture-of-experts entries and of tests/moe_mxfp4_cases.py (no GPU): every condition the cases claim, the
mutants a wrong kernel would compute held at least 10 bounds away from the reference, the plan line, and every host refusal of
llmie_moe_ffn_ex / llmie_moe_route_ex / llmie_moe_ffn_plan_ex with its code (refused before anything is dereferenced)."""
import ctypes as C
import os

import numpy as np
import pytest

import moe_cases as mc
import moe_mxfp4_cases as mq
import mxfp4_cases as mx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
FAKE = 4096   # an aligned non-NULL "device pointer": every call below is refused before anything is dereferenced
W_F16, W_INT8, W_MXFP4 = 0, 1, 5

_built = {}


def built(case):
    if case["id"] not in _built:
        b = mq.build(case)
        _built[case["id"]] = (b, mq.reference(b))
    return _built[case["id"]]


@pytest.fixture(scope="module")
def lib(llmie):
    llmie.build()
    return llmie.lib()


# ---------------------------------------------------------------- the cases
def test_case_list_covers_the_stated_shapes():
    assert [c["base"]["id"] for c in mq.CASES] == [c["id"] for c in mc.CASES]
    assert sorted({c["rows"] for c in mq.CASES}) == [1, 2, 4, 5, 16, 17, 33, 100, 300]
    assert {2112, 4160, 8256} <= {c["H"] for c in mq.CASES} and {2112, 4160, 8256} <= {c["Ie"] for c in mq.CASES}
    assert max(c["E"] for c in mq.CASES) == 128
    assert [c["id"] for c in mq.END_CASES] == ["lo", "hi"] and all(c["k"] == 1 and not c["base"]["resid"] for c in mq.END_CASES)
    assert sorted({c["base"]["id"] for c in mq.EPI_CASES}) == sorted(mq.EPI_IDS) and len(mq.EPI_CASES) == 2 * len(mq.EPI_IDS)
    assert len({c["id"] for c in mq.ALL_CASES}) == len(mq.ALL_CASES)


@pytest.mark.parametrize("case", mq.CASES + mq.END_CASES, ids=[c["id"] for c in mq.CASES + mq.END_CASES])
def test_scale_bytes_and_layout(case):
    b, ref = built(case)
    E, H, Ie = case["E"], case["H"], case["Ie"]
    assert b["gate_up_q"].shape == (E, 2 * Ie, H // 2) and b["gate_up_s"].shape == (E, 2 * Ie, H // 32)
    assert b["down_q"].shape == (E, H, Ie // 2) and b["down_s"].shape == (E, H, Ie // 32)
    for s in (b["gate_up_s"], b["down_s"]):
        assert s.dtype == np.uint8 and 104 <= int(s.min()) and int(s.max()) <= 140, (int(s.min()), int(s.max()))
    if case["end"] == "lo":
        assert 104 <= int(b["down_s"].min()) and int(b["down_s"].max()) == 107 and len(np.unique(b["down_s"])) == 4
    if case["end"] == "hi":
        assert int(b["down_s"].min()) == 137 and int(b["down_s"].max()) == 140 and np.abs(ref["y64"]).max() < 3e4
    if case["end"] is None:
        # the codes are what the library's quantiser makes of the fp16 matrices (layout of the flattened matrices), blocks differ
        q, s = mx.quantize(b["down16"].reshape(E * H, Ie))
        assert np.array_equal(q.reshape(b["down_q"].shape), b["down_q"]) and np.array_equal(s.reshape(b["down_s"].shape), b["down_s"])
        if H >= 256:
            assert len(np.unique(b["gate_up_s"])) >= 4
    assert np.isfinite(ref["y64"]).all() and np.abs(ref["y64"]).max() > 0 and np.abs(ref["y16"]).max() < 65504
    assert ref["bounds"]["max_abs"] > 0 and ref["bounds"]["rel"] > 0


@pytest.mark.parametrize("case", mq.EPI_CASES, ids=[c["id"] for c in mq.EPI_CASES])
def test_epilogue_cases_exercise_the_epilogue(case):
    b, ref = built(case)
    assert 0.10 <= ref["clamp_share"] <= 0.90, ref["clamp_share"]
    for n in ("router_bias", "gate_up_bias", "down_bias"):
        assert b[n] is not None and b[n].dtype == np.float16 and (b[n] != 0).any()
    # the biased logits are exact in fp32: integers of the unit, below 2^24 of it
    q = ref["logits"] / b["logit_unit"]
    assert np.array_equal(q, np.round(q)) and np.abs(q).max() < 2 ** 24
    assert np.array_equal(ref["logits"].astype(np.float32).astype(np.float64), ref["logits"])
    for m in mq.EPI_MUTANTS:
        y = mq.ffn(b, ref["experts"], ref["weights"], rounded=False, mutant=m)
        dist = mq.distance_in_bounds(y, ref)
        print("%s %s: %.0f bounds" % (case["id"], m, dist))
        assert dist >= 10, (case["id"], m, dist)


def test_router_bias_changes_a_selection():
    changed = 0
    for case in mq.EPI_CASES:
        b, ref = built(case)
        plain = mc.route(b["x"], b["router"], case["k"], case["flags"])[0]
        changed += int((plain != ref["experts"]).any(axis=1).sum())
    assert changed > 0


@pytest.mark.parametrize("cid", mq.MUTANT_IDS)
def test_quantisation_mutants_leave_the_bounds(cid):
    case = mq.BY_ID[cid + "_mxfp4"]
    b, ref = built(case)
    for name, (gu, dn) in mq.weight_mutants(b).items():
        y = mq.ffn(b, ref["experts"], ref["weights"], rounded=False, gate_up=gu, down=dn)
        dist = mq.distance_in_bounds(y, ref)
        print("%s %s: %.0f bounds" % (cid, name, dist))
        assert dist >= 10, (cid, name, dist)


def test_f16_case_without_epilogue_is_the_moe_cases_reference():
    """the restatement here, on fp16 experts without biases under the plain act, is moe_cases.ffn"""
    base = mc.BY_ID["r4_e8"]
    b = mq.build(mq._case(base, "f16"))
    r0 = mc.reference(mc.build(base))
    r1 = mq.reference(b)
    assert np.array_equal(r0["experts"], r1["experts"]) and np.array_equal(r0["y64"], r1["y64"]) and np.array_equal(r0["y16"], r1["y16"])


# ---------------------------------------------------------------- the entries, host side
class Desc(C.Structure):
    _fields_ = [("format", C.c_int), ("router", C.c_void_p), ("router_bias", C.c_void_p), ("gate_up", C.c_void_p), ("gate_up_scale", C.c_void_p),
                ("gate_up_bias", C.c_void_p), ("down", C.c_void_p), ("down_scale", C.c_void_p), ("down_bias", C.c_void_p), ("act", C.c_int),
                ("alpha", C.c_float), ("limit", C.c_float)]


def desc(fmt=W_MXFP4, **kw):
    d = Desc(format=fmt, router=FAKE, gate_up=FAKE, down=FAKE)
    if fmt == W_MXFP4:
        d.gate_up_scale, d.down_scale = FAKE + 1, FAKE + 3   # scale bytes need no alignment
    for n, v in kw.items():
        setattr(d, n, v)
    return d


def ffn_ex(lib, d, rows=4, H=256, Ie=192, E=8, k=2, flags=0, x=FAKE, y=FAKE, resid=None, ws=FAKE, ws_bytes=1 << 30, dtype=1):
    return lib.llmie_moe_ffn_ex(x, C.byref(d) if d is not None else None, resid, y, rows, H, Ie, E, k, flags, ws, ws_bytes, dtype, None)


def test_exports_and_python_surface(lib, llmie):
    vp, i, sz, u = C.c_void_p, C.c_int, C.c_size_t, C.c_uint
    want = {
        "llmie_moe_ffn_plan_ex": [i, i, i, i, i, u, i, i],
        "llmie_moe_route_ex": [vp, vp, i, i, i, i, u, vp, vp, i, vp],
        "llmie_moe_ffn_ex": [vp, vp, vp, vp, i, i, i, i, i, u, vp, sz, i, vp],
        "llmie_decoder_moe_attach_ex": [vp, vp, i, i, i, u, vp, sz],
    }
    for name, args in want.items():
        assert name in llmie.EXPORTS and getattr(lib, name).argtypes == args, name
    assert lib.llmie_moe_ffn_plan_ex.restype is C.c_char_p
    assert C.sizeof(llmie.MoeExpertsDesc) == C.sizeof(Desc) and [f[0] for f in llmie.MoeExpertsDesc._fields_] == [f[0] for f in Desc._fields_]
    assert (llmie.MOE_ACT_SWIGLU, llmie.MOE_ACT_SWIGLU_CLAMPED) == (0, 1)
    hdr = open(os.path.join(ROOT, "include", "llmie.h")).read()
    assert "LLMIE_MOE_ACT_SWIGLU = 0, LLMIE_MOE_ACT_SWIGLU_CLAMPED = 1" in hdr
    for fn in ("MoeExperts", "moe_route_ex", "moe_ffn_ex", "moe_ffn_plan_ex"):
        assert callable(getattr(llmie, fn))


def test_plan_ex_is_the_plan_line_with_format_and_act(lib):
    """fp16: the line of llmie_moe_ffn_plan; MXFP4: the gemv route up to 16 rows, so there the line of the forced GEMV plan"""
    for (rows, H, Ie, E, k) in ((1, 2880, 2880, 32, 4), (4, 256, 192, 8, 2), (5, 256, 192, 8, 2), (16, 256, 192, 8, 2), (17, 256, 192, 8, 2),
                                (300, 64, 192, 8, 2), (128, 4096, 14336, 8, 2)):
        for flags in (0, 4):
            for fmt, fname in ((W_F16, "f16"), (W_MXFP4, "mxfp4")):
                gemv = fmt == W_MXFP4 and flags == 0 and rows <= mq.GEMV_DEFAULT_ROWS_MXFP4
                plain = lib.llmie_moe_ffn_plan(rows, H, Ie, E, k, 2 if gemv else flags).decode()
                for act, aname in ((0, "swiglu"), (1, "swiglu_clamped")):
                    assert lib.llmie_moe_ffn_plan_ex(rows, H, Ie, E, k, flags, fmt, act).decode() == "%s format=%s act=%s" % (plain, fname, aname)
    for case in mq.ALL_CASES:
        line = lib.llmie_moe_ffn_plan_ex(case["rows"], case["H"], case["Ie"], case["E"], case["k"], 0, W_MXFP4 if case["fmt"] == "mxfp4" else W_F16, 0).decode()
        f = dict(w.split("=") for w in line.split())
        assert (f["route"], int(f["rt"]), int(f["tiles"])) == mq.expected_plan(case), case["id"]
    assert lib.llmie_moe_ffn_plan_ex(4, 256, 192, 8, 2, 0, W_INT8, 0) is None and b"format" in lib.llmie_last_error()
    assert lib.llmie_moe_ffn_plan_ex(4, 256, 192, 8, 2, 0, W_MXFP4, 2) is None and b"act" in lib.llmie_last_error()
    assert lib.llmie_moe_ffn_plan_ex(4, 250, 192, 8, 2, 0, W_MXFP4, 0) is None
    assert lib.llmie_moe_ffn_plan_ex(17, 256, 192, 8, 2, 2, W_MXFP4, 0) is None   # LLMIE_MOE_FORCE_GEMV above 16 rows


def test_ffn_ex_refusals(lib):
    inf, nan = float("inf"), float("nan")
    cases = [
        ("NULL descriptor", None, {}, INVALID),
        ("int8 experts", desc(W_INT8), {}, UNSUPPORTED),
        ("NULL gate_up scale with MXFP4", desc(gate_up_scale=None), {}, INVALID),
        ("NULL down scale with MXFP4", desc(down_scale=None), {}, INVALID),
        ("a scale with fp16 experts", desc(W_F16, gate_up_scale=FAKE), {}, INVALID),
        ("a down scale with fp16 experts", desc(W_F16, down_scale=FAKE), {}, INVALID),
        ("NULL router", desc(router=None), {}, INVALID),
        ("NULL codes", desc(down=None), {}, INVALID),
        ("codes off 16 bytes", desc(gate_up=FAKE + 8), {}, UNSUPPORTED),
        ("down codes off 16 bytes", desc(down=FAKE + 4), {}, UNSUPPORTED),
        ("router off 16 bytes", desc(router=FAKE + 2), {}, UNSUPPORTED),
        ("router bias off 2 bytes", desc(router_bias=FAKE + 1), {}, UNSUPPORTED),
        ("gate/up bias off 2 bytes", desc(gate_up_bias=FAKE + 1), {}, UNSUPPORTED),
        ("down bias off 2 bytes", desc(W_F16, down_bias=FAKE + 3), {}, UNSUPPORTED),
        ("unknown act", desc(act=2), {}, INVALID),
        ("limit 0", desc(act=1, alpha=1.702, limit=0.0), {}, INVALID),
        ("limit < 0", desc(act=1, alpha=1.702, limit=-1.0), {}, INVALID),
        ("limit inf", desc(act=1, alpha=1.702, limit=inf), {}, INVALID),
        ("limit nan", desc(act=1, alpha=1.702, limit=nan), {}, INVALID),
        ("alpha inf", desc(act=1, alpha=inf, limit=7.0), {}, INVALID),
        ("alpha nan", desc(W_F16, act=1, alpha=nan, limit=7.0), {}, INVALID),
        ("NULL x", desc(), dict(x=None), INVALID),
        ("x off 16 bytes", desc(), dict(x=FAKE + 2), UNSUPPORTED),
        ("hidden % 64", desc(), dict(H=96), UNSUPPORTED),
        ("fp32", desc(), dict(dtype=0), UNSUPPORTED),
        ("force gemv above 16 rows", desc(), dict(rows=17, flags=2), UNSUPPORTED),
        ("NULL workspace", desc(), dict(ws=None), WORKSPACE),
        ("short workspace", desc(), dict(ws_bytes=1024), WORKSPACE),
        ("short workspace, fp16 with a bias", desc(W_F16, down_bias=FAKE + 2), dict(ws_bytes=1024), WORKSPACE),
    ]
    for what, d, kw, code in cases:
        assert ffn_ex(lib, d, **kw) == code, what
        assert b"moe_ffn_ex" in lib.llmie_last_error(), what
    # bias pointers that are 2-byte aligned only and scale bytes without alignment pass every check up to the workspace
    ok = desc(act=1, alpha=1.702, limit=7.0, router_bias=FAKE + 2, gate_up_bias=FAKE + 6, down_bias=FAKE + 10)
    assert ffn_ex(lib, ok, ws_bytes=1024) == WORKSPACE


def test_route_ex_refusals(lib):
    def call(d, x=FAKE, rows=4, H=256, E=8, k=2, flags=0, dtype=1, out=FAKE):
        return lib.llmie_moe_route_ex(x, C.byref(d) if d is not None else None, rows, H, E, k, flags, out, out, dtype, None)
    assert call(None) == INVALID
    assert call(desc(router=None)) == INVALID
    assert call(desc(), out=None) == INVALID
    assert call(desc(router=FAKE + 8)) == UNSUPPORTED
    assert call(desc(router_bias=FAKE + 1)) == UNSUPPORTED and b"router_bias" in lib.llmie_last_error()
    assert call(desc(), k=9) == UNSUPPORTED
    assert call(desc(), dtype=0) == UNSUPPORTED
    assert call(desc(), flags=1 << 9) == INVALID


def test_workspace_query_covers_both_formats(lib):
    """the MXFP4 routes carve the workspace as the fp16 ones do: the ws= of the _ex plan line never exceeds llmie_moe_workspace_bytes"""
    for (rows, H, Ie, E, k) in ((1, 64, 64, 1, 1), (4, 256, 192, 8, 2), (17, 256, 192, 128, 8), (300, 64, 192, 8, 2), (128, 2880, 2880, 32, 4)):
        total = lib.llmie_moe_workspace_bytes(rows, H, Ie, E, k)
        for r in range(1, rows + 1, max(1, rows // 7)):
            for flags in (0, 4, 4 | 8, 4 | 16):
                line = lib.llmie_moe_ffn_plan_ex(r, H, Ie, E, k, flags, W_MXFP4, 1).decode()
                assert int(dict(w.split("=") for w in line.split())["ws"]) <= total


def test_moe_kernels_use_no_scratch(lib):
    """every kernel of csrc/moe.hip, the MXFP4 instantiations included, runs from registers: no scratch, no spills (read from the built
    code object, no GPU needed)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("ckr", os.path.join(ROOT, "tools", "check_kernel_resources.py"))
    ckr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ckr)
    ks = [k for k in ckr.kernel_metadata(os.path.join(ROOT, "llm-inference-engine_amd", "csrc", "_obj", "moe.hip.o")) if "moe_" in k["name"]]
    mx4 = [k for k in ks if "moe_mx4_" in k["name"]]
    assert len(mx4) == 12 and len(ks) >= 37, [k["name"] for k in ks]
    bad = [k for k in ks if k["scratch"] or k["vgpr_spill"] or k["sgpr_spill"]]
    assert not bad, bad
