"""The kernel route of every projection call, asserted without a GPU through llmie_linear_route (pure host code).

tests/golden/linear_routes.txt was recorded from the dispatch ladders as they stood before the planner existed (linear_f16_nk and
linear_wq with a dry-run probe at every launch site, returning the site's name instead of launching), over the grid below, together
with the two size queries that have to agree with the routes.  The planner, and everything that reads its plans, must reproduce the
recording exactly: a route that moves, or a size query that drifts from the routes, fails here.

Route names: gemv_ksplit gemv_lds splitk splitk_passes skinny swiglu256 tiles256 tiles256_part tiles128 generic (fp16 weights);
g8p g8p_swiglu int8_splitk_passes int8_splitk int8_skinny int4_splitk int4_chunks gemv_ksplit (int8 / int4), and
image_prefill+<fp16 route> / image_last+<fp16 route> for the fp16 image of quantised weights; "refused" where the call is refused.
"""
import ctypes as C
import os

import pytest

from test_linear_routes_gpu import F16_CASES, WQ_CASES

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linear_routes.txt")

FIXTURE_FP8 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linear_routes_fp8.txt")

W_F16, W_INT8, W_INT4, W_FP8 = 0, 1, 2, 3
FORMATS = [("f16", W_F16, 0), ("int8", W_INT8, 0), ("int4g128", W_INT4, 128), ("int4g64", W_INT4, 64)]
MS = [1, 2, 4, 5, 8, 9, 16, 32, 33, 64, 65, 100, 128, 129, 150, 191, 192, 193, 200, 250, 256, 257, 300, 384, 400, 512, 700, 768, 769,
      1024, 2048, 4096]
SHAPES = [(4096, 4096), (4096, 12288), (4096, 22016), (11008, 4096), (4096, 4000), (1024, 1000), (1152, 1000), (1001, 1000), (256, 4096),
          (4160, 4096), (512, 32000)]
EPILOGUES = ["plain", "bias+residual", "swiglu"]
# operand addresses: never dereferenced, only their alignment counts (each 256-byte aligned; x may sit 2 bytes further)
X, W, SCALE, Y, BIAS, RESIDUAL, WORKSPACE = (0x10000000 * (i + 1) for i in range(7))


def _route(lib, fmt, group, M, K, N, epi, ws, xoff):
    """ws: None (no workspace) or "auto" (as sized by llmie_linear_workspace_bytes, like the Python wrappers do)"""
    nbytes = lib.llmie_linear_workspace_bytes(fmt, M, K, N) if ws == "auto" else 0
    br = epi == "bias+residual"
    r = lib.llmie_linear_route(fmt, X + xoff, W, SCALE, Y, M, K, N, int(epi == "swiglu"), group, BIAS if br else None,
                               RESIDUAL if br else None, WORKSPACE if nbytes else None, nbytes)
    return r.decode() if r is not None else "refused"


def _prefill_bytes(llmie, fmt, group, T):
    cfg = llmie.DecoderConfig(head_num=32, kv_head_num=32, head_size=128, inter_size=11008, num_layers=32, vocab_size=32000,
                              max_seq_len=4096, max_batch=1, rotary_dim=128, rotary_base=10000.0, rms_eps=1e-5, dtype=llmie.F16, wfmt=fmt,
                              int4_group=group or 128, kv_fmt=0, k_scale=0.0, v_scale=0.0, flags=0)
    return llmie.lib().llmie_decoder_prefill_workspace_bytes(C.byref(cfg), T, 1)


def _rle(values):
    """run-length code over M: value*count"""
    out = []
    for v in values:
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return " ".join("%s*%d" % (v, n) for v, n in out)


def recording(llmie, route=_route):
    """key -> run-length coded answers over MS, in the fixture's order"""
    lib = llmie.lib()
    rec = {}
    for fname, fmt, group in FORMATS:
        for K, N in SHAPES:
            for epi in EPILOGUES:
                for ws in (None, "auto"):
                    for xoff in (0, 2):
                        key = "route %s K=%d N=%d %s ws=%s x+%d" % (fname, K, N, epi, ws or "none", xoff)
                        rec[key] = _rle(route(lib, fmt, group, M, K, N, epi, ws, xoff) for M in MS)
            rec["linear_workspace_bytes %s K=%d N=%d" % (fname, K, N)] = _rle(lib.llmie_linear_workspace_bytes(fmt, M, K, N) for M in MS)
        rec["prefill_workspace_bytes %s 7B" % fname] = _rle(_prefill_bytes(llmie, fmt, group, T) for T in MS)
    return rec


def _route_fp8(lib, M, K, N, epi, ws, xoff):
    """ws: None or "auto" (as sized by llmie_linear_fp8_workspace_bytes(M, K, N): the activation part, then the slabs)"""
    nbytes = lib.llmie_linear_fp8_workspace_bytes(M, K, N) if ws == "auto" else 0
    br = epi == "bias+residual"
    r = lib.llmie_linear_route(W_FP8, X + xoff, W, SCALE, Y, M, K, N, 0, 0, BIAS if br else None, RESIDUAL if br else None,
                               WORKSPACE if nbytes else None, nbytes)
    return r.decode() if r is not None else "refused"


def recording_fp8(llmie, route=_route_fp8):
    """the fp8 lines (golden/linear_routes_fp8.txt): llmie_linear_fp8's routes and the three size queries that follow them"""
    lib = llmie.lib()
    rec = {}
    for K, N in SHAPES:
        for epi in EPILOGUES[:2]:
            for ws in (None, "auto"):
                for xoff in (0, 2):
                    key = "route fp8 K=%d N=%d %s ws=%s x+%d" % (K, N, epi, ws or "none", xoff)
                    rec[key] = _rle(route(lib, M, K, N, epi, ws, xoff) for M in MS)
        rec["linear_fp8_workspace_bytes K=%d N=%d" % (K, N)] = _rle(lib.llmie_linear_fp8_workspace_bytes(M, K, N) for M in MS)
        rec["linear_workspace_bytes fp8 K=%d N=%d" % (K, N)] = _rle(lib.llmie_linear_workspace_bytes(W_FP8, M, K, N) for M in MS)
    rec["prefill_workspace_bytes fp8 7B"] = _rle(_prefill_bytes(llmie, W_FP8, 0, T) for T in MS)
    return rec


def _fixture(path=FIXTURE):
    rec = {}
    for line in open(path):
        if line.strip() and not line.startswith("#"):
            key, val = line.rstrip("\n").split(" : ")
            rec[key] = val
    return rec


@pytest.fixture(scope="module")
def built(llmie):
    llmie.build()
    return llmie


def test_routes_and_sizes_reproduce_the_recording(built):
    got, exp = recording(built), _fixture()
    assert list(got) == list(exp), "the grid of the fixture is not the grid of this test"
    wrong = ["%s\n    recorded %s\n    planned  %s" % (k, exp[k], got[k]) for k in exp if got[k] != exp[k]]
    assert not wrong, "%d of %d lines differ:\n%s" % (len(wrong), len(exp), "\n".join(wrong[:20]))


def test_fp8_routes_and_sizes_reproduce_the_recording(built):
    """linear_routes_fp8.txt: recorded like the first file, from linear_fp8 as it chose its kernels inline (a dry-run build in which
    each of its launch sites -- the GEMV, the tiled GEMM, the split-K passes -- returned its name, through llmie_linear_fp8 and so
    behind that entry's own checks), before plan_linear_fp8 existed.  A second file, so that the first keeps its grid."""
    got, exp = recording_fp8(built), _fixture(FIXTURE_FP8)
    assert list(got) == list(exp), "the grid of the fixture is not the grid of this test"
    wrong = ["%s\n    recorded %s\n    planned  %s" % (k, exp[k], got[k]) for k in exp if got[k] != exp[k]]
    assert not wrong, "%d of %d lines differ:\n%s" % (len(wrong), len(exp), "\n".join(wrong[:20]))
    routes = {r.split("*")[0] for k, v in exp.items() if k.startswith("route ") for r in v.split(" ")}
    assert routes == {"fp8_gemv", "fp8_gemm256", "fp8_splitk", "refused"}, routes


# the route each case id of tests/test_linear_routes_gpu.py names (longest prefix first)
ROUTE_OF_ID = [
    ("gemv", "gemv_ksplit"), ("skinny", "skinny"), ("splitk", "splitk"), ("passes", "splitk_passes"), ("midtiles", "tiles256_part"),
    ("tiled", "tiles128"), ("generic", "generic"),
    ("i8_gemv", "gemv_ksplit"), ("i8_skinny", "int8_skinny"), ("i8_splitk", "int8_splitk"), ("i8_midpasses", "int8_splitk_passes"),
    ("i8_image_k1152", "image_last+tiles128"), ("i8_image", "image_prefill+tiles256_part"),
    ("i4_gemv", "gemv_ksplit"), ("i4_splitk", "int4_splitk"), ("i4_chunks", "int4_chunks"), ("i4_image", "image_prefill+tiles256_part"),
]


def _named_route(case_id):
    return max((p for p in ROUTE_OF_ID if case_id.startswith(p[0])), key=lambda p: len(p[0]))[1]


@pytest.mark.parametrize("name,M,K,N,ws,xoff", F16_CASES, ids=[c[0] for c in F16_CASES])
def test_f16_case_takes_the_route_its_id_names(built, name, M, K, N, ws, xoff):
    assert _route(built.lib(), W_F16, 0, M, K, N, "bias+residual", ws, 2 * xoff) == _named_route(name)


@pytest.mark.parametrize("name,bits,M,K,N,group,ws", WQ_CASES, ids=[c[0] for c in WQ_CASES])
def test_quantised_case_takes_the_route_its_id_names(built, name, bits, M, K, N, group, ws):
    assert _route(built.lib(), W_INT8 if bits == 8 else W_INT4, group, M, K, N, "bias+residual", ws, 0) == _named_route(name)


def test_fused_swiglu_is_offered_exactly_where_the_ladders_ran_it(built):
    """"Has this call a fused SwiGLU form?" used to be answered by hand-written copies of the ladders' conditions; it is now "the plan
    is not refused".  Against the recorded ladders: no route where they refused, a route wherever they ran, and a reason with every
    refusal."""
    lib, exp = built.lib(), _fixture()
    for fname, fmt, group in FORMATS:
        for K, N in SHAPES:
            for ws in (None, "auto"):
                for xoff in (0, 2):
                    runs = exp["route %s K=%d N=%d swiglu ws=%s x+%d" % (fname, K, N, ws or "none", xoff)].split(" ")
                    recorded = [r.split("*")[0] for r in runs for _ in range(int(r.split("*")[1]))]
                    for M, was in zip(MS, recorded):
                        eligible = _route(lib, fmt, group, M, K, N, "swiglu", ws, xoff) != "refused"
                        assert eligible == (was != "refused"), (fname, M, K, N, ws, xoff, was)
                        assert eligible or lib.llmie_last_error(), (fname, M, K, N)
