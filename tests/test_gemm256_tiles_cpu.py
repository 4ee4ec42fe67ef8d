"""The tile plan of the 256-row GEMM family, asserted without a GPU through llmie_gemm256_tiles (pure host code).

tests/golden/gemm256_tiles.txt was recorded from the three launchers as they stood before the planner existed (gemm256_launch,
gemm256_swiglu_launch and gemm256_qkv_rope_launch with a dry-run probe at every kernel launch, appending the launch's family, tile
width, tile count and first column instead of launching), over the grid below.  The planner must reproduce the recording exactly: a
plan that moves shows on a GPU only as a few percent of prefill time, here it fails.

Plan text: family ("8p" eight-phase, "2s" two-stage; again in front of a range that changes it), then WIDTHxTILES@FIRSTCOL per launch.
"""
import os

import pytest

from test_gemm256_tiles_gpu import CASES
from test_linear_routes_cpu import MS as ROUTE_MS

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm256_tiles.txt")

FORMS = [("plain", 0), ("swiglu", 1), ("qkv_rope", 2)]
OPERANDS = [("f16", 0), ("e4m3", 1), ("int8", 2)]
MS = ROUTE_MS + [8192, 16384]
NS = [1000, 4000, 4096, 4224, 5120, 6144, 8192, 8320, 8328, 8448, 11008, 12288, 13824, 16640, 22016, 28672, 32000]
# (N, K): K = 4096, and one pair past the 32-bit limit of the eight-phase kernels' offsets (fp16: the two-stage fallback; int8 weights
# never take it)
SHAPES = [(N, 4096) for N in NS] + [(32000, 66560)]


def _rle(values):
    """run-length code over M: value*count"""
    out = []
    for v in values:
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return "; ".join("%s*%d" % (v, n) for v, n in out)


def recording(tiles):
    """key -> run-length coded plans over MS, in the fixture's order; tiles(form, operands, M, N, K) -> bytes or None"""
    rec = {}
    for form, fcode in FORMS:
        for ops, ocode in OPERANDS:
            for N, K in SHAPES:
                if form == "qkv_rope" and N % 128 != 0:
                    continue
                rows = 2 * N if form == "swiglu" else N   # SwiGLU: two_inter = 2 N weight rows, plan columns are those of [M, N]
                key = "%s %s N=%d K=%d" % (form, ops, rows, K)
                rec[key] = _rle(tiles(fcode, ocode, M, rows, K).decode() for M in MS)
    return rec


def _fixture():
    rec = {}
    for line in open(FIXTURE):
        if line.strip() and not line.startswith("#"):
            key, val = line.rstrip("\n").split(" : ")
            rec[key] = val
    return rec


@pytest.fixture(scope="module")
def built(llmie):
    llmie.build()
    return llmie


def test_tile_plans_reproduce_the_recording(built):
    got, exp = recording(built.lib().llmie_gemm256_tiles), _fixture()
    assert list(got) == list(exp), "the grid of the fixture is not the grid of this test"
    wrong = ["%s\n    recorded %s\n    planned  %s" % (k, exp[k], got[k]) for k in exp if got[k] != exp[k]]
    assert not wrong, "%d of %d lines differ:\n%s" % (len(wrong), len(exp), "\n".join(wrong[:20]))


@pytest.mark.parametrize("name,form,M,N,plan", CASES, ids=[c[0] for c in CASES])
def test_gpu_case_takes_the_plan_its_id_names(built, name, form, M, N, plan):
    for ops in ("f16", "e4m3", "int8"):
        assert built.gemm256_tiles(form, ops, M, N, 256) == "8p " + plan


def test_arguments_outside_the_forms_are_refused(built):
    lib = built.lib()
    for args in [(3, 0, 256, 256, 256), (0, 3, 256, 256, 256), (0, 0, 0, 256, 256), (1, 0, 256, 4100, 256), (2, 0, 256, 4160, 256)]:
        assert lib.llmie_gemm256_tiles(*args) is None and b"gemm256_tiles" in lib.llmie_last_error()
    assert lib.llmie_gemm256_tiles(0, 0, 1, 1, 1) == b"8p 128x1@0"
