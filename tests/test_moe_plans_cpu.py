"""The plan line of every mixture-of-experts call of a sweep, and the workspace queries, byte for byte (no GPU): what
llmie_moe_ffn_plan and llmie_moe_ffn_plan_ex print -- or `REFUSED rc text` where they refuse -- for fp16 and MXFP4 experts under
both acts, every row count 1..40 and the counts around the tile and RT edges, eight (hidden, inter) pairs up to and past the GEMV
kernels' 16384, four (experts, top_k) and every flag alone; and llmie_moe_workspace_bytes / llmie_decoder_moe_workspace_bytes on
the same geometries.  golden/moe_plans.txt.gz holds what the library printed when it was recorded (`python
tests/test_moe_plans_cpu.py --record`), one line per call: the planner, the plan text and the covering carve can be rearranged, and
a route, grid, tile count or workspace byte that moves fails here.  (The sweep is 45,000 lines, 7 MB as text: the file is the
gzip of that text, with a zeroed time stamp.)"""
import ctypes as C
import gzip
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "moe_plans.txt.gz")
W_F16, W_MXFP4 = 0, 5
FORMATS = (("f16", W_F16), ("mxfp4", W_MXFP4))
ACTS = (0, 1)
ROWS = tuple(range(1, 41)) + (63, 64, 65, 127, 128, 129, 300)
GEOMETRIES = ((64, 64), (256, 192), (2112, 64), (64, 2112), (4160, 64), (8256, 64), (16384, 64), (16448, 64))
EK = ((1, 1), (4, 1), (8, 2), (128, 8))
FLAGS = (0, 2, 4, 8, 16, 1)   # none, LLMIE_MOE_FORCE_GEMV, _FORCE_GROUPED, _FORCE_RT1, _FORCE_RT4, LLMIE_MOE_SOFTMAX_ALL
MAX_ROWS = (1, 4, 5, 16, 17, 127, 128, 300)
ENGINE_MAX_BATCH = 8


def _answer(lib, text):
    if text is not None:
        return text.decode()
    # (the plan queries return no code: the text of the refusal says which rule)
    return "REFUSED " + lib.llmie_last_error().decode()


def recording(llmie):
    """the file's lines, in its order"""
    lib = llmie.lib()
    lines = []
    for H, Ie in GEOMETRIES:
        for E, k in EK:
            for flags in FLAGS:
                for rows in ROWS:
                    call = (rows, H, Ie, E, k, flags)
                    lines.append("plan %d %d %d %d %d %d -> %s" % (call + (_answer(lib, lib.llmie_moe_ffn_plan(*call)),)))
                    for fname, fmt in FORMATS:
                        for act in ACTS:
                            lines.append("plan_ex %d %d %d %d %d %d %s %d -> %s" %
                                         (call + (fname, act, _answer(lib, lib.llmie_moe_ffn_plan_ex(*(call + (fmt, act)))))))
            cfg = llmie.DecoderConfig(head_num=H // 64, kv_head_num=H // 64, head_size=64, inter_size=64, num_layers=2, vocab_size=100,
                                      max_seq_len=64, max_batch=ENGINE_MAX_BATCH, rotary_dim=64, rotary_base=10000.0, rms_eps=1e-5, dtype=1,
                                      wfmt=W_F16, int4_group=128, kv_fmt=0, k_scale=0.0, v_scale=0.0, flags=0)
            for max_rows in MAX_ROWS:
                lines.append("workspace %d %d %d %d %d -> %d" % (max_rows, H, Ie, E, k, lib.llmie_moe_workspace_bytes(max_rows, H, Ie, E, k)))
                lines.append("decoder_workspace max_batch=%d %d %d %d %d %d -> %d" %
                             (ENGINE_MAX_BATCH, max_rows, H, Ie, E, k, lib.llmie_decoder_moe_workspace_bytes(C.byref(cfg), max_rows, Ie, E, k)))
    return lines


def _fixture():
    with gzip.open(GOLDEN, "rt") as f:
        return f.read().splitlines()


def test_the_recording_covers_the_sweep():
    lines = _fixture()
    per_call = 1 + len(FORMATS) * len(ACTS)
    assert len(lines) == len(GEOMETRIES) * len(EK) * (len(FLAGS) * len(ROWS) * per_call + 2 * len(MAX_ROWS))
    text = "\n".join(lines)
    for word in ("route=gemv rt=0", "route=grouped rt=1", "route=grouped rt=4", "format=mxfp4 act=swiglu_clamped", "format=f16 act=swiglu",
                 "REFUSED moe_ffn_plan: LLMIE_MOE_FORCE_GEMV with 17 rows", "REFUSED moe_ffn_plan_ex: LLMIE_MOE_FORCE_GEMV with hidden=16448"):
        assert word in text, word
    assert not any(line.endswith("-> 0") for line in lines if line.startswith(("workspace", "decoder_workspace")))


def test_every_plan_line_and_workspace_size_is_the_recorded_one(llmie):
    llmie.build()
    got, exp = recording(llmie), _fixture()
    wrong = [(g, e) for g, e in zip(got, exp) if g != e]
    assert len(got) == len(exp) and not wrong, "%d of %d lines differ, the first:\n got %s\n exp %s" % ((len(wrong), len(exp)) + (wrong or [("", "")])[0])


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_moe_plans_cpu.py --record")
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from conftest import load_llmie
    rec = recording(load_llmie())
    with open(GOLDEN, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
        f.write(("\n".join(rec) + "\n").encode())
    print("recorded %d lines" % len(rec))
