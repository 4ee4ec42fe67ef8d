"""The launch plan of the decode attention, asserted without a GPU through llmie_decoder_mha_plan (pure host code).

tests/golden/decode_attn_plans.txt was recorded from the launchers as they stood before the planner existed (launch_split,
dispatch_rep, decoder_mha_impl / decoder_mha_fp8kv, decoder_mha_rope and the three public entries, with a dry-run probe at the split,
merge and generic launches that appended the kernel's template arguments, grid, block, dynamic LDS and chunks per workgroup instead
of launching, and the returned status around it), over the grid below.  The planner must reproduce the recording exactly.

The second half holds tests/attn_cases.py to the plan: its chunk_len() and e4m3_cpw() restate two launch facts by hand (that module
must work without the library), and its seeded-defect classes are right only if they agree with the launcher.
"""
import ctypes
import os

import pytest

import attn_cases as ac

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_attn_plans.txt")
STATUS = {0: "OK", -1: "INVALID_ARG", -2: "UNSUPPORTED", -3: "LAUNCH", -4: "WORKSPACE"}
F = {"step_dev": 1, "ragged": 2, "bias": 4, "rope": 8, "tickets": 16, "slabs": 32, "paged": 64, "x32": 128, "bad_scales": 256}
OPERANDS = ("qkv", "bias", "k", "v", "slab", "wf", "wh", "slab_stride")

DTYPES = [("f16", 1), ("f32", 0)]
CACHES = ["native", "e4m3"]
HEAD_SIZES = [4, 32, 64, 80, 128, 256]
RATIOS = [1, 2, 3, 4, 8, 16]
BATCHES = [1, 2, 15, 16, 31, 32, 33, 64, 128, 65536]
KVH = 8            # batch 16 / 32 / 64 = 2 / 4 / 8 chunks per workgroup over the e4m3 cache
HOST_MAX_SEQ = 15488
BOUNDS = ["1", "C-1", "C", "C+1", "16C+1", "15360", "15361"]
# the forms of the public entries and the combinations the engine uses
FORMS = [("plain", ()), ("bias", ("bias",)), ("step_dev", ("step_dev",)), ("rope", ("rope",)), ("rope_dev", ("rope", "step_dev")),
         ("rope_tickets", ("rope", "tickets")), ("tickets", ("tickets",)), ("ragged", ("ragged", "step_dev", "rope")),
         ("ragged_no_lengths", ("ragged", "rope")), ("paged_ragged", ("paged", "ragged", "step_dev", "rope")),
         ("paged", ("paged", "rope")), ("paged_too_few_pages", ("paged", "ragged", "step_dev", "rope")),
         ("slabs", ("slabs", "rope", "step_dev")), ("x32", ("x32", "rope", "step_dev")),
         ("slabs_x32", ("slabs", "x32", "rope", "step_dev", "bias")), ("slabs_paged_ragged", ("slabs", "paged", "ragged", "rope", "step_dev")),
         ("bad_scales", ("bad_scales", "rope"))]
FORM_GEOMETRIES = [(128, 4), (80, 1), (64, 8)]
BATCH_GEOMETRIES = [(128, 4), (64, 8), (64, 1), (80, 1), (128, 3)]
ALIGN_FORMS = [("bias", ("bias",)), ("rope_dev", ("rope", "bias", "step_dev")), ("tickets", ("tickets", "bias")),
               ("slabs", ("slabs", "rope", "bias", "step_dev"))]


def chunk(dtype, cache, hs, batch):
    """tokens per workgroup of the geometry's split kernel (32, the workspace query's minimum chunk, where it has none)"""
    if hs not in ((64, 128) if cache == "e4m3" else (32, 64, 128, 256)):
        return 32
    if cache == "e4m3":
        cpw = 1
        while cpw < 8 and batch * KVH >= 128 * cpw:
            cpw *= 2
        return cpw * ac.chunk_len(ac.F16, hs, e4m3=True)
    return ac.chunk_len(dtype, hs)


def bound_of(name, C):
    return {"1": 1, "C-1": C - 1, "C": C, "C+1": C + 1, "16C+1": 16 * C + 1, "15360": 15360, "15361": 15361}[name]


def workspace_bytes(batch, head_num, head_size, max_seq_len):
    return batch * head_num * -(-max_seq_len // 32) * (head_size + 2) * 4


def _rle(values):
    out = []
    for v in values:
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return "; ".join("%s*%d" % (v, n) for v, n in out)


def recording(plan):
    """key -> run-length coded plans, in the fixture's order.  plan(dtype code, kv_e4m3, batch, head_num, kv_head_num, head_size,
    max_seq_len, step, forms, max_pages, num_pages, residues, workspace_bytes) -> (text or None, status)"""
    def one(dt, cache, hs, ratio, batch, bound, forms=(), mis=None, ws="exact", few_pages=False):
        dev = "step_dev" in forms
        max_seq = bound if dev else HOST_MAX_SEQ
        nh = KVH * ratio
        need = workspace_bytes(batch, nh, hs, max_seq)
        wsb = {"exact": need, "short": need - 1, "absent": -1}[ws]
        max_pages = -(-max_seq // 128) - (1 if few_pages else 0)
        res = 0 if mis is None else 2 << (4 * OPERANDS.index(mis))
        text, status = plan(dict(DTYPES)[dt], int(cache == "e4m3"), batch, nh, KVH, hs, max_seq, -1 if dev else bound,
                            sum(F[f] for f in forms), max_pages if "paged" in forms else 0, batch * max_pages + 1 if "paged" in forms else 0,
                            res, wsb)
        assert (text is None) == (status != 0)
        return text if text is not None else "refused " + STATUS[status]

    rec = {}
    for dt, _ in DTYPES:
        for cache in CACHES:
            for hs in HEAD_SIZES:
                for ratio in RATIOS:   # the bound, at batch 2
                    C = chunk(dt, cache, hs, 2)
                    rec["bounds %s %s hs%d r%d" % (dt, cache, hs, ratio)] = _rle(one(dt, cache, hs, ratio, 2, bound_of(b, C)) for b in BOUNDS)
            for hs, ratio in BATCH_GEOMETRIES:   # the batch, at the bound C + 1 of that batch
                rec["batches %s %s hs%d r%d" % (dt, cache, hs, ratio)] = _rle(
                    one(dt, cache, hs, ratio, b, chunk(dt, cache, hs, b) + 1) for b in BATCHES)
            for name, forms in FORMS:   # batches 2 and 33 at the bound C + 1, batch 2 at 15361
                for hs, ratio in FORM_GEOMETRIES:
                    rec["form %s %s %s hs%d r%d" % (name, dt, cache, hs, ratio)] = _rle(
                        one(dt, cache, hs, ratio, b, bound_of(bd, chunk(dt, cache, hs, b)), forms, few_pages=name == "paged_too_few_pages")
                        for b, bd in ((2, "C+1"), (33, "C+1"), (2, "15361")))
            for name, forms in ALIGN_FORMS:   # every pointer aligned, then each in turn 2 bytes off
                C = chunk(dt, cache, 128, 2)
                rec["alignment %s %s %s hs128 r4" % (name, dt, cache)] = _rle(one(dt, cache, 128, 4, 2, C + 1, forms, mis=m) for m in (None,) + OPERANDS)
            for hs, ratio in FORM_GEOMETRIES:   # workspace absent, one byte short, exact
                for name, forms in (("plain", ()), ("rope_dev", ("rope", "step_dev"))):
                    C = chunk(dt, cache, hs, 2)
                    rec["workspace %s %s %s hs%d r%d" % (name, dt, cache, hs, ratio)] = _rle(
                        one(dt, cache, hs, ratio, 2, C + 1, forms, ws=w) for w in ("absent", "short", "exact"))
    return rec


def ctypes_plan(fn):
    """plan() of recording() over a C function with llmie_decoder_mha_plan's signature"""
    fn.restype = ctypes.c_char_p
    fn.argtypes = [ctypes.c_int] * 8 + [ctypes.c_uint, ctypes.c_int, ctypes.c_int, ctypes.c_ulonglong, ctypes.c_longlong, ctypes.c_void_p]

    def plan(*args):
        status = ctypes.c_int(0)
        t = fn(*args, ctypes.addressof(status))
        return (t.decode() if t is not None else None), status.value
    return plan


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


def test_plans_reproduce_the_recording(built):
    got, exp = recording(ctypes_plan(built.lib().llmie_decoder_mha_plan)), _fixture()
    assert list(got) == list(exp), "the grid of the fixture is not the grid of this test"
    wrong = ["%s\n    recorded %s\n    planned  %s" % (k, exp[k], got[k]) for k in exp if got[k] != exp[k]]
    assert not wrong, "%d of %d lines differ:\n%s" % (len(wrong), len(exp), "\n".join(wrong[:20]))


def _fields(text):
    """{"kind", "cpw", "chunk", ...} of a plan text"""
    words = text.split()
    out = {"kind": words[0]}
    for w in words:
        for key in ("cpw", "chunk"):
            if w.startswith(key):
                out[key] = int(w[len(key):])
    return out


def test_attn_cases_chunk_and_cpw_are_the_plans(built):
    """every case of tests/attn_cases.py: the kind its test expects, and the module's hand-copied chunk length and chunks per workgroup"""
    code = {ac.F16: built.F16, ac.F32: built.F32}
    seen = set()
    for _, dtype, geo, step, _ in ac.uniform_cases():
        hs, ratio, bs, max_seq = geo[0], geo[1], geo[2], ac.max_seq_of(dtype, geo[0], geo[6])
        for forms in ((), ("step_dev",), ("rope",), ("rope", "tickets")):
            text, status = built.decoder_mha_plan(code[dtype], bs, ac.NH, ac.NH // ratio, hs, max_seq, step, forms=forms + (("bias",) if geo[5] else ()))
            assert status == 0, (dtype, geo, step, forms, built.lib().llmie_last_error())
            f = _fields(text)
            assert (f["kind"], f["cpw"], f["chunk"]) == ("split", 1, ac.chunk_len(dtype, hs)), (dtype, geo, step, forms, text)
        seen.add(("uniform", dtype, hs, ratio))
    for _, dtype, geo, steps in ac.ragged_cases():
        hs, ratio, bs, max_seq = geo[0], geo[1], geo[2], ac.max_seq_of(dtype, geo[0], geo[6])
        max_pages = -(-max_seq // ac.KV_PAGE)
        for forms, pages in ((("ragged", "step_dev", "rope"), 0), (("ragged", "step_dev", "rope", "paged"), max_pages)):
            text, status = built.decoder_mha_plan(code[dtype], bs, ac.NH, ac.NH // ratio, hs, max_seq, forms=forms + (("bias",) if geo[5] else ()),
                                                  max_pages=pages, num_pages=bs * pages + 3 if pages else 0)
            assert status == 0, (dtype, geo, steps, forms, built.lib().llmie_last_error())
            f = _fields(text)
            assert (f["kind"], f["cpw"], f["chunk"]) == ("split", 1, ac.chunk_len(dtype, hs)), (dtype, geo, steps, forms, text)
        seen.add(("ragged", dtype, hs, ratio))
    for _, dtype, g, step in ac.generic_cases():
        hs, nh, kvh, bs, bias = g
        text, status = built.decoder_mha_plan(code[dtype], bs, nh, kvh, hs, ac.GENERIC_MAX_SEQ, step, forms=("bias",) if bias else ())
        assert status == 0 and _fields(text)["kind"] == "generic", (dtype, g, step, text)
        seen.add(("generic", dtype, hs, nh // kvh))
    for _, hs, ratio, bs, _, step in ac.e4m3_cases():   # as the engine calls it: RoPE fused, the position on the device
        text, status = built.decoder_mha_plan(built.F16, bs, ac.E4M3_KVH * ratio, ac.E4M3_KVH, hs, ac.e4m3_max_seq(hs), kv_e4m3=True,
                                              forms=("rope", "step_dev"))
        assert status == 0, (hs, ratio, bs, step, built.lib().llmie_last_error())
        f = _fields(text)
        assert (f["kind"], f["cpw"], f["chunk"]) == ("split", ac.e4m3_cpw(bs), ac.e4m3_cpw(bs) * ac.chunk_len(ac.F16, hs, e4m3=True)), (hs, ratio, bs, text)
        seen.add(("e4m3", hs, ratio, bs))
    assert len(seen) == 2 * (2 * len(ac.GEOMETRIES) + len(ac.GEOMETRIES_F32_ONLY)) + 2 * len(ac.GENERIC) + 12


def test_the_entries_return_the_recorded_status(built):
    """refused calls return before any launch: made-up aligned addresses, no device (as tests/test_abi_cpu.py)"""
    lib, rec = built.lib(), _fixture()
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
    q, k, v, o, ws, tab, lens, table = (0x1000 * i for i in range(1, 9))
    need = lambda bs, nh, hs, ms: workspace_bytes(bs, nh, hs, ms)

    def recorded(key, index):   # the index-th value of a run-length coded line
        vals = [val for part in rec[key].split("; ") for val in [part.rsplit("*", 1)[0]] * int(part.rsplit("*", 1)[1])]
        return {"refused " + name: code for code, name in STATUS.items()}[vals[index]]

    # head ratio 3 with RoPE (hs 128, kv heads 8 -> 24 heads)
    assert lib.llmie_decoder_mha_rope(q, None, k, v, o, 0, 2, 24, 8, 128, 256, 129, None, ws, need(2, 24, 128, 256), tab, 128, None, built.F16,
                                      None) == UNSUPPORTED
    # paged with head size 80
    C1 = 33
    assert lib.llmie_decoder_mha_ragged(q, None, k, v, o, 0, 2, 8, 8, 80, C1, lens, ws, need(2, 8, 80, C1), tab, 80, table, 1, 3, built.F16,
                                        None) == UNSUPPORTED == recorded("form paged_ragged f16 native hs80 r1", 0)
    # ragged without lengths
    assert lib.llmie_decoder_mha_ragged(q, None, k, v, o, 0, 2, 32, 8, 128, 129, None, ws, need(2, 32, 128, 129), tab, 128, None, 0, 0, built.F16,
                                        None) == INVALID == recorded("form ragged_no_lengths f16 native hs128 r4", 0)
    # one byte short of the workspace: LLMIE_ERR_WORKSPACE over the native cache ...
    n = need(2, 32, 128, HOST_MAX_SEQ)
    assert lib.llmie_decoder_mha(q, None, k, v, o, 0, 2, 32, 8, 128, HOST_MAX_SEQ, 129, None, ws, n - 1, built.F16,
                                 None) == WORKSPACE == recorded("workspace plain f16 native hs128 r4", 1)
    assert b"workspace too small" in lib.llmie_last_error()
    # ... and LLMIE_ERR_UNSUPPORTED over the e4m3 cache, which no public entry reaches: the engine's call, through the query
    assert built.decoder_mha_plan(built.F16, 2, 32, 8, 128, 257, kv_e4m3=True, forms=("rope", "step_dev"),
                                  workspace_bytes=need(2, 32, 128, 257) - 1) == (None, UNSUPPORTED)
    assert recorded("workspace rope_dev f16 e4m3 hs128 r4", 1) == UNSUPPORTED
    # the generic kernel's logits of 15361 tokens do not fit the LDS
    assert lib.llmie_decoder_mha(q, None, k, v, o, 0, 2, 8, 8, 80, HOST_MAX_SEQ, 15361, None, ws, 0, built.F16,
                                 None) == UNSUPPORTED == recorded("bounds f16 native hs80 r1", 6)
    assert b"15360" in lib.llmie_last_error()
