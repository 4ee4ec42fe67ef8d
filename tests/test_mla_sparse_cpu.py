"""MLA sparse decode without a GPU: both planners are pure host code -- the plan texts and their grid arithmetic, every refusal of the
planners and of the entries (pointers that are never dereferenced), the workspace sizes --, and the three kernels' registers, LDS and
scratch on the built code object."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built(llmie):
    llmie.build()
    return llmie


@pytest.mark.parametrize("heads,top_k,batch", [(16, 1, 1), (16, 256, 3), (32, 257, 2), (128, 2048, 2), (128, 4096, 1)])
def test_sparse_plan_follows_top_k(built, heads, top_k, batch):
    splits = -(-top_k // 256)
    merge = "none" if splits == 1 else "%dx%d/128" % (heads, batch)
    want = "mla_sparse f16 nh%d hb16 tile32 chunk256 topk%d grid %dx%dx%d merge %s" % (heads, top_k, splits, heads // 16, batch, merge)
    assert built.mla_decode_sparse_plan(batch, heads, top_k, 8192) == (want, 0)
    assert built.mla_decode_sparse_plan(batch, heads, top_k, 8192, paged=True, max_pages=64, num_pages=200) == (want, 0)
    assert built.lib().llmie_mla_decode_workspace_bytes(batch, heads, top_k) == (0 if splits == 1 else batch * heads * splits * 514 * 4)


@pytest.mark.parametrize("batch,top_k,max_seq_len,max_ctx,grid", [
    (2, 2048, 32768, 0, "512x2"), (1, 64, 300, 257, "5x1"), (3, 40, 700, 0, "11x3"), (1, 256, 256, 0, "none"), (2, 256, 700, 200, "none")])
def test_index_plan_and_workspace(built, batch, top_k, max_seq_len, max_ctx, grid):
    want = "mla_index f16 ih64 id128 keys64 topk%d grid %s select %dx1024" % (top_k, grid, batch)
    assert built.mla_index_topk_plan(batch, top_k, max_seq_len, max_ctx) == (want, 0)
    span = max_ctx or max_seq_len
    need = batch * -(-span // 256) * 256 * 4
    assert built.lib().llmie_mla_index_topk_workspace_bytes(batch, span) == need
    short = built.mla_index_topk_plan(batch, top_k, max_seq_len, max_ctx, workspace_bytes=need - 1)
    assert short == ((want, 0) if grid == "none" else (None, -4))   # no logits, no workspace


SPARSE = dict(batch=2, head_num=16, top_k=512, max_seq_len=1024)
INDEX = dict(batch=2, top_k=64, max_seq_len=1024)


@pytest.mark.parametrize("base,kwargs,status,word", [
    (SPARSE, dict(batch=0), -1, "batch=0"), (SPARSE, dict(head_num=24), -2, "head_num=24"), (SPARSE, dict(head_num=144), -2, "head_num=144"),
    (SPARSE, dict(max_seq_len=0), -1, "max_seq_len"), (SPARSE, dict(top_k=0), -1, "top_k=0"), (SPARSE, dict(top_k=4097), -1, "top_k=4097"),
    (SPARSE, dict(paged=True, max_pages=7, num_pages=8), -1, "max_pages=7"),
    (SPARSE, dict(paged=True, max_pages=8, num_pages=1 << 24), -2, "2^31 - 1"), (SPARSE, dict(batch=3, max_seq_len=1 << 30), -2, "2^31 - 1"),
    (SPARSE, dict(workspace_bytes=2 * 16 * 2 * 514 * 4 - 1), -4, "workspace"), (SPARSE, dict(workspace_bytes=None), -4, "workspace"),
    (INDEX, dict(batch=0), -1, "batch=0"), (INDEX, dict(batch=65536), -1, "batch=65536"), (INDEX, dict(top_k=0), -1, "top_k=0"),
    (INDEX, dict(top_k=4097), -1, "top_k=4097"), (INDEX, dict(max_seq_len=0), -1, "max_seq_len"), (INDEX, dict(max_ctx=1025), -1, "max_ctx"),
    (INDEX, dict(paged=True, max_pages=7, num_pages=8), -1, "max_pages=7"), (INDEX, dict(workspace_bytes=None), -4, "workspace"),
])
def test_planner_refusals_carry_a_message(built, base, kwargs, status, word):
    plan = built.mla_decode_sparse_plan if base is SPARSE else built.mla_index_topk_plan
    assert plan(**dict(base, **kwargs)) == (None, status)
    assert word in built.lib().llmie_last_error().decode()


P, ODD = 4096, 4104   # addresses that are never dereferenced: every refusal comes first
# the arguments of a good call, in the entry's order (llmie_mla_decode_sparse: 18, llmie_mla_index_topk: 18)
ENTRY = dict(decode_sparse=dict(q_lat=P, cache=P, o_lat=P, sel=P, sel_count=P, layer=0, batch=2, head_num=16, top_k=512, max_seq_len=1024, ctx_len=P,
                                scale=0.1, workspace=P, workspace_bytes=1 << 20, block_table=None, max_pages=0, num_pages=0, stream=None),
             index_topk=dict(q_idx=P, w_idx=P, k_idx=P, sel=P, sel_count=P, logits_out=None, layer=0, batch=2, top_k=64, max_seq_len=1024, max_ctx=0,
                             ctx_len=P, workspace=P, workspace_bytes=1 << 20, block_table=None, max_pages=0, num_pages=0, stream=None))


@pytest.mark.parametrize("entry,kwargs,status,word", [
    ("decode_sparse", dict(sel=None), -1, "NULL"), ("decode_sparse", dict(sel_count=None), -1, "NULL"), ("decode_sparse", dict(q_lat=None), -1, "NULL"),
    ("decode_sparse", dict(layer=-1), -1, "layer=-1"), ("decode_sparse", dict(scale=0.0), -1, "softmax_scale"),
    ("decode_sparse", dict(scale=float("inf")), -1, "softmax_scale"), ("decode_sparse", dict(top_k=5000), -1, "top_k=5000"),
    ("decode_sparse", dict(head_num=8), -2, "head_num=8"), ("decode_sparse", dict(workspace=None), -4, "workspace"),
    ("decode_sparse", dict(workspace_bytes=100), -4, "workspace"), ("decode_sparse", dict(workspace=ODD), -1, "aligned"),
    ("decode_sparse", dict(cache=ODD), -1, "aligned"), ("decode_sparse", dict(block_table=P, max_pages=7, num_pages=8), -1, "max_pages=7"),
    ("index_topk", dict(w_idx=None), -1, "NULL"), ("index_topk", dict(sel=None), -1, "NULL"), ("index_topk", dict(ctx_len=None), -1, "NULL"),
    ("index_topk", dict(layer=-1), -1, "layer=-1"), ("index_topk", dict(top_k=0), -1, "top_k=0"), ("index_topk", dict(max_ctx=2000), -1, "max_ctx"),
    ("index_topk", dict(workspace=None), -4, "workspace"), ("index_topk", dict(workspace_bytes=2 * 1024 * 4 - 1), -4, "workspace"),
    ("index_topk", dict(workspace=ODD), -1, "aligned"), ("index_topk", dict(q_idx=ODD), -1, "aligned"),
    ("index_topk", dict(block_table=P, max_pages=7, num_pages=8), -1, "max_pages=7"),
])
def test_entries_refuse_before_touching_a_pointer(built, entry, kwargs, status, word):
    assert getattr(built.lib(), "llmie_mla_" + entry)(*dict(ENTRY[entry], **kwargs).values()) == status
    assert word in built.lib().llmie_last_error().decode()


def test_sparse_kernels_resources(built):
    """no scratch, no spills; the attention at two workgroups per CU (LDS <= 80 KB, 256 VGPRs); the logits kernel without LDS"""
    spec = importlib.util.spec_from_file_location("ckr", os.path.join(ROOT, "tools", "check_kernel_resources.py"))
    ckr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ckr)
    ks = ckr.kernel_metadata(os.path.join(ROOT, "llm-inference-engine_amd", "csrc", "_obj", "mla_sparse.hip.o"))
    by = {n: [k for k in ks if n in k["name"]] for n in ("mla_index_logits_kernel", "mla_index_select_kernel", "mla_sparse_attend_kernel")}
    assert all(len(v) == 1 for v in by.values()), [k["name"] for k in ks]
    bad = [k for v in by.values() for k in v if k["vgpr_spill"] or k.get("sgpr_spill") or k["scratch"]]
    assert not bad, bad
    attend, logits = by["mla_sparse_attend_kernel"][0], by["mla_index_logits_kernel"][0]
    assert attend["lds"] <= 81920 and attend["vgpr"] <= 256, attend
    assert logits["lds"] == 0, logits
