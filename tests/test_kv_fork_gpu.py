"""llmie_kv_pages_fork on the GPU against a numpy model of pools, tables and lengths: after the call both pools, the block table
and the lengths equal the model byte for byte EVERYWHERE -- pages that no table names and token rows at and past the tail
included -- for every parent pattern (identity, swap, 3-cycle, all from row 0, a mix with parents out of range), lengths on and
around the page boundaries, fp16 and one-byte caches, rows and pool bases that break 16-byte alignment, and under graph replay."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
L, ROWS, MAX_PAGES = 2, 6, 3
NUM_PAGES = 2 * ROWS * MAX_PAGES + 3
LENS = [0, 1, 127, 128, 129, 255, 256, 300]
PARENTS = {"identity": [0, 1, 2, 3, 4, 5], "swap": [1, 0, 2, 3, 5, 4], "cycle3": [1, 2, 0, 3, 4, 5], "all_from_0": [0, 0, 0, 0, 0, 0],
           "mixed_out_of_range": [3, -1, 0, 6, 4, 2]}


def model_fork(kp, vp, table, own, parent, lens, num_pages):
    """the header's rules on numpy arrays; pools [L, num_pages, kvh, 128, row_bytes] uint8.  Returns new (kp, vp, table, lens)."""
    rows, max_pages = table.shape
    nk, nv, nt, nl = kp.copy(), vp.copy(), table.copy(), lens.copy()
    for j in range(rows):
        q = int(parent[j])
        if q == j or q < 0 or q >= rows:
            continue
        n = int(lens[q])
        if n < 0 or n > 128 * max_pages:
            continue
        pc, r = divmod(n, 128)
        if r > 0:
            src, dst = int(table[q, pc]), int(own[j, pc])
            if not (0 <= src < num_pages and 0 <= dst < num_pages):
                continue
            nk[:, dst, :, :r] = kp[:, src, :, :r]
            nv[:, dst, :, :r] = vp[:, src, :, :r]
        nl[j] = n
        nt[j, :pc] = table[q, :pc]
        nt[j, pc:] = own[j, pc:]
    return nk, nv, nt, nl


def setup(rng, kvh, row_bytes, lens, base_offset=0):
    """pools of random bytes (at `base_offset` bytes into their allocation), pages handed out in shuffled order: every row owns
    MAX_PAGES pages that its table names, and a second set in own_table for the pages a fork writes"""
    perm = rng.permutation(NUM_PAGES)
    table = perm[:ROWS * MAX_PAGES].reshape(ROWS, MAX_PAGES).astype(np.int32)
    own = perm[ROWS * MAX_PAGES:2 * ROWS * MAX_PAGES].reshape(ROWS, MAX_PAGES).astype(np.int32)
    # a row's pages at indices >= cached_len / 128 are its own: there the two tables agree (the caller contract)
    for j in range(ROWS):
        table[j, lens[j] // 128:] = own[j, lens[j] // 128:]
    shape = (L, NUM_PAGES, kvh, 128, row_bytes)
    n = int(np.prod(shape))
    kp, vp = rng.integers(0, 256, n, dtype=np.uint8).reshape(shape), rng.integers(0, 256, n, dtype=np.uint8).reshape(shape)
    dk = torch.zeros(n + 16, dtype=torch.uint8, device=DEV)
    dv = torch.zeros(n + 16, dtype=torch.uint8, device=DEV)
    dkp, dvp = dk[base_offset:base_offset + n].view(shape), dv[base_offset:base_offset + n].view(shape)
    dkp.copy_(torch.from_numpy(kp))
    dvp.copy_(torch.from_numpy(vp))
    return kp, vp, table, own, dkp, dvp


def pools_as(dkp, elem_bytes):
    """the byte pools as the engine's tensors: [L, num_pages, kvh, 128, hs] of elem_bytes-wide elements"""
    return dkp if elem_bytes == 1 else dkp.view(torch.float16)


def run_and_check(llmie, rng, kvh, hs, elem_bytes, parent, lens, base_offset=0):
    row_bytes = hs * elem_bytes
    lens = np.asarray(lens, np.int32)
    kp, vp, table, own, dkp, dvp = setup(rng, kvh, row_bytes, lens, base_offset)
    d_table, d_own = torch.from_numpy(table).to(DEV), torch.from_numpy(own).to(DEV)
    d_parent, d_lens = torch.tensor(parent, dtype=torch.int32, device=DEV), torch.from_numpy(lens).to(DEV)
    if base_offset % 2 == 0 or elem_bytes == 1:
        llmie.kv_pages_fork(pools_as(dkp, elem_bytes), pools_as(dvp, elem_bytes), d_table, d_own, d_parent, d_lens)
    else:   # (a torch view of 2-byte elements cannot start at an odd byte: the C entry takes any address)
        ws = torch.empty(llmie.kv_pages_fork_workspace_bytes(ROWS, L, kvh, hs, elem_bytes, MAX_PAGES), dtype=torch.uint8, device=DEV)
        rc = llmie.lib().llmie_kv_pages_fork(dkp.data_ptr(), dvp.data_ptr(), d_table.data_ptr(), d_own.data_ptr(), d_parent.data_ptr(),
                                             d_lens.data_ptr(), ROWS, L, kvh, hs, MAX_PAGES, NUM_PAGES, elem_bytes, ws.data_ptr(),
                                             ws.numel(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, llmie.lib().llmie_last_error()
    torch.cuda.synchronize()
    ek, ev, et, el = model_fork(kp, vp, table, own, parent, lens, NUM_PAGES)
    assert np.array_equal(d_lens.cpu().numpy(), el)
    assert np.array_equal(d_table.cpu().numpy(), et)
    assert np.array_equal(dkp.cpu().numpy(), ek) and np.array_equal(dvp.cpu().numpy(), ev)
    assert np.array_equal(d_own.cpu().numpy(), own) and d_parent.cpu().tolist() == list(parent)
    return ek, kp


def lens_for(rng, i):
    """six lengths out of LENS, rotated so that the patterns together meet every length as a source"""
    return [LENS[(i + 3 * j) % len(LENS)] for j in range(ROWS)]


@pytest.mark.parametrize("kvh,hs,elem_bytes", [(1, 64, 1), (4, 64, 2), (1, 128, 2), (4, 128, 1)])
@pytest.mark.parametrize("pattern", list(PARENTS))
def test_fork_equals_the_model(llmie, pattern, kvh, hs, elem_bytes):
    rng = np.random.default_rng([len(pattern), kvh, hs, elem_bytes])
    changed = False
    for i in range(len(LENS)):   # every length meets every position of the pattern
        ek, kp = run_and_check(llmie, rng, kvh, hs, elem_bytes, PARENTS[pattern], lens_for(rng, i))
        changed |= not np.array_equal(ek, kp)
    assert changed == (pattern != "identity")   # the cases do copy tails (and the identity copies nothing)


def test_every_length_is_a_source_at_every_tail():
    seen = {lens_for(None, i)[q] for i in range(len(LENS)) for q in range(ROWS)}
    assert seen == set(LENS)


@pytest.mark.parametrize("hs,elem_bytes,base_offset", [(60, 1, 0), (63, 2, 0), (64, 2, 8), (128, 1, 1), (64, 2, 2), (36, 1, 4)])
def test_rows_and_bases_off_the_16_byte_grid(llmie, hs, elem_bytes, base_offset):
    rng = np.random.default_rng([hs, elem_bytes, base_offset])
    for pattern in ("swap", "cycle3", "all_from_0"):
        run_and_check(llmie, rng, 2, hs, elem_bytes, PARENTS[pattern], [129, 255, 1, 300, 127, 130], base_offset)


def test_page_ids_out_of_range_leave_the_row_untouched(llmie):
    """a tail page outside [0, num_pages) on either side, or a parent length outside [0, 128 * max_pages]: the row keeps its table,
    its length and its bytes"""
    rng = np.random.default_rng(5)
    kvh, hs, eb = 2, 64, 2
    lens = np.asarray([130, 5, 385, 128, 64, -3], np.int32)   # (385 and -3: lengths outside [0, 128 * max_pages])
    kp, vp, table, own, dkp, dvp = setup(rng, kvh, hs * eb, lens)
    table[0, 1] = NUM_PAGES     # the source tail page of rows forked from row 0
    own[3, 0] = -1              # the destination tail page of row 3 (from row 4, 64 tokens)
    own[5, 2] = NUM_PAGES + 7   # not a tail page of this fork (row 5 forks at 5 tokens): ids of later pages are not looked at
    parent = [5, 0, 1, 4, 2, 1]      # rows 0 and 4 would take the two impossible lengths
    d_table, d_own = torch.from_numpy(table).to(DEV), torch.from_numpy(own).to(DEV)
    d_parent, d_lens = torch.tensor(parent, dtype=torch.int32, device=DEV), torch.from_numpy(lens).to(DEV)
    llmie.kv_pages_fork(pools_as(dkp, eb), pools_as(dvp, eb), d_table, d_own, d_parent, d_lens)
    torch.cuda.synchronize()
    ek, ev, et, el = model_fork(kp, vp, table, own, parent, lens, NUM_PAGES)
    assert el.tolist() == [130, 5, 5, 128, 64, 5] and np.array_equal(et[1], table[1]) and np.array_equal(et[3], table[3])
    assert et[5, 2] == NUM_PAGES + 7
    assert np.array_equal(d_lens.cpu().numpy(), el) and np.array_equal(d_table.cpu().numpy(), et)
    assert np.array_equal(dkp.cpu().numpy(), ek) and np.array_equal(dvp.cpu().numpy(), ev)


def test_graph_replay_follows_the_new_parent(llmie):
    rng = np.random.default_rng(9)
    kvh, hs, eb = 2, 128, 2
    lens = np.asarray([129, 255, 1, 300, 127, 130], np.int32)
    kp, vp, table, own, dkp, dvp = setup(rng, kvh, hs * eb, lens)
    d_table, d_own, d_lens = torch.from_numpy(table).to(DEV), torch.from_numpy(own).to(DEV), torch.from_numpy(lens).to(DEV)
    d_parent = torch.tensor(PARENTS["identity"], dtype=torch.int32, device=DEV)
    ws = torch.empty(llmie.kv_pages_fork_workspace_bytes(ROWS, L, kvh, hs, eb, MAX_PAGES), dtype=torch.uint8, device=DEV)
    k16, v16 = pools_as(dkp, eb), pools_as(dvp, eb)
    llmie.kv_pages_fork(k16, v16, d_table, d_own, d_parent, d_lens, workspace=ws)   # the identity: changes nothing
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        llmie.kv_pages_fork(k16, v16, d_table, d_own, d_parent, d_lens, workspace=ws)
    torch.cuda.synchronize()
    assert np.array_equal(dkp.cpu().numpy(), kp) and np.array_equal(d_table.cpu().numpy(), table)
    parent = PARENTS["cycle3"]
    d_parent.copy_(torch.tensor(parent, dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    ek, ev, et, el = model_fork(kp, vp, table, own, parent, lens, NUM_PAGES)
    assert not np.array_equal(ek, kp)
    assert np.array_equal(d_lens.cpu().numpy(), el) and np.array_equal(d_table.cpu().numpy(), et)
    assert np.array_equal(dkp.cpu().numpy(), ek) and np.array_equal(dvp.cpu().numpy(), ev)
