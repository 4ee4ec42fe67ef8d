"""Tests of the sliding-window attention tests (tests/window_attn_cases.py), and what the windowed decode attention promises
without a device: its launch plan (llmie_decoder_mha_window_plan, pure host code) and its argument refusals.  No GPU.
"""
import ctypes

import numpy as np
import pytest

import attn_cases as ac
import test_decode_attn_plan_cpu as plans
import window_attn_cases as wc


@pytest.fixture(scope="module")
def built(llmie):
    llmie.build()
    return llmie


# ------------------------------------------------------------------------------------------------------------- the generator
@pytest.mark.parametrize("geo", wc.GEOMETRIES, ids=[g[0] for g in wc.GEOMETRIES])
def test_a_window_over_the_whole_context_is_full_attention(geo):
    """W >= step: the masked restatement is attn_cases.reference, the reference of the unwindowed tests"""
    C = wc.chunk_of(geo)
    for steps in wc.step_sets(C + 1, C):
        c = wc.build(geo, C + 1, 4, steps)
        full = ac.reference(c)
        assert np.array_equal(wc.reference(c, max(steps), 4), full)
        assert np.array_equal(wc.reference(c, wc.MAX_SEQ + 7, 0), full)
        assert np.array_equal(wc.reference(c, 0, 0), full)
        if max(steps) > C + 1 + 4:   # ... and the case's own window is not: its outside rows dominate the full softmax
            assert np.abs(c.ref - full).max() > 0.1


@pytest.mark.parametrize("cid,geo,W", wc.decode_cases(), ids=[d[0] for d in wc.decode_cases()])
def test_planted_rows_own_the_mask_and_the_outside_rows_would(cid, geo, W):
    """every case of the GPU test: each owner's row holds >= 0.9 of the VISIBLE mass; each row planted just outside the mask would
    hold >= 0.9 of every head's mass if the mask let it in (the generator asserts both; here the numbers are looked at again, and the
    places of the outside rows)"""
    n_out = 0
    for S, steps in wc.sink_sets(W, wc.chunk_of(geo)):
        c = wc.build(geo, W, S, steps)
        for b, s in enumerate(steps):
            vis = wc.visible(s, W, S)
            want = []
            if S < s - W:
                want = [s - 1 - W] + ([S] if S < s - W - 1 else [])
            assert c.outside[b] == want and not any(vis[p] for p in want)
            assert all(vis[p] for p in c.pos[b] if p is not None)
            for h in range(c.nh):
                assert c.pos[b][h] is None or c.mass[b][h] >= 0.9
                assert set(c.out_mass[b][h]) == set(want) and all(m >= 0.9 for m in c.out_mass[b][h].values())
                n_out += len(want)
            for g in range(c.kvh):   # the heads of a KV head own different rows
                own = [p for p in c.pos[b][g * c.rep:(g + 1) * c.rep] if p is not None]
                assert len(own) == len(set(own)) and len(own) == min(c.rep, len(c.classes[b]))
    assert n_out > 0


# ------------------------------------------------------------------------------------------------------ the live-chunk mapping
def test_live_chunks_cover_every_visible_key_once():
    """all (step, W, S, chunk) of a small grid: the chunks are distinct and ascending, each holds a visible key, together they hold
    all of them; a window over the whole context walks the unwindowed chunks; the count respects the device-step bound"""
    for chunk in (1, 2, 3, 4, 8):
        for step in range(1, 42):
            for W in range(0, 46):
                for S in range(0, 20) if W else (0,):
                    live = wc.live_chunks(step, W, S, chunk)
                    vis = wc.visible(step, W, S)
                    assert live == sorted(set(live)), (step, W, S, chunk)
                    covered = np.zeros(step, bool)
                    for ch in live:
                        assert vis[ch * chunk:(ch + 1) * chunk].any(), (step, W, S, chunk, ch)
                        covered[ch * chunk:(ch + 1) * chunk] = True
                    assert not (vis & ~covered).any(), (step, W, S, chunk)
                    if W == 0 or W >= step:
                        assert live == list(range(-(-step // chunk)))
                    assert len(live) <= wc.live_bound(41, W, S, chunk), (step, W, S, chunk)


def _live(text):
    """(window, sinks, "<=" or "", live count) of a windowed plan text"""
    w = text.split()
    i = w.index("window")
    assert w[i + 2] == "sinks" and w[i + 4] == "live"
    n = w[i + 5]
    return int(w[i + 1]), int(w[i + 3]), "<=" if n.startswith("<=") else "", int(n.lstrip("<="))


def _grid_x(text):
    w = text.split()
    return int(w[w.index("grid") + 1].split("x")[0])


@pytest.mark.parametrize("geo", wc.GEOMETRIES, ids=[g[0] for g in wc.GEOMETRIES])
def test_host_step_plans_count_the_live_chunks(built, geo):
    """the planner's live count for a host step is the Python restatement's (which the exhaustive test above checks), and is the
    grid's x extent; the chunk is the one this module assumes"""
    _, hs, ratio, _, scales = geo
    C = wc.chunk_of(geo)
    for W in wc.windows(C) + [wc.MAX_SEQ]:
        for S in (0, 1, 4, C + 3, 2 * C, 2 * C + 5):
            for step in sorted({1, 2, W, W + 1, W + C, W + 2 * C, W + 3 * C - 1, W + C + 37, W + C + 128, wc.MAX_SEQ} & set(range(1, wc.MAX_SEQ + 1))):
                text, status = built.decoder_mha_window_plan(built.F16, wc.BATCH, wc.KVH * ratio, wc.KVH, hs, wc.MAX_SEQ, W, S, step=step,
                                                             kv_e4m3=scales is not None, forms=("rope",))
                assert status == 0, built.lib().llmie_last_error()
                assert "chunk%d " % C in text and " cpw1 " in text
                n = len(wc.live_chunks(step, W, S, C))
                assert _live(text) == (W, S, "", n) and _grid_x(text) == n, (W, S, step, text)
                assert ("merge none" in text) == (n == 1), text


@pytest.mark.parametrize("geo", wc.GEOMETRIES, ids=[g[0] for g in wc.GEOMETRIES])
def test_device_step_grid_is_bounded_by_the_window(built, geo):
    """grid x <= ceil(S / chunk) + ceil(W / chunk) + 1 whatever max_seq_len is"""
    _, hs, ratio, _, scales = geo
    C = wc.chunk_of(geo)
    for W, S in ((1, 0), (5, 4), (C, 1), (C + 1, C + 3), (4096, 4)):
        xs = set()
        for max_seq in (8192, 32768, 131072):
            max_pages = max_seq // 128
            text, status = built.decoder_mha_window_plan(built.F16, 1, wc.KVH * ratio, wc.KVH, hs, max_seq, W, S, kv_e4m3=scales is not None,
                                                         forms=("rope", "ragged", "step_dev", "paged"), max_pages=max_pages, num_pages=64)
            assert status == 0, built.lib().llmie_last_error()
            bound = -(-S // C) + -(-W // C) + 1
            assert _grid_x(text) <= bound and _live(text) == (W, S, "<=", _grid_x(text)), text
            xs.add(_grid_x(text))
            full, _ = built.decoder_mha_plan(built.F16, 1, wc.KVH * ratio, wc.KVH, hs, max_seq, kv_e4m3=scales is not None,
                                             forms=("rope", "ragged", "step_dev", "paged"), max_pages=max_pages, num_pages=64)
            assert _grid_x(full) == max_seq // C
        assert len(xs) == 1, xs


def test_without_a_window_the_plans_are_the_recorded_ones(built):
    """llmie_decoder_mha_window_plan(window = 0) over the whole grid of tests/golden/decode_attn_plans.txt: byte for byte the lines
    of llmie_decoder_mha_plan"""
    fn = built.lib().llmie_decoder_mha_window_plan
    fn.restype = ctypes.c_char_p

    def plan(*args):
        status = ctypes.c_int(0)
        t = fn(*args, 0, 0, ctypes.addressof(status))
        return (t.decode() if t is not None else None), status.value

    got, exp = plans.recording(plan), plans._fixture()
    assert list(got) == list(exp)
    wrong = [k for k in exp if got[k] != exp[k]]
    assert not wrong, wrong[:10]


# ----------------------------------------------------------------------------------------------------------------- refusals
def test_windowed_forms_without_a_kernel_are_refused(built):
    """fp32, head sizes 32 / 256 and the generic kernel's geometries have no windowed instantiation: an error that says so, never an
    answer that attends to everything"""
    ok = dict(forms=("rope", "ragged", "step_dev"))
    for dtype, hs, nh, kvh, e4m3 in ((built.F32, 128, 8, 2, False), (built.F16, 32, 8, 2, False), (built.F16, 256, 8, 2, False),
                                     (built.F16, 128, 6, 2, False), (built.F16, 80, 8, 8, False), (built.F16, 128, 16, 2, True)):
        text_w, status_w = built.decoder_mha_window_plan(dtype, 2, nh, kvh, hs, 2048, 100, 4, kv_e4m3=e4m3, **ok)
        assert text_w is None and status_w == -2, (dtype, hs, nh, kvh, text_w)
        err = built.lib().llmie_last_error()
        assert (b"window" in err) or (e4m3 and b"fp8 KV" in err), err
    # (unaligned operands fall to the generic kernel, which has no window either)
    text_w, status_w = built.decoder_mha_window_plan(built.F16, 2, 8, 2, 128, 2048, 100, 4, step=300, residues={"k": 2})
    assert text_w is None and status_w == -2 and b"window" in built.lib().llmie_last_error()
    # every windowed geometry is planned
    for hs in (64, 128):
        for ratio in (1, 2, 4, 8):
            for e4m3 in (False, True):
                text_w, status_w = built.decoder_mha_window_plan(built.F16, 2, 2 * ratio, 2, hs, 2048, 100, 4, kv_e4m3=e4m3, **ok)
                assert (status_w == 0) == (not (e4m3 and ratio == 8)), (hs, ratio, e4m3)


def test_bad_window_arguments_fail_before_the_device(built):
    lib = built.lib()
    one = ctypes.c_void_p(16)   # never dereferenced: the checks fail first
    call = lambda window, sinks, batch=1: lib.llmie_decoder_mha_window(one, None, one, one, one, 0, batch, 8, 2, 128, 2048, one, one, 1 << 30,
                                                                       None, 0, None, 0, 0, window, sinks, None, 0, 1.0, 1.0, built.F16, None)
    assert call(-1, 0) == -1 and b"negative" in lib.llmie_last_error()
    assert call(5, -2) == -1 and b"negative" in lib.llmie_last_error()
    assert call(16, 4, batch=0) == -1 and b"bad shape" in lib.llmie_last_error()
    for window, sinks in ((-1, 0), (5, -1)):
        text, status = built.decoder_mha_window_plan(built.F16, 1, 8, 2, 128, 2048, window, sinks, step=7)
        assert text is None and status == -1
    # W = 0 is full attention and the sinks are then ignored: the plan of the unwindowed call
    assert built.decoder_mha_window_plan(built.F16, 1, 8, 2, 128, 2048, 0, 3, step=700) == built.decoder_mha_plan(built.F16, 1, 8, 2, 128, 2048, step=700)
    adv = lambda table, cached, status, batch, max_pages, window, sinks: lib.llmie_kv_window_advance(table, max_pages, cached, None, batch, window,
                                                                                                     sinks, status, None)
    assert adv(None, one, one, 1, 4, 8, 0) == -1 and b"NULL" in lib.llmie_last_error()
    assert adv(one, one, one, 0, 4, 8, 0) == -1 and b"bad shape" in lib.llmie_last_error()
    assert adv(one, one, one, 1, 4, 0, 0) == -1 and b"window >= 1" in lib.llmie_last_error()
    assert adv(one, one, one, 1, 4, 8, -1) == -1


# -------------------------------------------------------------------------------------------------------------- the page ring
def test_the_ring_restatement_keeps_a_sequence_in_the_formulas_pages():
    """wc.ring_advance (the restatement the GPU test holds llmie_kv_window_advance to), one token per step: with exactly
    ring_pages(W, S) pool pages status stays 0, every visible key's page is mapped at every step and no pool page is mapped twice;
    one page less and status 1 comes (if at all) at the first token of a page, for W = 200, S = 4 at the first step that needs the missing
    page (token 384) and not before"""
    for W, S in ((200, 4), (1, 0), (128, 128), (129, 1), (300, 130)):
        pool = wc.ring_pages(W, S)
        for short in (0, 1):
            max_pages = 24
            row = [-1] * max_pages
            free = list(range(pool - short))
            failed = None
            for cached in range(0, max_pages * wc.KV_PAGE):
                p = cached // wc.KV_PAGE
                if row[p] < 0 and free:   # the caller's own pages first
                    row[p] = free.pop(0)
                new, status = wc.ring_advance(row, cached, 1, W, S)
                if status:
                    assert new == row
                    failed = cached
                    break
                row = new
                mapped = [x for x in row if x >= 0]
                assert len(mapped) == len(set(mapped))
                vis = wc.visible(cached + 1, W, S)
                assert all(row[t // wc.KV_PAGE] >= 0 for t in np.flatnonzero(vis))
            if short == 0:
                assert failed is None, (W, S, failed)
            else:
                # (the formula is an upper bound: a window far shorter than a page gets by with less; W = 200, S = 4 does not)
                assert failed is None or failed % wc.KV_PAGE == 0, (W, S, failed)
                assert failed == 3 * wc.KV_PAGE or (W, S) != (200, 4), (W, S, failed)


# ------------------------------------------------------------------------------------------------- prefill and engine restatements
@pytest.mark.parametrize("kv", ["f16", "np2"])
def test_prefill_cases_own_the_mask(kv):
    """the windowed prefill generator: owners inside the mask of their row with >= 0.9 of the visible mass, outside rows that would
    take >= 0.9 (asserted inside; here: that they exist, where they lie, and that W >= every context is the unwindowed reference)"""
    import prefill_attn_cases as pc
    for W, S in ((1, 0), (17, 4), (65, 70), (512, 4)):
        c = wc.make_prefill_case("cpu", 8, 2, wc.PREFILL_LENS, wc.PREFILL_HIST, kv, "q64w4t1", W, S)
        assert len(c.owners) >= 100   # (W = 1, S = 0: one visible key per row, so one owner per KV head and row)
        for (s, i, h), o in c.owners.items():
            qpos = c.hist[s] + i
            assert o.slot <= qpos and (o.slot > qpos - W or o.slot < S)
            for p in c.outside[(s, i, h)]:
                assert p == qpos + 1 or (p <= qpos - W and p >= S)
        n_out = sum(len(v) for v in c.outside.values())
        assert n_out > 50 and len(c.out_mass) == n_out
        full = pc.reference(c, c.deq(c.k_cpu, 0), c.deq(c.v_cpu, 1))
        if W >= max(c.ctx):
            assert all(np.array_equal(a, b) for a, b in zip(c.ref, full))
        else:
            assert max(np.abs(a - b).max() for a, b in zip(c.ref, full)) > 0.1
        dead = wc.prefill_dead_rows(c)
        assert dead.any() == (W < max(c.hist))


def test_window_layer_restatement_without_a_window_is_the_projects():
    import model_param_cases as mpc
    rng = np.random.default_rng(1)
    nh, kvh, hs, inter, lens, hist = 4, 2, 32, 64, [5, 9], [3, 0]
    layers = mpc.draw_layers(rng, nh, kvh, hs, inter, 2)
    cfg = dict(head_num=nh, kv_head_num=kvh, head_size=hs, inter_size=inter, rms_eps=1e-5, rotary_dim=hs, rotary_base=10000.0)
    x = rng.standard_normal((sum(lens), nh * hs))
    k0, v0 = rng.standard_normal((2, 2, 2, kvh, 16, hs))
    ka, va, kb, vb, kc, vc = k0.copy(), v0.copy(), k0.copy(), v0.copy(), k0.copy(), v0.copy()
    a = mpc.layer_restatement(cfg, layers, x, ka, va, lens, hist)
    b = wc.window_layer_restatement(cfg, layers, x, kb, vb, lens, hist, [0, 0], 0)
    c = wc.window_layer_restatement(cfg, layers, x, kc, vc, lens, hist, [3, 0], 1)
    assert np.array_equal(a, b) and np.array_equal(ka, kb) and np.array_equal(va, vb)
    assert np.abs(a - c).max() > 1e-3 and np.array_equal(ka[0], kc[0])   # (layer 0 stores the same rows; its output differs)
