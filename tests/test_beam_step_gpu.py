"""llmie_beam_step on the GPU against a float64 numpy restatement of the rules in include/llmie.h: parent, token, length and
finished flag exactly, the cumulative log-probability within 1e-4 (the sampler tests' bound on a log-probability).

Inputs: a bulk drawn from N(0, 1) and clipped at 3, per row width + 2 planted head tokens at 6 + 0.25 k (exact in fp16), cum values
on a 1/16 grid.  Every case asserts ON THE REFERENCE that adjacent keys among the first width + 1 candidates of every group differ
by more than 1e-3 -- or tie exactly inside one row, or are the tie the case is about -- so that fp32 against float64 cannot change
an order; SEEDS holds, per case, the first seed for which that holds (found on the CPU with this file's own reference)."""
import numpy as np
import pytest
import torch

DEV = "cuda"
NEG = float("-inf")
GAP = 1e-3
TOL = 1e-4
NP_DT = {"f16": np.float16, "f32": np.float32}

# (kind, vocab, width, groups, dtype, length_penalty) -> seed; cases that are not listed use seed 0
SEEDS = {
    ("mixed", 7, 16, 3, "f16", 0.0): 1, ("mixed", 7, 16, 3, "f32", 0.0): 1, ("mixed", 1000, 16, 1, "f16", 0.0): 2,
    ("mixed", 1000, 16, 1, "f32", 0.0): 2, ("mixed", 1000, 16, 3, "f16", 0.0): 1, ("mixed", 1000, 16, 3, "f32", 0.0): 1,
    ("mixed", 32001, 16, 1, "f16", 0.0): 1, ("mixed", 32001, 16, 1, "f32", 0.0): 1, ("end_id_picked", 1000, 4, 3, "f16", 0.0): 1,
    ("end_id_picked", 1000, 4, 3, "f32", 0.0): 1, ("length_penalty", 32001, 16, 1, "f16", 1.0): 10,
    ("length_penalty", 32001, 16, 1, "f32", 1.0): 10,
}


class Case:
    def __init__(self, logits, cum, gen_len, fin, end_id, lp, allow_ties=False):
        self.logits, self.cum, self.gen_len, self.fin = logits, cum.astype(np.float32), gen_len.astype(np.int32), fin.astype(np.uint8)
        self.end_id, self.lp, self.allow_ties = end_id, lp, allow_ties
        self.groups, self.width = cum.shape
        self.vocab = logits.shape[1]


def _heads(V, W):
    return min(W + 2, max(V - 2, 1))


def _base(rng, V, W, G, dt):
    """live beams everywhere: bulk, planted heads, distinct cum values on the 1/16 grid, unequal lengths"""
    x = np.clip(rng.standard_normal((G * W, V)), -3, 3).astype(np.float32)
    nh = _heads(V, W)
    for r in range(G * W):
        pos = rng.choice(V, nh, replace=False)
        x[r, pos] = 6 + 0.25 * rng.permutation(nh)
    cum = np.stack([-rng.choice(129, W, replace=False) / 16.0 for _ in range(G)])
    gen_len = rng.integers(1, 9, (G, W))
    return x.astype(NP_DT[dt]), cum, gen_len, np.zeros((G, W), np.uint8)


def _top_token(x, r):
    return int(np.argmax(np.where(np.isnan(x[r].astype(np.float64)), -np.inf, x[r].astype(np.float64))))


def make_case(kind, V, W, G, dt, lp, seed):
    rng = np.random.default_rng([seed, V, W, G, len(kind)])
    x, cum, gen_len, fin = _base(rng, V, W, G, dt)
    end_id, ties = V - 1, False
    for r in range(G * W):   # keep end_id out of the heads unless a case puts it there
        if x[r, end_id] >= 6 and kind != "end_id_picked":
            x[r, end_id] = 0.5
    if kind == "first_step":
        for g in range(G):
            x[g * W:(g + 1) * W] = x[g * W]
        cum[:] = NEG
        cum[:, 0] = 0
        gen_len[:] = 0
    elif kind == "mixed":
        if W >= 4:
            fin[:, 1] = 1
            cum[:, 2] = NEG
            cum[:, 3] = np.nan
            fin[:, 3] = rng.integers(0, 2, G)
        if W >= 16:
            fin[:, 9] = 1
            cum[:, 12] = NEG
    elif kind == "all_finished":
        cum = -np.sort(-cum, axis=1)
        fin[:] = 1
    elif kind == "finished_rank":   # beam 1 finished above every live candidate, beam 2 finished below all of them
        cum = np.minimum(cum, -2.0)
        cum[:, 1], fin[:, 1] = -1.0, 1
        cum[:, 2], fin[:, 2] = -100.0, 1
    elif kind == "end_id_picked":   # the best beam's best token is end_id
        best = np.argmax(cum, axis=1)
        g0 = 0
        end_id = _top_token(x, g0 * W + int(best[g0]))
    elif kind == "nan_logits":
        for r in range(G * W):
            x[r, rng.choice(V, max(1, V // 9), replace=False)] = np.nan
            x[r, _top_token(x, r)] = np.nan   # the pick moves to the next head
        x[W - 1] = np.nan                  # a row without any candidate
    elif kind == "tie_rows":           # beams 0 and 1 of every group: the same row bit for bit at the same cum
        ties = True
        for g in range(G):
            x[g * W + 1] = x[g * W]
            cum[g, 1] = cum[g, 0] = cum[g].max() + 1 / 16
    elif kind == "tie_in_row":         # the two best tokens of every row carry the same value
        for r in range(G * W):
            t = _top_token(x, r)
            o = (t + 3) % V
            x[r, o] = x[r, t]
    elif kind == "length_penalty":
        gen_len = rng.integers(1, 40, (G, W))
        cum = cum - 4.0
    else:
        raise KeyError(kind)
    return Case(x, cum, gen_len, fin, end_id, lp, ties)


def reference(c):
    """(parent, token, cum float64, gen_len, finished, sorted candidate lists) by the rules of include/llmie.h, in float64"""
    G, W = c.groups, c.width
    parent, token = np.zeros((G, W), np.int32), np.zeros((G, W), np.int32)
    cum, gen_len, fin = np.zeros((G, W)), np.zeros((G, W), np.int32), np.zeros((G, W), np.uint8)
    lists = []
    for g in range(G):
        cands = []
        for w in range(W):
            cw = float(c.cum[g, w])
            if not cw > NEG:
                continue
            if c.fin[g, w]:
                cands.append([0.0, w, 0, c.end_id, cw, int(c.gen_len[g, w]), 1])
                continue
            x = c.logits[g * W + w].astype(np.float64)
            ok = ~np.isnan(x)
            if not ok.any():
                continue
            m = x[ok].max()
            lse = m + np.log(np.exp(x[ok] - m).sum())
            ids = np.nonzero(ok)[0]
            order = ids[np.lexsort((ids, -x[ids]))][:W]
            for k, v in enumerate(order):
                score = cw + (x[v] - lse)
                if not np.isnan(score):
                    cands.append([0.0, w, k, int(v), score, int(c.gen_len[g, w]) + 1, int(v == c.end_id)])
        for cd in cands:
            cd[0] = cd[4] if c.lp == 0 else cd[4] / float(cd[5]) ** c.lp
        cands.sort(key=lambda cd: (-cd[0], cd[1], cd[2]))
        lists.append(cands)
        for j in range(W):
            if j < len(cands):
                _, w, _, v, score, ln, f = cands[j]
                parent[g, j], token[g, j], cum[g, j], gen_len[g, j], fin[g, j] = g * W + w, v, score, ln, f
            else:
                parent[g, j], token[g, j], cum[g, j], gen_len[g, j], fin[g, j] = g * W + j, c.end_id, NEG, 0, 1
    return parent, token, cum, gen_len, fin, lists


def gaps_ok(c, lists):
    """adjacent keys among the first width + 1 candidates: more than GAP apart, or an exact tie inside one row, or -- where the case
    is about it -- an exact tie between rows"""
    for cands in lists:
        for a, b in zip(cands[:c.width], cands[1:c.width + 1]):
            d = a[0] - b[0]
            if d > GAP or (d == 0 and (a[1] == b[1] or c.allow_ties)):
                continue
            return False
    return True


def build(kind, V, W, G, dt, lp=0.0):
    c = make_case(kind, V, W, G, dt, lp, SEEDS.get((kind, V, W, G, dt, lp), 0))
    ref = reference(c)
    assert gaps_ok(c, ref[5]), "the input's keys are closer than %g: pick another seed" % GAP
    return c, ref


def run(llmie, c, logits=None):
    logits = torch.from_numpy(c.logits).to(DEV) if logits is None else logits
    st = llmie.BeamState(torch.from_numpy(c.cum).to(DEV), torch.from_numpy(c.gen_len).to(DEV), torch.from_numpy(c.fin).to(DEV))
    parent, token = llmie.beam_step(logits, st, c.end_id, c.lp)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (parent, token, st.cum, st.gen_len, st.finished)]


def check(got, ref):
    parent, token, cum, gen_len, fin = got
    assert np.array_equal(parent, ref[0]), (parent, ref[0])
    assert np.array_equal(token, ref[1]), (token, ref[1])
    assert np.array_equal(gen_len, ref[3])
    assert np.array_equal(fin, ref[4])
    dead = np.isneginf(ref[2])
    assert np.array_equal(np.isneginf(cum), dead)
    err = np.abs(cum[~dead].astype(np.float64) - ref[2][~dead])
    print("max |cum - reference| = %.3g" % (err.max() if err.size else 0.0))
    assert (err <= TOL).all(), err.max()


GRID = [(V, W, G, dt) for V in (7, 1000, 32001) for W in (1, 4, 16) for G in (1, 3) for dt in ("f16", "f32")]
SPECIAL = [(1000, 4, 3, "f16"), (1000, 4, 3, "f32"), (32001, 16, 1, "f16"), (32001, 16, 1, "f32")]
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("V,W,G,dt", GRID)
def test_mixed_states(llmie, V, W, G, dt):
    """live, finished and dead (-inf and NaN) beams in one group"""
    c, ref = build("mixed", V, W, G, dt)
    check(run(llmie, c), ref)


@pytest.mark.parametrize("V,W,G,dt", GRID)
def test_first_step(llmie, V, W, G, dt):
    """one live beam per request over identical rows: width distinct tokens, all from beam 0; vocab 7 under width 16 has 7
    candidates and leaves dead slots with the stated fill"""
    c, ref = build("first_step", V, W, G, dt)
    got = run(llmie, c)
    check(got, ref)
    n = min(W, V)
    assert (got[0][:, :n] == (np.arange(G) * W)[:, None]).all()
    assert all(len(set(got[1][g, :n])) == n for g in range(G))
    if V < W:
        assert np.array_equal(got[0][:, V:], (np.arange(G) * W)[:, None] + np.arange(V, W)[None, :]) and (got[1][:, V:] == c.end_id).all()
        assert np.isneginf(got[2][:, V:]).all() and (got[3][:, V:] == 0).all() and (got[4][:, V:] == 1).all()


@pytest.mark.parametrize("V,W,G,dt", SPECIAL)
def test_all_finished(llmie, V, W, G, dt):
    c, ref = build("all_finished", V, W, G, dt)
    got = run(llmie, c)
    check(got, ref)
    assert np.array_equal(got[0], np.arange(G * W).reshape(G, W)) and (got[1] == c.end_id).all()
    assert np.array_equal(got[2], c.cum) and np.array_equal(got[3], c.gen_len) and np.array_equal(got[4], c.fin)


@pytest.mark.parametrize("V,W,G,dt", SPECIAL)
def test_finished_beam_outranks_and_is_pushed_out(llmie, V, W, G, dt):
    c, ref = build("finished_rank", V, W, G, dt)
    assert (ref[0][:, 0] == np.arange(G) * W + 1).all() and (ref[1][:, 0] == c.end_id).all()   # the strong one leads
    assert not (ref[0] == (np.arange(G) * W + 2)[:, None]).any()                                # the weak one is gone
    check(run(llmie, c), ref)


@pytest.mark.parametrize("V,W,G,dt", SPECIAL)
def test_end_id_picked_by_a_live_beam(llmie, V, W, G, dt):
    c, ref = build("end_id_picked", V, W, G, dt)
    assert ref[1][0, 0] == c.end_id and ref[4][0, 0] == 1 and not c.fin.any()
    check(run(llmie, c), ref)


@pytest.mark.parametrize("V,W,G,dt", SPECIAL + [(7, 4, 1, "f16")])
def test_nan_logits(llmie, V, W, G, dt):
    """NaN logits count neither in lse nor in the pick; a row of nothing but NaN has no candidates"""
    c, ref = build("nan_logits", V, W, G, dt)
    if W > 1:
        assert not (ref[0][0] == W - 1).any()
    check(run(llmie, c), ref)


@pytest.mark.parametrize("V,W,G,dt", SPECIAL)
def test_exact_ties(llmie, V, W, G, dt):
    """two bit-identical rows at equal cum: the lower beam first; equal logits inside a row: the lower id first"""
    c, ref = build("tie_rows", V, W, G, dt)
    assert (ref[0][:, 0] == np.arange(G) * W).all() and (ref[0][:, 1] == np.arange(G) * W + 1).all()
    assert (ref[1][:, 0] == ref[1][:, 1]).all()
    check(run(llmie, c), ref)
    c, ref = build("tie_in_row", V, W, G, dt)
    assert (ref[0][:, 0] == ref[0][:, 1]).all() and (ref[1][:, 0] < ref[1][:, 1]).all()
    check(run(llmie, c), ref)


@pytest.mark.parametrize("lp", [0.0, 0.6, 1.0])
@pytest.mark.parametrize("V,W,G,dt", SPECIAL)
def test_length_penalty(llmie, V, W, G, dt, lp):
    c, ref = build("length_penalty", V, W, G, dt, lp)
    if lp:
        c0 = make_case("length_penalty", V, W, G, dt, 0.0, SEEDS.get(("length_penalty", V, W, G, dt, lp), 0))
        assert not np.array_equal(reference(c0)[0][:, 0], ref[0][:, 0]), "the penalty does not change a winner"
    check(run(llmie, c), ref)


@pytest.mark.parametrize("V,W,dt", [(32001, 4, "f16"), (1000, 16, "f32")])
def test_same_bits_again_and_in_another_slot(llmie, V, W, dt):
    """two runs give equal bits; a group moved from slot 0 to slot 2 among other neighbours gives equal bits (at vocab 32001 its
    fp16 rows then lie at other residues of 16 bytes)"""
    a, _ = build("mixed", V, W, 3, dt)
    b = make_case("mixed", V, W, 3, dt, 0.0, 101)
    first, again = run(llmie, a), run(llmie, a)
    for x, y in zip(first, again):
        assert np.array_equal(x, y, equal_nan=True) and x.tobytes() == y.tobytes()
    for arr_b, arr_a in ((b.logits.reshape(3, W, V), a.logits.reshape(3, W, V)), (b.cum, a.cum), (b.gen_len, a.gen_len), (b.fin, a.fin)):
        arr_b[2] = arr_a[0]
    moved = run(llmie, b)
    assert np.array_equal(moved[0][2] - 2 * W, first[0][0])
    for i in range(1, 5):
        assert moved[i][2].tobytes() == first[i][0].tobytes()


def test_graph_replay_reads_the_new_contents(llmie):
    """one capture at vocab 1000, width 4; replayed after logits and state were overwritten it equals the eager call on them"""
    V, W, G = 1000, 4, 3
    a, _ = build("mixed", V, W, G, "f16")
    b, ref_b = build("length_penalty", V, W, G, "f16")
    logits = torch.from_numpy(a.logits).to(DEV)
    st = llmie.BeamState(torch.from_numpy(a.cum).to(DEV), torch.from_numpy(a.gen_len).to(DEV), torch.from_numpy(a.fin).to(DEV))
    out = (torch.zeros((G, W), dtype=torch.int32, device=DEV), torch.zeros((G, W), dtype=torch.int32, device=DEV))
    ws = torch.empty(llmie.beam_step_workspace_bytes(G, W, V), dtype=torch.uint8, device=DEV)
    assert a.end_id == b.end_id and a.lp == b.lp   # (launch arguments: the two cases share them)
    llmie.beam_step(logits, st, a.end_id, a.lp, workspace=ws, out=out)   # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        llmie.beam_step(logits, st, a.end_id, a.lp, workspace=ws, out=out)
    logits.copy_(torch.from_numpy(b.logits))
    st.cum.copy_(torch.from_numpy(b.cum))
    st.gen_len.copy_(torch.from_numpy(b.gen_len))
    st.finished.copy_(torch.from_numpy(b.fin))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.cpu().numpy() for t in (out[0], out[1], st.cum, st.gen_len, st.finished)]
    eager = run(llmie, b)
    for x, y in zip(replayed, eager):
        assert x.tobytes() == y.tobytes()
    check(replayed, ref_b)
