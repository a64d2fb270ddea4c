"""similar_items on the GPU (csrc/similar_items.hip; CARCA.similar_items, KNN.similar_items, ops.similar_rows; DESIGN.md
section 17).  Every case is judged by tests/similar_ref.py: the formula stated in fp64 over the SAME fp32 table rows, read
back from the device; scores within 8 x the fp32 statement's own error + 4 eps32 max|ref64| (the rule of
tests/test_hip_row_kernels.py), ids at every position whose reference neighbours are more than 1e-5 max(1, max|ref64|)
away -- at least 90 % of the positions of each case -- and padding exactly (0, 0.0).  The structure, tie, chunk, candidate
and reproducibility tests compare bits."""
import functools
import pickle

import numpy as np
import pytest
import torch

from carca_replication_amd import CarcaHipError, catalogue, ops
from carca_replication_amd.catalogue import CandidateSet
from carca_replication_amd.modules import KNN
from tests import similar_ref as R
from tests.test_hip_recommend import _setup

pytestmark = pytest.mark.gpu


# ---- tables and references, built once -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _table(n_items, K, pad=0, seed=0):
    """randn [n_items, K] on the CPU (row 0 zero, as every item table's) and its device copy with the row stride
    round_up(K, 4) + pad, every column past K poisoned with NaN: they must not reach a product."""
    g = torch.Generator().manual_seed(1000 * seed + n_items + K)
    X = torch.randn(n_items, K, generator=g)
    X[0] = 0
    ld = (K + 3) // 4 * 4 + pad
    dev = torch.full((n_items, ld), float("nan"))
    dev[:, :K] = X
    return X, dev.cuda()


@functools.lru_cache(maxsize=None)
def _refs(n_items, K, metric, pad=0, seed=0):
    X, _ = _table(n_items, K, pad, seed)
    S64 = R.ref_scores(X, K, metric, torch.float64)
    S32 = R.ref_scores(X, K, metric, torch.float32)
    return S64, R.score_tolerance(S32[1:, 1:], S64[1:, 1:]), float(S64.abs().max())


def _queries(n_items, Q, seed=3):
    """Q query ids: ids 1 and n_items - 1 first, then random ones (duplicates allowed)."""
    rng = np.random.default_rng(seed + Q)
    ids = np.concatenate([np.array([1, n_items - 1])[:min(Q, 2)], rng.integers(1, n_items, size=max(Q - 2, 0))])
    return torch.from_numpy(ids.astype(np.int64))


# ---- 1. op level against the reference --------------------------------------------------------------------------------
# (n_items, K, stride pad, Q, k, metric): K <= 128 runs the query-stationary kernel (64 / 96 / 128 wide), K > 128 the
# streaming one; n_items = 4097 is 256 tiles + 1 item, Q = 65 / 300 more than one query block with a partial last one.
# The last column is the share of positions whose ids are NOT compared, measured with the CPU reference.
OP_CASES = [
    (300, 62, 0, 299, 128, "cosine"),    # 0.011
    (4097, 64, 0, 65, 128, "cosine"),    # 0.023
    (4097, 90, 4, 5, 10, "cosine"),      # 0.000
    (1000, 37, 8, 70, 128, "cosine"),    # 0.017
    (300, 4, 0, 1, 10, "cosine"),        # 0.000
    (300, 96, 0, 300, 1, "cosine"),      # 0.000
    (300, 128, 0, 65, 10, "cosine"),     # 0.000
    (300, 132, 0, 300, 10, "cosine"),    # 0.004
    (300, 4102, 0, 5, 10, "cosine"),     # 0.000 (k = 100 would skip 10.4 %: cosines concentrate at this width)
    (4097, 128, 0, 65, 10, "dot"),       # 0.003
    (300, 4102, 4, 5, 10, "dot"),        # 0.000 (k = 100: 10.4 %, as for cosine)
    (1000, 37, 0, 5, 1, "dot"),          # 0.000
    (300, 96, 4, 65, 128, "dot"),        # 0.028
    (300, 132, 4, 65, 128, "dot"),       # 0.026
    # the streaming loop's edges (csrc/row_stream.h: 4 chunks of 16 columns in flight, chains folded every 16 chunks)
    (300, 192, 0, 65, 10, "dot"),        # 0.003  12 chunks: three unrolled groups, folded only at the end
    (300, 256, 0, 65, 10, "dot"),        # 0.006  exactly one fold, no tail
    (300, 260, 0, 65, 10, "cosine"),     # 0.009  17 chunks: one fold plus a one-chunk tail
    (300, 1028, 0, 65, 10, "dot"),       # 0.018  four folds plus tail
    (77, 132, 0, 70, 10, "dot"),         # 0.000  last workgroup: a 13-row wave and waves without rows; 2nd query block partial
]


@pytest.mark.parametrize("case", OP_CASES, ids=[f"n{c[0]}-K{c[1]}+{c[2]}-Q{c[3]}-k{c[4]}-{c[5]}" for c in OP_CASES])
def test_similar_rows_matches_reference(case):
    n, K, pad, Q, k, metric = case
    _, dev = _table(n, K, pad)
    S64, tol, scale = _refs(n, K, metric, pad)
    items = _queries(n, Q)
    ws, wi, full, _ = R.ref_topk(S64, items.tolist(), k)
    got = ops.similar_rows(dev, K, items.cuda(), k, metric)
    R.check(got, (ws, wi), full, k, tol, scale)


# ---- 2. structure, bit-exact ------------------------------------------------------------------------------------------
def test_two_item_catalogue_is_all_padding():
    _, dev = _table(2, 64)
    s, i = ops.similar_rows(dev, 64, torch.tensor([1, 1, 0]).cuda(), 5)
    assert s.shape == (3, 5) and not bool(s.any()) and not bool(i.any())
    s, i = ops.similar_rows(dev, 64, torch.tensor([1]).cuda(), 5, exclude_self=False)  # item 1 is its own only neighbour
    assert i.cpu().tolist() == [[1, 0, 0, 0, 0]] and not bool(s[0, 1:].any()) and abs(float(s[0, 0]) - 1.0) < 1e-6


@pytest.mark.parametrize("K", [62, 132])
def test_padding_invalid_and_duplicate_queries(K):
    n = 40
    _, dev = _table(n, K)
    S64, tol, scale = _refs(n, K, "cosine")
    items = torch.tensor([5, 0, -1, n, 5, 7, 2 ** 40 + 5, n - 1])
    k = 64  # 38 eligible items: positions 38 .. 63 are padding
    got = ops.similar_rows(dev, K, items.cuda(), k)
    ws, wi, full, _ = R.ref_topk(S64, items.tolist(), k)
    R.check(got, (ws, wi), full, k, tol, scale)
    s, i = got[0].cpu(), got[1].cpu()
    for row in (1, 2, 3, 6):  # ids outside [1, n_items): fully padded
        assert not bool(s[row].any()) and not bool(i[row].any())
    assert torch.equal(s[0], s[4]) and torch.equal(i[0], i[4])  # duplicates give identical rows
    assert int((i[0] != 0).sum()) == n - 2 and 5 not in i[0].tolist()


def test_no_queries():
    _, dev = _table(300, 62)
    s, i = ops.similar_rows(dev, 62, torch.zeros(0, dtype=torch.int64).cuda(), 7)
    assert s.shape == (0, 7) and i.shape == (0, 7) and s.dtype == torch.float32 and i.dtype == torch.int64 and s.is_cuda


@pytest.mark.parametrize("K", [90, 132])
def test_items_none_is_every_item(K):
    n = 300
    _, dev = _table(n, K)
    a = ops.similar_rows(dev, K, None, 10)
    b = ops.similar_rows(dev, K, torch.arange(n).cuda(), 10)
    assert a[0].shape == (n, 10) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not bool(a[0][0].any()) and not bool(a[1][0].any())  # row 0: padding
    S64, tol, scale = _refs(n, K, "cosine")
    ws, wi, full, _ = R.ref_topk(S64, list(range(n)), 10)
    R.check(a, (ws, wi), full, 10, tol, scale)


@pytest.mark.parametrize("K", [64, 4102])
def test_query_first_without_exclude_self(K):
    n = 300
    _, dev = _table(n, K)
    S64, tol, scale = _refs(n, K, "cosine")
    items = _queries(n, 20)
    s, i = ops.similar_rows(dev, K, items.cuda(), 5, "cosine", exclude_self=False)
    assert torch.equal(i[:, 0].cpu(), items)
    assert float((s[:, 0].cpu().double() - 1.0).abs().max()) <= tol
    ws, wi, full, _ = R.ref_topk(S64, items.tolist(), 5, exclude_self=False)
    R.check((s, i), (ws, wi), full, 5, tol, scale)


@pytest.mark.parametrize("K", [37, 132])
def test_all_zero_row_scores_exactly_zero(K):
    n = 50
    X, dev = _table(n, K)
    dev = dev.clone()
    dev[[7, 20], :K] = 0
    s, i = ops.similar_rows(dev, K, torch.tensor([7, 3]).cuda(), n - 2)
    s, i = s.cpu(), i.cpu()
    assert not bool(s[0].any()) and i[0].tolist() == [j for j in range(1, n) if j != 7]  # eligible, all tied at 0: id order
    at = i[1].tolist()
    assert float(s[1, at.index(7)]) == 0.0 and float(s[1, at.index(20)]) == 0.0 and at.index(7) < at.index(20)


# ---- 3. ties ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,metric", [(64, "cosine"), (90, "dot"), (132, "cosine")])
def test_duplicate_rows_tie_to_the_smaller_id(K, metric):
    n, base = 301, 120
    g = torch.Generator().manual_seed(5)
    rows = torch.randn(base, K, generator=g)
    owner = torch.cat([torch.arange(base), torch.arange(base), torch.arange(60)])  # every row twice, half of them thrice
    owner = owner[torch.randperm(owner.numel(), generator=g)]
    X = torch.zeros(n, K)
    X[1:] = rows[owner]
    ld = (K + 3) // 4 * 4
    dev = torch.zeros(n, ld)
    dev[:, :K] = X
    dev = dev.cuda()
    S64, S32 = R.ref_scores(X, K, metric, torch.float64), R.ref_scores(X, K, metric, torch.float32)
    tol, scale = R.score_tolerance(S32[1:, 1:], S64[1:, 1:]), float(S64.abs().max())
    items = torch.arange(1, n)
    for k in (128, 7):
        s, i = ops.similar_rows(dev, K, items.cuda(), k, metric)
        ws, wi, full, _ = R.ref_topk(S64, items.tolist(), k)
        R.check((s, i), (ws, wi), full, k, tol, scale, ties=True)
        s, i = s.cpu(), i.cpu()
        grp = owner[i - 1]  # the row behind each returned id
        same = grp[:, 1:] == grp[:, :-1]
        assert bool(same.any())
        assert torch.equal(s[:, 1:][same], s[:, :-1][same])  # duplicates score bit-identically
        assert bool((i[:, 1:][same] > i[:, :-1][same]).all())  # and list by ascending id inside their group


# ---- 4. chunks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,cands", [(62, False), (132, False), (90, True)])
def test_chunked_call_equals_one_chunk(K, cands):
    n, Q = 300, 150
    _, dev = _table(n, K)
    items = _queries(n, Q).cuda()
    S = CandidateSet(torch.arange(1, n), n, device="cuda") if cands else None
    C = n - 1 if cands else n
    budget = 4 * 64 * C + 100  # 64 rows fit, 128 do not: chunks of 64, 64 and 22 queries
    assert catalogue.similar_chunk_rows(budget, C) == 64 and len(catalogue.similar_chunks(Q, 64)) == 3
    one = ops.similar_rows(dev, K, items, 20, candidates=S)
    three = ops.similar_rows(dev, K, items, 20, candidates=S, max_scratch_bytes=budget)
    assert torch.equal(one[0], three[0]) and torch.equal(one[1], three[1])
    tiny = ops.similar_rows(dev, K, items, 20, candidates=S, max_scratch_bytes=1)  # below one block: still 64 at a time
    assert torch.equal(one[0], tiny[0]) and torch.equal(one[1], tiny[1])


# ---- 5. candidates ---------------------------------------------------------------------------------------------------
def _draw(n_items, c, seed=11):
    rng = np.random.default_rng(seed + c)
    forced = [n_items - 1, 1][:min(2, c)]
    rest = rng.choice(np.arange(2, n_items - 1), size=c - len(forced), replace=False)
    ids = np.concatenate([np.array(forced, dtype=np.int64), rest.astype(np.int64)])
    rng.shuffle(ids)
    return torch.from_numpy(ids)


@pytest.mark.parametrize("K,metric", [(62, "cosine"), (132, "dot")])
@pytest.mark.parametrize("c", [1, 40, 256, 257])
def test_candidates_match_reference_and_unrestricted_bits(K, metric, c):
    n, k = 300, 128
    _, dev = _table(n, K)
    S64, tol, scale = _refs(n, K, metric)
    S = _draw(n, c)
    items = _queries(n, 70)  # most queries lie outside a small S
    assert not set(items.tolist()) <= set(S.tolist())
    cs = CandidateSet(S, n, device="cuda")
    got = ops.similar_rows(dev, K, items.cuda(), k, metric, candidates=cs)
    ws, wi, full, _ = R.ref_topk(S64, items.tolist(), k, allowed=S.tolist())
    R.check(got, (ws, wi), full, k, tol, scale)
    assert set(got[1].cpu().reshape(-1).tolist()) <= set(S.tolist()) | {0}
    raw = ops.similar_rows(dev, K, items.cuda(), k, metric, candidates=S.cuda())  # a raw tensor builds the same set
    assert torch.equal(raw[0], got[0]) and torch.equal(raw[1], got[1])
    mask = torch.zeros(n, dtype=torch.bool)
    mask[S] = True
    raw = ops.similar_rows(dev, K, items.cuda(), k, metric, candidates=mask.cuda())
    assert torch.equal(raw[0], got[0]) and torch.equal(raw[1], got[1])


@pytest.mark.parametrize("K,metric", [(62, "cosine"), (90, "dot"), (132, "cosine")])
def test_candidate_scores_are_the_unrestricted_bits(K, metric):
    """On a catalogue of 120 items the unrestricted call with k = 128 lists every eligible item, so every (query, id) pair
    returned under a set S has its unrestricted score to compare with: the same bits."""
    n, k = 120, 128
    _, dev = _table(n, K)
    items = _queries(n, 70).cuda()
    fs, fi = ops.similar_rows(dev, K, items, k, metric)
    fs, fi = fs.cpu(), fi.cpu()
    for c in (1, 40, 100):
        S = _draw(n, c)
        gs, gi = ops.similar_rows(dev, K, items, k, metric, candidates=CandidateSet(S, n, device="cuda"))
        gs, gi = gs.cpu(), gi.cpu()
        for q in range(items.numel()):
            where = {int(i): j for j, i in enumerate(fi[q].tolist()) if i}
            want = sorted(set(S.tolist()) - {int(items[q])})
            assert sorted(i for i in gi[q].tolist() if i) == want
            for j, i in enumerate(gi[q].tolist()):
                if i:
                    assert gs[q, j].view(torch.int32) == fs[q, where[i]].view(torch.int32)


@pytest.mark.parametrize("K", [64, 132])
def test_every_item_as_candidates_equals_none(K):
    n = 300
    _, dev = _table(n, K)
    items = _queries(n, 70).cuda()
    for metric in ("cosine", "dot"):
        a = ops.similar_rows(dev, K, items, 128, metric)
        b = ops.similar_rows(dev, K, items, 128, metric, candidates=torch.arange(1, n).cuda())
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_empty_candidate_set():
    _, dev = _table(300, 62)
    s, i = ops.similar_rows(dev, 62, _queries(300, 5).cuda(), 4, candidates=CandidateSet(torch.tensor([0, 300]), 300, device="cuda"))
    assert s.shape == (5, 4) and not bool(s.any()) and not bool(i.any())


# ---- 6. models -------------------------------------------------------------------------------------------------------
# (d, H, embedding)
MODEL_CASES = [(64, 2, "all"), (90, 3, "attrctx"), (128, 4, "id"), (62, 2, "mlpid")]


@functools.lru_cache(maxsize=None)
def _model(d, H, emb):
    n_ctx = 6 if emb in ("all", "attrctx") else 0
    return _setup(d, H, emb, "ca", "identity", True, 16, 3, 300, n_ctx, 1)[4]


@pytest.mark.parametrize("case", MODEL_CASES, ids=[f"{c[0]}x{c[1]}-{c[2]}" for c in MODEL_CASES])
def test_model_similar_items(case):
    d, H, emb = case
    model = _model(d, H, emb)
    n = 300
    items = _queries(n, 70).cuda()
    T = model.embeds.item_table()
    assert T.shape[0] == n
    for metric, k in (("cosine", 128), ("dot", 10)):
        got = model.similar_items(items, k, metric)
        op = ops.similar_rows(T, d, items, k, metric)
        assert torch.equal(got[0], op[0]) and torch.equal(got[1], op[1])
        X = T[:, :d].cpu()
        S64, S32 = R.ref_scores(X, d, metric, torch.float64), R.ref_scores(X, d, metric, torch.float32)
        ws, wi, full, _ = R.ref_topk(S64, items.tolist(), k)
        R.check(got, (ws, wi), full, k, R.score_tolerance(S32[1:, 1:], S64[1:, 1:]), float(S64.abs().max()))
    again = model.similar_items(items, 128, "cosine")
    model.train()  # no dropout site in the item table: the same bits in training mode
    try:
        tr = model.similar_items(items, 128, "cosine")
    finally:
        model.eval()
    ev = model.similar_items(items, 128, "cosine")
    assert torch.equal(tr[0], ev[0]) and torch.equal(tr[1], ev[1]) and torch.equal(again[0], ev[0])
    allq = model.similar_items(None, 3)
    assert allq[0].shape == (n, 3) and not bool(allq[1][0].any())


def test_model_follows_an_optimizer_step_and_pickles_without_caches():
    model = _setup(64, 2, "id", "dot", "identity", True, 16, 3, 300, 0, 1, seed=3)[4]
    items = _queries(300, 20).cuda()
    before = model.similar_items(items, 10)
    assert "_item_rnorm_cache" in model.embeds.__dict__
    r0 = model.embeds.__dict__["_item_rnorm_cache"][1]
    assert model.similar_items(items, 10)[0] is not None and model.embeds.__dict__["_item_rnorm_cache"][1] is r0  # cached
    opt = torch.optim.SGD(model.parameters(), lr=0.5)
    E = model.embeds.items_embed.weight
    g = torch.Generator().manual_seed(9)
    E.grad = torch.randn(E.shape, generator=g).cuda()
    opt.step()
    after = model.similar_items(items, 10)
    assert model.embeds.__dict__["_item_rnorm_cache"][1] is not r0
    assert not torch.equal(before[1], after[1])
    T = model.embeds.item_table()
    op = ops.similar_rows(T, 64, items, 10)  # norms computed afresh from the new table
    assert torch.equal(after[0], op[0]) and torch.equal(after[1], op[1])
    blob = pickle.dumps(model)
    state = model.embeds.__getstate__()
    assert "_item_rnorm_cache" not in state and "_item_table_cache" not in state
    clone = pickle.loads(blob)
    assert "_item_rnorm_cache" not in clone.embeds.__dict__
    again = clone.cuda().eval().similar_items(items, 10)
    assert torch.equal(again[0], after[0]) and torch.equal(again[1], after[1])


def test_attribute_embedding_needs_its_table():
    model = _setup(64, 2, "all", "ca", "identity", True, 16, 3, 300, 6, 1)[4]
    model.embeds.register_attr_table(None)
    with pytest.raises(CarcaHipError, match="register_attr_table"):
        model.similar_items(torch.tensor([1]).cuda(), 3)


@pytest.mark.parametrize("F,kind", [(32, "multihot"), (37, "multihot"), (37, "random"), (4102, "multihot"), (4102, "random")])
def test_knn_similar_items_agrees_with_recommend(F, kind):
    n, k = 300, 20
    g = torch.Generator().manual_seed(F)
    A = (torch.rand(n, F, generator=g) < 0.1).float() if kind == "multihot" else torch.randn(n, F, generator=g)
    A[0] = 0
    knn = KNN()
    knn.register_attr_table(A.cuda())
    ids = _queries(n, 40).cuda()
    got = knn.similar_items(ids, k, "dot", exclude_self=False)
    rs, ri = knn.recommend((ids[:, None], None, None), None, k, exclude=None)
    S64, S32 = R.ref_scores(A, F, "dot", torch.float64), R.ref_scores(A, F, "dot", torch.float32)
    tol, scale = R.score_tolerance(S32[1:, 1:], S64[1:, 1:]), float(S64.abs().max())
    assert float((got[0] - rs).abs().max()) <= 2 * tol  # both within tol of the reference
    _, _, full, _ = R.ref_topk(S64, ids.tolist(), k, exclude_self=False)
    # unambiguous positions: a multi-hot table's integer scores tie exactly, in the reference and (exact sums) in both
    # calls, and exact ties go to the smaller id in both; measured share of compared positions 0.98 .. 1.00
    clear = R.clear_positions(full, k, scale, ties=True)
    gi, ri = got[1].cpu(), ri.cpu()
    for q, c in enumerate(clear):
        assert torch.equal(gi[q][c], ri[q][c])
    assert R.compared_share(clear) >= 0.9
    # and against the reference itself, cosine included (the cached norms)
    for metric in ("dot", "cosine"):
        S64, S32 = R.ref_scores(A, F, metric, torch.float64), R.ref_scores(A, F, metric, torch.float32)
        ws, wi, full, _ = R.ref_topk(S64, ids.tolist(), k)
        R.check(knn.similar_items(ids, k, metric), (ws, wi), full, k, R.score_tolerance(S32[1:, 1:], S64[1:, 1:]),
                float(S64.abs().max()), ties=True)
    assert knn.__dict__["_similar_cache"][2]["rnorm"] is not None
    pickle.dumps(knn)


@pytest.mark.parametrize("F,kind", [(37, "random"), (256, "random"), (260, "random"), (4102, "random"), (64, "multihot")])
def test_knn_similar_items_has_recommend_bits(F, kind):
    """With the query's own row kept and no exclusion the two calls return the same bits.  F = 256 / 260 / 4102: both run
    one kernel (csrc/row_stream.h) with aligned loads, at one fold, one fold plus a tail and many folds.  F = 37:
    recommend's unaligned loads against similar_items' query-stationary kernel over a zero-padded copy of the table (one
    chain in the same order).  The multi-hot table: recommend's int8 products against fp32 ones (exact integer sums)."""
    n, k = 300, 20
    g = torch.Generator().manual_seed(F)
    A = (torch.rand(n, F, generator=g) < 0.1).float() if kind == "multihot" else torch.randn(n, F, generator=g)
    A[0] = 0
    knn = KNN()
    knn.register_attr_table(A.cuda())
    ids = _queries(n, 40).cuda()
    ss, si = knn.similar_items(ids, k, "dot", exclude_self=False)
    rs, ri = knn.recommend((ids[:, None], None, None), None, k, exclude=None)
    assert torch.equal(ss, rs) and torch.equal(si, ri)


# ---- 7. reproducibility -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [90, 4102])
def test_two_calls_give_the_same_bits(K):
    n = 300
    _, dev = _table(n, K)
    items = _queries(n, 65).cuda()
    for metric in ("cosine", "dot"):
        a = ops.similar_rows(dev, K, items, 128, metric)
        b = ops.similar_rows(dev, K, items, 128, metric)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # a pair's bits do not depend on the query's position or on Q
    a = ops.similar_rows(dev, K, items, 128)
    b = ops.similar_rows(dev, K, items.flip(0)[:7], 128)
    assert torch.equal(a[0].flip(0)[:7], b[0]) and torch.equal(a[1].flip(0)[:7], b[1])
