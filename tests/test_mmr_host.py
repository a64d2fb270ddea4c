"""CPU checks of the diversity re-rank (csrc/mmr_rerank.hip): the C ABI surface, the argument errors
that need no device, and the float64 greedy reference the GPU tests judge by (tests/mmr_ref.py) on a table small enough
to work out by hand."""
import pytest
import torch

from carca_replication_amd import CarcaHipError, _lib, catalogue, ops, train
from carca_replication_amd.modules import CARCA, KNN
from tests import mmr_ref as R
from tests.test_knn_catalogue_host import _header_fields


def test_entry_point_declared_and_bound():
    assert "carca_mmr_rerank" in _lib.declared_symbols()
    assert "carca_mmr_rerank" in _lib.SIGNATURES
    assert "mmr_rerank.hip" in _lib.SOURCES
    assert _header_fields("CarcaMmrDesc") == [f[0] for f in _lib.MmrDesc._fields_]
    assert hasattr(CARCA, "recommend_diverse") and hasattr(KNN, "recommend_diverse") and hasattr(ops, "mmr_rerank")
    assert hasattr(train, "evaluate_full_diverse")


def test_abi_version_unchanged():
    assert _lib.load().carca_abi_version() == 3


def test_argument_errors():
    X = torch.randn(10, 8)
    s, i = torch.rand(2, 5), torch.randint(1, 10, (2, 5))
    for lam in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="lam"):
            ops.mmr_rerank(s, i, X, 8, 3, lam=lam)
    with pytest.raises(ValueError, match="l2"):
        ops.mmr_rerank(s, i, X, 8, 3, metric="l2")
    for k in (0, 6):  # k < 1, k > P
        with pytest.raises(CarcaHipError, match="k = "):
            ops.mmr_rerank(s, i, X, 8, k)
    with pytest.raises(CarcaHipError, match="128"):  # P > 128
        ops.mmr_rerank(torch.rand(2, 129), torch.ones(2, 129, dtype=torch.int64), X, 8, 3)
    with pytest.raises(CarcaHipError, match="float32"):
        ops.mmr_rerank(s.double(), i, X, 8, 3)
    with pytest.raises(CarcaHipError, match="integer"):
        ops.mmr_rerank(s, i.float(), X, 8, 3)
    with pytest.raises(CarcaHipError, match="one shape"):
        ops.mmr_rerank(s, i[:, :4], X, 8, 3)
    with pytest.raises(CarcaHipError, match="one shape"):
        ops.mmr_rerank(s[0], i[0], X, 8, 3)
    with pytest.raises(CarcaHipError, match="table"):
        ops.mmr_rerank(s, i, X.double(), 8, 3)
    with pytest.raises(CarcaHipError, match="table"):
        ops.mmr_rerank(s, i, X, 9, 3)  # n_cols past the table's width
    with pytest.raises(CarcaHipError, match="CPU tensor"):
        ops.mmr_rerank(s, i, X, 8, 3)
    # the checks of the model methods that need no device come before the recommend call
    m = KNN()
    p = (torch.ones(2, 3, dtype=torch.int64), None, None)
    with pytest.raises(ValueError, match="lam"):
        m.recommend_diverse(p, lam=2.0)
    with pytest.raises(ValueError, match="metric"):
        m.recommend_diverse(p, metric="euclid")
    with pytest.raises(CarcaHipError, match="k = 11"):
        m.recommend_diverse(p, k=11, pool=10)
    with pytest.raises(CarcaHipError, match="pool size 129"):
        m.recommend_diverse(p, k=5, pool=129)
    with pytest.raises(CarcaHipError, match="register_attr_table"):
        m.recommend_diverse(p)
    with pytest.raises(CarcaHipError, match="candidate"):  # KNN still takes no candidate set
        train.evaluate_full_diverse(m, [], "cpu", 5, candidates=torch.tensor([1, 2]))


# item 0 is padding; 1 = (3, 4), 2 = (6, 8) (parallel to 1), 3 = (-4, 3) (orthogonal to both), 4 = 0; a third, unused column
X5 = torch.tensor([[0.0, 0.0, 9.0], [3.0, 4.0, 9.0], [6.0, 8.0, 9.0], [-4.0, 3.0, 9.0], [0.0, 0.0, 9.0]])


def test_reference_similarities_on_a_hand_made_table():
    ids = torch.tensor([[1, 2, 7, 3, 4]])  # 7 is outside the table: an invalid entry, its row and column read as zeros
    G, valid = R.pool_sims(X5, ids, 2, "cosine")
    assert valid.tolist() == [[True, True, False, True, True]]
    want = torch.tensor([[1.0, 1, 0, 0, 0], [1, 1, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 1, 0], [0, 0, 0, 0, 0]], dtype=torch.float64)
    assert torch.allclose(G[0], want, atol=1e-15)
    assert G[0, 4].tolist() == [0.0] * 5  # an all-zero row: exactly 0 to everything, itself included
    Gd, _ = R.pool_sims(X5, ids, 2, "dot")
    assert Gd[0, 0].tolist() == [25.0, 50.0, 0.0, 0.0, 0.0] and Gd[0, 1, 1] == 100.0 and Gd[0, 3, 3] == 25.0


def test_reference_path_on_a_hand_made_table():
    ids = torch.tensor([[1, 2, 7, 3, 4]])
    s = torch.tensor([[0.9, 0.8, 0.85, 0.5, 0.1]])
    G, valid = R.pool_sims(X5, ids, 2, "cosine")
    # rel over the valid entries (s_min 0.1, s_max 0.9): 1, 0.875, -, 0.5, 0
    rel = R.relevance(s, valid, True)
    assert torch.allclose(rel[0, [0, 1, 3, 4]], torch.tensor([1.0, 0.875, 0.5, 0.0], dtype=torch.float64), atol=1e-7)
    # lam = 1/2.  t0: 0.5 rel -> position 0 (item 1).  M: item 2 -> 1, items 3 and 4 -> 0.
    # t1: item 2 0.4375 - 0.5 = -0.0625; item 3 0.25; item 4 0 -> position 3 (item 3).  t2: item 4 (0) over item 2
    # (-0.0625).  t3: item 2.  The invalid position 2 is never taken although its score is the second best.
    out = R.greedy(G, s, valid, 4, 0.5)
    assert out["pos"].tolist() == [[0, 3, 4, 1]]
    assert out["deficit"].abs().max() == 0
    assert torch.allclose(out["gap"][0, :3], torch.tensor([0.5 - 0.4375, 0.25, 0.0625], dtype=torch.float64), atol=1e-7)
    assert out["gap"][0, 3] == float("inf")
    # ILD: pairs (1,3), (1,4), (3,4), (2,3), (2,4) are at distance 1, the parallel pair (1,2) at 0: 5 / 6
    assert abs(float(out["ild"][0]) - 5.0 / 6.0) < 1e-12
    rs, ri = R.gather_outputs(s, ids, out["pos"])
    assert ri.tolist() == [[1, 3, 4, 2]] and rs.tolist() == [[s[0, 0], s[0, 3], s[0, 4], s[0, 1]]]
    # k beyond the valid entries: position -1, and the outputs pad with (0, 0)
    out5 = R.greedy(G, s, valid, 5, 0.5)
    assert out5["pos"].tolist() == [[0, 3, 4, 1, -1]] and abs(float(out5["ild"][0]) - 5.0 / 6.0) < 1e-12
    rs, ri = R.gather_outputs(s, ids, out5["pos"])
    assert ri[0, 4] == 0 and rs[0, 4] == 0
    # lam = 1: the first k valid entries in pool order; ILD of (1, 2, 3): pairs at 0, 1, 1
    out1 = R.greedy(G, s, valid, 3, 1.0)
    assert out1["pos"].tolist() == [[0, 1, 3]] and abs(float(out1["ild"][0]) - 2.0 / 3.0) < 1e-12
    # lam = 0: at t0 every objective is 0 -> position 0; then pure diversity: item 2 has -1, items 3 and 4 tie at 0 -> the
    # smaller position 3, then 4
    out0 = R.greedy(G, s, valid, 3, 0.0)
    assert out0["pos"].tolist() == [[0, 3, 4]] and out0["gap"][0].tolist() == [0.0, 0.0, 1.0]


def test_reference_ties_go_to_the_smaller_pool_position():
    s = torch.tensor([[1.0, 0.5, 0.5]])
    for ids, want in (([[1, 4, 3]], [[0, 1, 2]]), ([[1, 3, 4]], [[0, 1, 2]])):
        ids = torch.tensor(ids)
        G, valid = R.pool_sims(X5, ids, 2, "cosine")
        # after item 1: rel = 0 and M = 0 for both of items 3 and 4 -> an exact tie, decided by the position, not the id
        out = R.greedy(G, s, valid, 3, 0.5)
        assert out["gap"][0, 1] == 0 and out["pos"].tolist() == want
    # a repeated id is an entry of its own; one score for every entry: rel = 0 everywhere
    ids = torch.tensor([[2, 2, 3]])
    G, valid = R.pool_sims(X5, ids, 2, "cosine")
    flat = torch.tensor([[0.3, 0.3, 0.3]])
    assert R.relevance(flat, valid, True).tolist() == [[0.0, 0.0, 0.0]]
    assert R.relevance(flat, valid, False)[0, 0] == flat.double()[0, 0]
    out = R.greedy(G, flat, valid, 3, 0.5)
    assert out["pos"].tolist() == [[0, 2, 1]]  # the second copy of item 2 (M = 1) after the orthogonal item 3 (M = 0)
    # a forced walk reports how far below the maximum each step was
    w = R.greedy(G, flat, valid, 3, 0.5, forced=torch.tensor([[0, 1, 2]]))
    assert torch.allclose(w["deficit"][0], torch.tensor([0.0, 0.5, 0.0], dtype=torch.float64), atol=1e-12)


def test_integer_reference_agrees_with_the_float64_one():
    g = torch.Generator().manual_seed(5)
    X = (torch.rand(40, 12, generator=g) < 0.4).float()
    X[0] = 0
    X[7] = X[3]
    ids = torch.randint(0, 44, (6, 9), generator=g)
    s = torch.randint(0, 4, (6, 9), generator=g).float()
    pos = R.greedy_int(X, ids, s, 12, 9)
    G, valid = R.pool_sims(X, ids, 12, "dot")
    assert torch.equal(pos, R.greedy(G, s, valid, 9, 0.5, normalize=False)["pos"])
    assert bool(((pos >= 0).sum(1) == valid.sum(1)).all())
    assert R.positions_of(torch.tensor([[3, 0, 9]]), torch.tensor([[9, 3, 5]])).tolist() == [[1, -1, 0]]
    assert R.margin(120) == 4.0 * 128 * 2.0 ** -24
