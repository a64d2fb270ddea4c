"""CPU checks of similar_items (csrc/similar_items.hip): the C ABI surface, the chunk arithmetic, the
argument errors that need no device, and the fp64 reference the GPU tests judge by (tests/similar_ref.py) on a table small
enough to work out by hand."""
import pytest
import torch

from carca_replication_amd import CarcaHipError, _lib, catalogue, ops
from carca_replication_amd.catalogue import CandidateSet
from carca_replication_amd.modules import CARCA, KNN
from tests import similar_ref as R
from tests.test_knn_catalogue_host import _header_fields


def test_entry_points_declared_and_bound():
    for name in ("carca_similar_items", "carca_row_rnorm"):
        assert name in _lib.declared_symbols()
        assert name in _lib.SIGNATURES
    assert "similar_items.hip" in _lib.SOURCES
    assert hasattr(CARCA, "similar_items") and hasattr(KNN, "similar_items") and hasattr(ops, "similar_rows")
    assert _header_fields("CarcaSimilarDesc") == [f[0] for f in _lib.SimilarDesc._fields_]


def test_abi_version_unchanged():
    assert _lib.load().carca_abi_version() == 3


@pytest.mark.parametrize("budget", [0, 1, 4 * 64 * 300 - 1, 4 * 64 * 300, 50_000, 150_000, 1 << 20, 1 << 30])
@pytest.mark.parametrize("C", [1, 40, 300, 4097, 1_000_001])
def test_chunk_rows(budget, C):
    qc = catalogue.similar_chunk_rows(budget, C)
    assert qc % 64 == 0 and qc >= 64
    if budget >= 4 * 64 * C:  # the budget allows one block: the buffer stays within it, and one more block would not
        assert qc * C * 4 <= budget < (qc + 64) * C * 4
    else:
        assert qc == 64


def test_chunk_slices():
    assert catalogue.similar_chunks(150, 64) == [(0, 64), (64, 128), (128, 150)]  # a partial last chunk
    assert catalogue.similar_chunks(128, 64) == [(0, 64), (64, 128)]
    assert catalogue.similar_chunks(1, 64) == [(0, 1)]
    assert catalogue.similar_chunks(0, 64) == []
    # the GPU chunk test's numbers: C = 300, Q = 150 and a budget that holds 64 rows but not 128
    assert catalogue.similar_chunk_rows(100_000, 300) == 64
    for Q, qc in ((1000, 192), (4097, 64), (65, 128)):
        sl = catalogue.similar_chunks(Q, qc)
        assert sl[0][0] == 0 and sl[-1][1] == Q and all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
        assert all(0 < hi - lo <= qc for lo, hi in sl) and all(hi - lo == qc for lo, hi in sl[:-1])


def test_argument_errors():
    X = torch.randn(10, 8)
    ids = torch.tensor([1, 2])
    for k in (0, 129):
        with pytest.raises(CarcaHipError, match="128"):
            ops.similar_rows(X, 8, ids, k)
    with pytest.raises(ValueError, match="l2"):
        ops.similar_rows(X, 8, ids, 3, "l2")
    with pytest.raises(CarcaHipError, match="items"):
        ops.similar_rows(X, 8, ids.float(), 3)
    with pytest.raises(CarcaHipError, match="items"):
        ops.similar_rows(X, 8, ids.view(1, 2), 3)
    with pytest.raises(CarcaHipError, match="n_items = 11"):
        ops.similar_rows(X, 8, ids, 3, candidates=CandidateSet(torch.tensor([1, 2]), 11))
    with pytest.raises(CarcaHipError, match="CPU tensor"):
        ops.similar_rows(X, 8, ids, 3)
    with pytest.raises(CarcaHipError, match="CPU tensor"):
        ops.similar_rows(X, 8, None, 3, "dot", candidates=CandidateSet(torch.tensor([1, 2]), 10))
    m = KNN()
    with pytest.raises(CarcaHipError, match="register_attr_table"):
        m.similar_items(ids, 3)
    with pytest.raises(ValueError):
        m.similar_items(ids, 3, metric="euclid")


def test_knn_cache_follows_the_table_and_stays_out_of_pickles():
    m = KNN()
    m.register_attr_table(torch.ones(4, 6))
    c = m._similar_tables()
    assert c["rows"].shape == (4, 8) and torch.equal(c["rows"][:, :6], m._attr_table) and not bool(c["rows"][:, 6:].any())
    assert m._similar_tables() is c  # cached
    m._attr_table[1, 2] = 0.5  # an in-place change bumps _version
    c2 = m._similar_tables()
    assert c2 is not c and float(c2["rows"][1, 2]) == 0.5
    assert "_similar_cache" not in m.__getstate__()
    m.register_attr_table(torch.ones(4, 8))
    assert m._similar_tables()["rows"] is m._attr_table  # F % 4 == 0: no copy


def test_reference_on_a_hand_made_table():
    # item 0 is padding; 1 = (3, 4), 2 = (6, 8) (parallel to 1), 3 = (-4, 3) (orthogonal to 1), 4 = 0; a third, unused column
    X = torch.tensor([[0.0, 0.0, 9.0], [3.0, 4.0, 9.0], [6.0, 8.0, 9.0], [-4.0, 3.0, 9.0], [0.0, 0.0, 9.0]])
    for dtype in (torch.float32, torch.float64):
        dot = R.ref_scores(X, 2, "dot", dtype)
        assert dot.dtype == dtype
        assert dot[1].tolist() == [0.0, 25.0, 50.0, 0.0, 0.0] and dot[2, 2] == 100.0 and dot[3, 2] == 0.0
        cos = R.ref_scores(X, 2, "cosine", dtype)
        assert torch.allclose(cos[1], torch.tensor([0.0, 1.0, 1.0, 0.0, 0.0], dtype=dtype), atol=1e-6)
        assert cos[4].tolist() == [0.0] * 5  # an all-zero row scores exactly 0, against everything
    S = R.ref_scores(X, 2, "dot", torch.float64)
    s, i, full, order = R.ref_topk(S, [1, 1, 0, 5, -1, 4], 3)
    assert i[0].tolist() == [2, 3, 4] and s[0].tolist() == [50.0, 0.0, 0.0]  # the tie at 0 goes to the smaller id
    assert torch.equal(i[1], i[0]) and i[2].tolist() == [0, 0, 0] and i[3].tolist() == [0, 0, 0] and i[4].tolist() == [0, 0, 0]
    assert i[5].tolist() == [1, 2, 3] and s[5].tolist() == [0.0, 0.0, 0.0]
    assert full[0].tolist() == [50.0, 0.0, 0.0] and order[0].tolist() == [2, 3, 4] and full[2].numel() == 0
    s, i, _, _ = R.ref_topk(S, [1], 4, exclude_self=False)
    assert i[0].tolist() == [2, 1, 3, 4] and s[0].tolist() == [50.0, 25.0, 0.0, 0.0]
    s, i, full, _ = R.ref_topk(S, [1, 2], 3, allowed=[4, 2, 0, 9])  # the complement of S excluded; the query need not be in S
    assert i.tolist() == [[2, 4, 0], [4, 0, 0]] and s[0].tolist() == [50.0, 0.0, 0.0] and full[1].tolist() == [0.0]
    # clear positions: 50 stands apart; the two zeros tie exactly -- compared only where exact ties are the reference's own
    _, _, full, _ = R.ref_topk(S, [1], 3)
    assert R.clear_positions(full, 3, 50.0)[0].tolist() == [True, False, False]
    assert R.clear_positions(full, 3, 50.0, ties=True)[0].tolist() == [True, True, True]
    assert R.clear_positions(full, 2, 50.0)[0].tolist() == [True, False]  # the neighbour past k counts
    assert R.score_tolerance(S.float(), S) == 4.0 * R.EPS32 * 100.0
