"""CPU checks of the candidate-set restriction of CARCA.recommend / rank_items:
catalogue.CandidateSet's normalisation and errors, and the C ABI surface of carca_recommend_among /
carca_rank_items_among (declared, exported, bound; the ctypes struct matching the header)."""
import ctypes as C
import inspect

import pytest
import torch

from carca_replication_amd import CarcaHipError, _lib, catalogue
from carca_replication_amd.catalogue import CandidateSet
from carca_replication_amd.modules import CARCA, KNN
from tests.test_knn_catalogue_host import _header_fields


def test_normalisation_of_an_id_list():
    S = CandidateSet(torch.tensor([7, 3, 3, 0, -2, 19, 20, 25, 1, 7], dtype=torch.int64), 20)
    assert S.ids.dtype == torch.int32 and S.ids.device.type == "cpu" and S.ids.is_contiguous()
    assert S.ids.tolist() == [1, 3, 7, 19]  # sorted, distinct, inside [1, n_items)
    assert S.n_items == 20 and len(S) == 4
    # an int64 id that would wrap into range as int32 is dropped, not wrapped
    assert CandidateSet(torch.tensor([2 ** 32 + 5, 5]), 20).ids.tolist() == [5]
    # int32 input
    assert CandidateSet(torch.tensor([4, 2], dtype=torch.int32), 20).ids.tolist() == [2, 4]


def test_mask_equals_ids():
    g = torch.Generator().manual_seed(0)
    mask = torch.rand(50, generator=g) < 0.3
    mask[0] = True  # the padding item is never a candidate
    ids = torch.nonzero(mask).reshape(-1)
    a, b = CandidateSet(mask, 50), CandidateSet(ids.flip(0), 50)
    assert torch.equal(a.ids, b.ids) and a.ids.dtype == torch.int32
    assert 0 not in a.ids.tolist() and len(a) == int(mask[1:].sum())


def test_empty_set():
    for items in (torch.zeros(0, dtype=torch.int64), torch.tensor([0, -1, 30]), torch.zeros(30, dtype=torch.bool)):
        S = CandidateSet(items, 30)
        assert len(S) == 0 and S.ids.shape == (0,) and S.ids.dtype == torch.int32
        assert S.contains(torch.tensor([[0, 1, 29]])).tolist() == [[False, False, False]]


def test_contains():
    S = CandidateSet(torch.tensor([2, 5, 9]), 10)
    q = torch.tensor([[0, 2, 3], [9, 10, -1], [5, 2 ** 40, 1]])
    assert S.contains(q).tolist() == [[False, True, False], [True, False, False], [True, False, False]]


def test_errors():
    with pytest.raises(CarcaHipError, match="integer"):
        CandidateSet(torch.tensor([1.0, 2.0]), 10)
    with pytest.raises(CarcaHipError, match="1-D"):
        CandidateSet(torch.tensor([[1, 2], [3, 4]]), 10)
    with pytest.raises(CarcaHipError, match="mask"):
        CandidateSet(torch.zeros(9, dtype=torch.bool), 10)
    with pytest.raises(CarcaHipError, match="1-D"):
        CandidateSet([1, 2, 3], 10)
    # a set built for another catalogue, and a bad raw argument, at the call (before anything touches a device)
    D = _lib.RecommendDesc()
    D.n_items = 20
    with pytest.raises(CarcaHipError, match="n_items = 10"):
        catalogue._candidates("recommend", CandidateSet(torch.tensor([1, 2]), 10), D, [], "cpu")
    for bad in (torch.tensor([1.0]), torch.tensor([[1, 2]]), torch.zeros(19, dtype=torch.bool)):
        with pytest.raises(CarcaHipError):
            catalogue._candidates("recommend", bad, D, [], "cpu")
    with pytest.raises(CarcaHipError, match="candidates"):
        catalogue._candidates("recommend", [1, 2], D, [], "cpu")
    assert catalogue._candidates("recommend", None, D, [], "cpu") is None


def test_entry_points_declared_exported_and_bound():
    lib = _lib.load()
    for name in ("carca_recommend_among", "carca_rank_items_among"):
        assert name in _lib.declared_symbols()
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    assert _lib.SIGNATURES["carca_recommend_among"][1][1] is C.POINTER(_lib.Candidates)
    assert lib.carca_abi_version() == 3
    for fn in (CARCA.recommend, CARCA.rank_items):
        assert inspect.signature(fn).parameters["candidates"].default is None
    for fn in (KNN.recommend, KNN.rank_items):  # out of scope: the KNN calls take no candidate set
        assert "candidates" not in inspect.signature(fn).parameters


def test_ctypes_struct_matches_header():
    assert _header_fields("CarcaCandidates") == [f[0] for f in _lib.Candidates._fields_]
    assert C.sizeof(_lib.Candidates) == 16 and _lib.Candidates.n.offset == 8


def test_evaluators_take_candidates_and_refuse_models_without_them():
    from carca_replication_amd import train

    for fn in (train.evaluate_full, train.evaluate_full_ranks):
        assert inspect.signature(fn).parameters["candidates"].default is None
    with pytest.raises(CarcaHipError, match="KNN"):
        train._candidate_set(KNN(), "rank_items", torch.tensor([1, 2]), "cpu")
    assert train._candidate_set(KNN(), "rank_items", None, "cpu") is None
