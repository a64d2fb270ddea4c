"""catalogue.ModelSide, the part that needs no GPU: desc() sets exactly the model-side fields of the
descriptor class it is asked for, leaves every other field zero or null, and refuses a class of the other model."""
import ctypes as C

import pytest

from carca_replication_amd import CarcaHipError, _lib
from carca_replication_amd.catalogue import ModelSide

EXCLUSION = ("exclude", "n_exclude", "ld_exclude")
CARCA_FIELDS = ("B", "L", "n_items", "d", "H") + tuple(n for n, _ in _lib._CARCA_MODEL if n not in EXCLUSION)
KNN_FIELDS = ("B", "L", "n_items", "F") + tuple(n for n, _ in _lib._KNN_MODEL if n not in EXCLUSION)


def _made_up(cls, names):
    """name -> a value no other name has: a large one for a pointer field, a small one for the rest."""
    types = dict(cls._fields_)
    return {n: (0x7F0000001000 + 0x1000 * i if types[n] is C.c_void_p else 3 + i) for i, n in enumerate(names)}


def _check(side, cls, values):
    D = side.desc(cls)
    assert isinstance(D, cls)
    for name, _ in cls._fields_:
        got = getattr(D, name)
        if name in values:
            assert got == values[name], (cls.__name__, name)
        else:
            assert not got, (cls.__name__, name, got)  # (0, or None for a null pointer)


def test_pointer_fields_are_void_pointers():
    # (_made_up tells a pointer by its ctype: the model-side pointers must all be that type for its values to be distinct)
    for cls, names in ((_lib.RecommendDesc, CARCA_FIELDS), (_lib.KnnRecommendDesc, KNN_FIELDS)):
        types = dict(cls._fields_)
        assert {types[n] for n in names} <= {C.c_void_p, C.c_int32, C.c_int64}
        assert len(set(_made_up(cls, names).values())) == len(names)


@pytest.mark.parametrize("cls", [_lib.RecommendDesc, _lib.RankDesc, _lib.ListsDesc, _lib.ExplainDesc])
def test_carca_side_fills_the_model_side_of_every_carca_descriptor(cls):
    values = _made_up(_lib.RecommendDesc, CARCA_FIELDS)
    side = ModelSide(fields=dict(values), p_ids=None)
    _check(side, cls, values)
    _check(side, cls, values)  # a second descriptor from the same side: desc() consumed nothing
    assert side.fields == values


@pytest.mark.parametrize("cls", [_lib.KnnRecommendDesc, _lib.KnnRankDesc])
def test_knn_side_fills_the_model_side_of_both_knn_descriptors(cls):
    values = _made_up(_lib.KnnRecommendDesc, KNN_FIELDS)
    _check(ModelSide(fields=dict(values), p_ids=None), cls, values)


def test_a_side_of_the_other_model_is_refused():
    knn = ModelSide(fields=_made_up(_lib.KnnRecommendDesc, KNN_FIELDS), p_ids=None)
    carca = ModelSide(fields=_made_up(_lib.RecommendDesc, CARCA_FIELDS), p_ids=None)
    with pytest.raises(CarcaHipError, match="RecommendDesc has no field"):
        knn.desc(_lib.RecommendDesc)
    with pytest.raises(CarcaHipError, match="KnnRankDesc has no field"):
        carca.desc(_lib.KnnRankDesc)


def test_tensors_are_held_by_name():
    T, qt = object(), object()
    side = ModelSide(fields={}, p_ids="ids", T=T, qt=qt)
    assert side.T is T and side.qt is qt and side.p_ids == "ids" and side.contexts is None
    assert ModelSide(fields={}, p_ids="ids", contexts="X").contexts == "X"
