"""CARCA.explain_items / explain_top_slots / recommend_explained, the parts that need no GPU: the C
surface, the Python surface, the argument errors raised before any tensor is touched, and the selection reference the GPU
tests use."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from carca_replication_amd import CarcaHipError, _lib, catalogue
from carca_replication_amd.modules import CARCA
from tests.explain_ref import top_slots
from tests.model_util import build_model
from tests.test_recommend_lists_host import _header_fields


def test_entry_point_declared_and_bound():
    assert "carca_explain_lists" in _lib.declared_symbols()
    res, args = _lib.SIGNATURES["carca_explain_lists"]
    assert res is C.c_int and args == [C.POINTER(_lib.ExplainDesc), C.c_void_p]
    assert "explain_lists.hip" in _lib.SOURCES


def test_abi_version_unchanged():
    with open(os.path.join(os.path.dirname(_lib._HERE), "include", "carca_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define\s+CARCA_ABI_VERSION\s+3\b", header)
    assert "carca_abi_version() != 3" in inspect.getsource(_lib.load)
    assert "carca.py:253-263" in header and "carca.py:338-347" in header


def test_ctypes_struct_matches_header():
    fields = [f[0] for f in _lib.ExplainDesc._fields_]
    assert _header_fields("CarcaExplainDesc") == fields
    # the model side and the list are CarcaListsDesc's, name for name: one function fills both, and recommend_explained
    # copies recommend's model side
    lists = [f[0] for f in _lib.ListsDesc._fields_]
    upto = lists.index("ld_items") + 1
    assert fields[:upto] == lists[:upto]
    model = [f[0] for f in _lib.RecommendDesc._fields_ if f[0] not in ("scores", "ld_scores", "ids_out", "ld_ids_out")]
    assert fields[:len(model)] == model
    for (name, ctype), (lname, ltype) in zip(_lib.ExplainDesc._fields_[:upto], _lib.ListsDesc._fields_[:upto]):
        assert ctype is ltype, name
        assert getattr(_lib.ExplainDesc, name).offset == getattr(_lib.ListsDesc, lname).offset


def test_python_surface():
    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    E = inspect.Parameter.empty
    assert params(CARCA.explain_items) == [("self", E), ("profile", E), ("context", E), ("items", E),
                                           ("allow_composed", False)]
    assert params(CARCA.explain_top_slots) == [("self", E), ("profile", E), ("context", E), ("items", E), ("m", 3),
                                               ("allow_composed", False)]
    assert params(CARCA.recommend_explained) == [("self", E), ("profile", E), ("context", E), ("k", 10), ("m", 3),
                                                 ("exclude", "profile"), ("candidates", None), ("allow_composed", False)]
    assert catalogue.EXPLAIN_TOP_MAX == 8
    assert CARCA.explain_items.__doc__ and CARCA.explain_top_slots.__doc__ and CARCA.recommend_explained.__doc__


def _cpu_model(dec):
    return build_model(dict(d=64, H=4, n_blocks=1, decoder=dec), 50, 24, 6, 12, 16)


def test_errors_that_need_no_device():
    prof = (torch.ones(2, 16, dtype=torch.int64), None, torch.zeros(2, 16, 6))
    ctx, items = torch.zeros(2, 6), torch.ones(2, 5, dtype=torch.int64)
    model = _cpu_model("ca")
    calls = (lambda mo: mo.explain_items(prof, ctx, items), lambda mo: mo.explain_top_slots(prof, ctx, items),
             lambda mo: mo.recommend_explained(prof, ctx))
    model.train()
    for call in calls:
        with pytest.raises(CarcaHipError, match="eval"):
            call(model)
    dot = _cpu_model("dot").eval()
    for call in calls:
        with pytest.raises(CarcaHipError, match="DotProduct"):
            call(dot)
    with pytest.raises(CarcaHipError, match="WeightedDotProduct"):
        _cpu_model("wdot").eval().explain_items(prof, ctx, items)
    for m in (0, 9, -1):
        with pytest.raises(CarcaHipError, match="1..8"):
            catalogue.explain_top_slots("explain_top_slots", None, prof, items, m)
        with pytest.raises(CarcaHipError, match="1..8"):
            catalogue.recommend_explained("recommend_explained", None, prof, 10, m, "profile")
    with pytest.raises(CarcaHipError, match="128"):
        catalogue.recommend_explained("recommend_explained", None, prof, 129, 3, "profile")
    for bad in (items.float(), items[0], items[:1], items[:, :0], items != 0):
        with pytest.raises(CarcaHipError, match="items"):
            catalogue.explain_items("explain_items", None, prof, bad)
        with pytest.raises(CarcaHipError, match="items"):
            catalogue.explain_top_slots("explain_top_slots", None, prof, bad, 3)


def test_reference_on_a_hand_made_example():
    p_x = torch.tensor([[0, 7, 0, 9, 7, 3], [0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 4]])
    contrib = torch.zeros(3, 2, 6, dtype=torch.float64)
    # user 0: slots 1 and 4 tie at 0.5 (the later one first), slot 3 is the largest, slot 5 negative; the padding slots
    # 0 and 2 carry values that must never be picked
    contrib[0, 0] = torch.tensor([9.0, 0.5, 9.0, 0.75, 0.5, -0.25])
    contrib[0, 1] = torch.tensor([0.0, -1.0, 0.0, -1.0, -1.0, -1.0])  # all equal: latest first
    contrib[2, 0, 5] = 0.125
    s, i, v = top_slots(contrib, p_x, 3)
    assert s[0].tolist() == [[3, 4, 1], [5, 4, 3]] and i[0].tolist() == [[9, 7, 7], [3, 7, 9]]
    assert v[0].tolist() == [[0.75, 0.5, 0.5], [-1.0, -1.0, -1.0]]
    assert s[1].tolist() == [[-1] * 3] * 2 and i[1].tolist() == [[0] * 3] * 2 and not bool(v[1].any())
    assert s[2].tolist() == [[5, -1, -1], [5, -1, -1]] and i[2].tolist() == [[4, 0, 0], [4, 0, 0]]
    assert v[2].tolist() == [[0.125, 0.0, 0.0], [0.0, 0.0, 0.0]]
    s, i, v = top_slots(contrib, p_x, 8)
    assert s[0, 0].tolist() == [3, 4, 1, 5, -1, -1, -1, -1]
    live = torch.tensor([[True, False], [True, True], [False, True]])
    s, i, v = top_slots(contrib, p_x, 1, live)
    assert s[:, :, 0].tolist() == [[3, -1], [-1, -1], [-1, 5]] and i[:, :, 0].tolist() == [[9, 0], [0, 0], [0, 4]]
