"""Per-user candidate lists (CARCA.score_items / recommend_from, train.evaluate_listed), the parts
that need no GPU: the C surface, the Python surface and the selection reference the GPU tests use."""
import ctypes as C
import inspect
import os
import re

import torch

from carca_replication_amd import _lib, catalogue, train
from carca_replication_amd.modules import CARCA
from tests.lists_ref import lists_topk, positive_rank


def test_entry_points_declared_and_bound():
    for name in ("carca_score_lists", "carca_recommend_lists"):
        assert name in _lib.declared_symbols()
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args == [C.POINTER(_lib.ListsDesc), C.c_void_p]
    assert "recommend_lists.hip" in _lib.SOURCES


def test_abi_version_unchanged():
    with open(os.path.join(os.path.dirname(_lib._HERE), "include", "carca_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define\s+CARCA_ABI_VERSION\s+3\b", header)
    assert "carca_abi_version() != 3" in inspect.getsource(_lib.load)


def _header_fields(struct):
    with open(os.path.join(os.path.dirname(_lib._HERE), "include", "carca_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
    names = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        first, *rest = decl.split(",")
        names.append(first.split()[-1].lstrip("*"))
        names += [n.strip() for n in rest]
    return names


def test_ctypes_struct_matches_header():
    fields = [f[0] for f in _lib.ListsDesc._fields_]
    assert _header_fields("CarcaListsDesc") == fields
    # the model side is CarcaRecommendDesc's, name for name, so one function fills both
    model = [f[0] for f in _lib.RecommendDesc._fields_ if f[0] not in ("scores", "ld_scores", "ids_out", "ld_ids_out")]
    assert fields[:len(model)] == model


def test_python_surface():
    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    E = inspect.Parameter.empty
    assert params(CARCA.score_items) == [("self", E), ("profile", E), ("context", E), ("items", E),
                                         ("allow_composed", False)]
    assert params(CARCA.recommend_from) == [("self", E), ("profile", E), ("context", E), ("items", E), ("k", 10),
                                            ("exclude", "profile"), ("allow_composed", False)]
    assert params(train.evaluate_listed) == [("model", E), ("loader", E), ("device", E), ("k", E)]
    assert catalogue.LIST_FUSED_MAX == 1024
    assert CARCA.score_items.__doc__ and CARCA.recommend_from.__doc__ and train.evaluate_listed.__doc__


def test_reference_on_a_hand_made_example():
    n = 10
    items = torch.tensor([[3, 5, 3, 0, 12, 7], [2, 4, 6, 8, 4, -1]])
    scores = torch.tensor([[0.5, 0.9, 0.5, 0.0, 0.0, 0.9], [0.1, 0.99, 0.3, 0.3, 0.99, 0.0]])
    # user 0: a tie (5 and 7 at 0.9: the smaller id first), a duplicate (3), id 0 and an id outside the catalogue
    s, i = lists_topk(scores, items, n, 4)
    assert i.tolist() == [[5, 7, 3, 0], [4, 6, 8, 2]]
    assert torch.equal(s, torch.tensor([[0.9, 0.9, 0.5, 0.0], [0.99, 0.3, 0.3, 0.1]]))
    s, i = lists_topk(scores, items, n, 4, excluded=[{7, 9}, {4}])
    assert i.tolist() == [[5, 3, 0, 0], [6, 8, 2, 0]]
    assert torch.equal(s, torch.tensor([[0.9, 0.5, 0.0, 0.0], [0.3, 0.3, 0.1, 0.0]]))
    s, i = lists_topk(scores, items, n, 2)
    assert i.tolist() == [[5, 7], [4, 6]]
    assert positive_rank(i, torch.tensor([7, 8])).tolist() == [1, -1]
