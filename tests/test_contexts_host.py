"""Several request contexts per user (CARCA.score_items_at / best_context / recommend_at), the parts
that need no GPU: the C surface, the Python signatures, and the argument errors -- raised before anything is launched
(the model here lives on the CPU)."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from carca_replication_amd import CarcaHipError, _lib, catalogue
from carca_replication_amd.modules import CARCA
from tests.model_util import build_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("carca_score_lists_at", "carca_recommend_at", "carca_recommend_among_at")


def _header():
    with open(os.path.join(ROOT, "include", "carca_hip.h")) as f:
        return f.read()


# ---- the C surface ----------------------------------------------------------------------------------------------------
def test_entry_points_declared_and_bound():
    L, R, X, S = (C.POINTER(t) for t in (_lib.ListsDesc, _lib.RecommendDesc, _lib.Contexts, _lib.Candidates))
    vp, i = C.c_void_p, C.c_int
    assert _lib.SIGNATURES["carca_score_lists_at"] == (i, [L, X, vp, i, vp])
    assert _lib.SIGNATURES["carca_recommend_at"] == (i, [R, X, vp])
    assert _lib.SIGNATURES["carca_recommend_among_at"] == (i, [R, X, S, vp])
    declared = _lib.declared_symbols()
    for name in ENTRIES:
        assert name in declared, name
    assert "recommend_contexts.hip" in _lib.SOURCES
    assert os.path.exists(os.path.join(ROOT, "carca_replication_amd", "csrc", "recommend_contexts.hip"))


def test_contexts_struct_matches_the_header_field_for_field():
    body = re.search(r"typedef struct CarcaContexts \{(.*?)\} CarcaContexts;", _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = (C.c_void_p, decl.rsplit("*", 1)[1]) if "*" in decl else (C.c_int32, decl.split(None, 1)[1])
        if "*" not in decl:
            assert decl.split()[0] == "int", decl
        fields += [(n.strip(), ctype) for n in names.split(",")]
    assert fields == list(_lib.Contexts._fields_)
    assert [n for n, _ in fields] == ["n_contexts", "user_q", "ld_user_q", "user_off", "ld_user_off", "user_m", "ld_user_m"]


def test_abi_version_stays_3_and_the_descriptors_keep_their_fields():
    assert re.search(r"#define CARCA_ABI_VERSION 3\b", _header())
    # additions only: the descriptors the new entry points take are the single-context calls' own
    assert [f[0] for f in _lib.ListsDesc._fields_][-8:] == ["items", "n_list", "ld_items", "sorted_rows", "scores",
                                                           "ld_scores", "ids_out", "ld_ids_out"]
    assert [f[0] for f in _lib.RecommendDesc._fields_][-4:] == ["scores", "ld_scores", "ids_out", "ld_ids_out"]


def test_symbols_in_the_built_library():
    lib = _lib.load()
    for name in ENTRIES:
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SIGNATURES[name][1]
    assert lib.carca_abi_version() == 3


def test_python_surface():
    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    E = inspect.Parameter.empty
    assert params(CARCA.score_items_at) == [("self", E), ("profile", E), ("contexts", E), ("items", E),
                                            ("allow_composed", False)]
    assert params(CARCA.best_context) == [("self", E), ("profile", E), ("contexts", E), ("items", E),
                                          ("allow_composed", False)]
    assert params(CARCA.recommend_at) == [("self", E), ("profile", E), ("contexts", E), ("k", 10), ("exclude", "profile"),
                                          ("candidates", None), ("allow_composed", False), ("max_scratch_bytes", 1 << 30)]
    for fn in (CARCA.score_items_at, CARCA.best_context, CARCA.recommend_at):
        assert fn.__doc__


# ---- argument errors --------------------------------------------------------------------------------------------------
def test_argument_errors_before_any_launch(monkeypatch):
    """Every argument error is raised before the model side runs: the two functions that launch first are replaced by
    functions that fail the test."""
    n, B, L, n_ctx = 50, 3, 8, 6
    model = build_model(dict(d=64, H=4, n_blocks=1, embedding="all", decoder="ca"), n, 24, n_ctx, 12, L).eval()

    def launched(*a, **kw):
        raise AssertionError("the model side ran before the arguments were checked")

    monkeypatch.setattr(catalogue, "carca_model_side_at", launched)
    monkeypatch.setattr(catalogue, "carca_model_side", launched)
    prof = (torch.ones(B, L, dtype=torch.int64), None, torch.zeros(B, L, n_ctx))
    items = torch.ones(B, 5, dtype=torch.int64)
    good = torch.zeros(B, 2, n_ctx)
    calls = {
        "score_items_at": lambda X, **kw: model.score_items_at(prof, X, items, **kw),
        "best_context": lambda X, **kw: model.best_context(prof, X, items, **kw),
        "recommend_at": lambda X, **kw: model.recommend_at(prof, X, **kw),
    }
    for name, call in calls.items():
        for bad in (torch.zeros(B, n_ctx), torch.zeros(B, 2, n_ctx, 1), torch.zeros(B, 2, n_ctx, dtype=torch.int64), None):
            with pytest.raises(CarcaHipError, match=rf"{name}: contexts must be a float \[B, C, n_ctx\] tensor"):
                call(bad)
        with pytest.raises(CarcaHipError, match=f"{name}: contexts has {B + 1} rows, the profile has B = {B} users"):
            call(torch.zeros(B + 1, 2, n_ctx))
        with pytest.raises(CarcaHipError, match=f"{name}: contexts holds C = 0 contexts"):
            call(torch.zeros(B, 0, n_ctx))
    for k in (0, 129):
        with pytest.raises(CarcaHipError, match=f"recommend_at: k = {k} outside 1..128"):
            calls["recommend_at"](good, k=k)
    for bad_items in (items.float(), items[0], items[:2], torch.zeros(B, 0, dtype=torch.int64)):
        with pytest.raises(CarcaHipError, match=r"items must be an int \[B, N\] tensor"):
            model.score_items_at(prof, good, bad_items)
        with pytest.raises(CarcaHipError, match=r"items must be an int \[B, N\] tensor"):
            model.best_context(prof, good, bad_items)
    model.train()
    for name, call in calls.items():
        with pytest.raises(CarcaHipError, match=f"{name}: the model is in training mode"):
            call(good)


def test_cpu_tensors_raise_and_name_no_fallback():
    model = build_model(dict(d=64, H=4, n_blocks=1, embedding="all", decoder="ca"), 50, 24, 6, 12, 8).eval()
    prof = (torch.ones(3, 8, dtype=torch.int64), None, torch.zeros(3, 8, 6))
    with pytest.raises(CarcaHipError, match="needs CUDA/ROCm tensors"):
        model.recommend_at(prof, torch.zeros(3, 2, 6))
