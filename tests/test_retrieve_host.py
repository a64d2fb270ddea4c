"""The deep top-k (CARCA.retrieve / KNN.retrieve), the parts that need no GPU: the C surface, the
tuning key, the Python signatures and the k check -- raised before the model side runs (the models here live on the
CPU)."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from carca_replication_amd import CarcaHipError, _lib, catalogue, ops
from carca_replication_amd.modules import CARCA, KNN
from tests.model_util import build_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("carca_retrieve", "carca_retrieve_among", "carca_knn_retrieve")


def test_entry_points_declared_bound_and_built():
    R, S, K = (C.POINTER(t) for t in (_lib.RecommendDesc, _lib.Candidates, _lib.KnnRecommendDesc))
    vp, i = C.c_void_p, C.c_int
    assert _lib.SIGNATURES["carca_retrieve"] == (i, [R, vp])
    assert _lib.SIGNATURES["carca_retrieve_among"] == (i, [R, S, vp])
    assert _lib.SIGNATURES["carca_knn_retrieve"] == (i, [K, vp])
    declared = _lib.declared_symbols()
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SIGNATURES[name][1]
    assert lib.carca_abi_version() == 3
    assert "retrieve.hip" in _lib.SOURCES and "deep_select.h" in _lib.HEADERS
    for name in ("retrieve.hip", "deep_select.h"):
        assert os.path.exists(os.path.join(ROOT, "carca_replication_amd", "csrc", name))


def test_abi_version_stays_3_and_the_descriptors_keep_their_fields():
    with open(os.path.join(ROOT, "include", "carca_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define CARCA_ABI_VERSION 3\b", header)
    assert [f[0] for f in _lib.RecommendDesc._fields_][-4:] == ["scores", "ld_scores", "ids_out", "ld_ids_out"]
    assert [f[0] for f in _lib.KnnRecommendDesc._fields_][:5] == ["B", "L", "n_items", "F", "k"]
    assert "key 24" in header


def test_tuning_key_round_trips():
    assert ops.TUNE_RETRIEVE_PARTS == 24
    lib = _lib.load()
    assert lib.carca_get_tuning(24) == 0
    try:
        for v in (7, 64, 1):
            assert lib.carca_set_tuning(ops.TUNE_RETRIEVE_PARTS, v) == 0
            assert lib.carca_get_tuning(24) == v and ops.get_tuning(ops.TUNE_RETRIEVE_PARTS) == v
    finally:
        lib.carca_set_tuning(ops.TUNE_RETRIEVE_PARTS, 0)
    assert lib.carca_get_tuning(24) == 0
    assert lib.carca_get_tuning(25) == -1  # (the next key does not exist)


def test_recommends_cap_is_unchanged():
    assert catalogue.KMAX == 128 and catalogue.RETRIEVE_KMAX == 4096
    with pytest.raises(CarcaHipError, match=r"recommend: k = 129 outside 1\.\.128"):
        catalogue._check_k("recommend", 129)


def test_python_surface():
    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    E = inspect.Parameter.empty
    assert params(CARCA.retrieve) == [("self", E), ("profile", E), ("context", E), ("k", 1000), ("exclude", "profile"),
                                      ("candidates", None), ("allow_composed", False)]
    assert params(KNN.retrieve) == [("self", E), ("profile", E), ("context", None), ("k", 1000), ("exclude", "profile")]
    assert params(catalogue.retrieve) == [("what", E), ("desc", E), ("entry", E), ("model_side", E), ("profile", E),
                                          ("k", E), ("exclude", E), ("candidates", None)]
    assert CARCA.retrieve.__doc__ and KNN.retrieve.__doc__ and catalogue.retrieve.__doc__


def test_k_outside_the_range_raises_before_the_model_side_runs(monkeypatch):
    n, B, L, n_ctx = 50, 3, 8, 6
    model = build_model(dict(d=64, H=4, n_blocks=1, embedding="all", decoder="ca"), n, 24, n_ctx, 12, L).eval()
    knn = KNN()
    knn.register_attr_table(torch.zeros(n, 5))

    def launched(*a, **kw):
        raise AssertionError("the model side ran before k was checked")

    monkeypatch.setattr(catalogue, "carca_model_side", launched)
    monkeypatch.setattr(catalogue, "knn_model_side", launched)
    prof = (torch.ones(B, L, dtype=torch.int64), None, torch.zeros(B, L, n_ctx))
    ctx = torch.zeros(B, n_ctx)
    for k in (0, 4097):
        with pytest.raises(CarcaHipError, match=rf"^retrieve: k = {k} outside 1\.\.4096"):
            model.retrieve(prof, ctx, k=k)
        with pytest.raises(CarcaHipError, match=rf"^KNN\.retrieve: k = {k} outside 1\.\.4096"):
            knn.retrieve(prof, None, k=k)
        with pytest.raises(CarcaHipError, match=rf"^x: k = {k} outside 1\.\.4096"):
            catalogue.retrieve("x", _lib.RecommendDesc, "carca_retrieve", launched, prof, k, "profile")
    with pytest.raises(AssertionError, match="the model side ran"):  # a k inside the range does reach the model side
        model.retrieve(prof, ctx, k=4096)
    model.train()
    with pytest.raises(CarcaHipError, match="retrieve: the model is in training mode"):
        model.retrieve(prof, ctx, k=10)


def test_c_entry_points_check_the_depth_before_any_launch():
    """The checks of rc_check / kc_check with the deep bound, on descriptors whose k or row strides fail them: both are
    read before anything is allocated or launched (the pointers are never followed)."""
    lib = _lib.load()
    D = _lib.RecommendDesc(B=1, L=1, n_items=10, d=64, H=1, k=4097, decoder=1, p_ids=64, ld_p_ids=1, item_q=64,
                           ld_item_q=64, user_q=64, ld_user_q=64, scores=64, ld_scores=4097, ids_out=64, ld_ids_out=4097)
    cand = _lib.Candidates(64, 3)
    for call in (lambda: lib.carca_retrieve(C.byref(D), None), lambda: lib.carca_retrieve_among(C.byref(D), C.byref(cand), None)):
        D.k, D.ld_scores = 4097, 4097
        assert call() == -1 and b"retrieve: k = 4097 exceeds the largest k, 4096" in lib.carca_last_error()
        D.k = 0
        assert call() == -2 and b"retrieve: k must be positive" in lib.carca_last_error()
        D.k, D.ld_scores = 4096, 4095
        assert call() == -2 and b"retrieve: row stride shorter than its row" in lib.carca_last_error()
    K = _lib.KnnRecommendDesc(B=1, L=1, n_items=10, F=4, k=4097, p_ids=64, ld_p_ids=1, table=64, ld_table=4, scores=64,
                              ld_scores=4097, ids_out=64, ld_ids_out=4097)
    assert lib.carca_knn_retrieve(C.byref(K), None) == -1 and b"knn_retrieve: k = 4097 outside 1..4096" in lib.carca_last_error()
    K.k = 0
    assert lib.carca_knn_retrieve(C.byref(K), None) == -1
    K.k, K.ld_ids_out = 4096, 4095
    assert lib.carca_knn_retrieve(C.byref(K), None) == -2 and b"row stride shorter than k" in lib.carca_last_error()
    assert lib.carca_retrieve(None, None) == -2 and lib.carca_knn_retrieve(None, None) == -2


def test_cpu_tensors_raise_and_name_no_fallback():
    model = build_model(dict(d=64, H=4, n_blocks=1, embedding="all", decoder="ca"), 50, 24, 6, 12, 8).eval()
    prof = (torch.ones(3, 8, dtype=torch.int64), None, torch.zeros(3, 8, 6))
    with pytest.raises(CarcaHipError, match="needs CUDA/ROCm tensors"):
        model.retrieve(prof, torch.zeros(3, 6), k=500)
