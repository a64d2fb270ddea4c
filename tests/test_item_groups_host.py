"""Item groups (catalogue.ItemGroups, CARCA.recommend_by_group / recommend_capped), the parts that
need no GPU: the normalisation of a label tensor, every constructor error, the C surface, and the argument errors of the
two methods, which are raised before anything is launched (the model here lives on the CPU)."""
import ctypes as C
import inspect

import pytest
import torch

from carca_replication_amd import CarcaHipError, _lib, catalogue
from carca_replication_amd.catalogue import ItemGroups
from carca_replication_amd.modules import CARCA
from tests.model_util import build_model

# id:       0  1   2  3  4   5  6  7  8  9
LABELS = [3, 2, -1, 0, 4, -7, 2, 0, 4, 0]  # entry 0 names a real group and is ignored; group 1 and group 3 are empty


def _check_invariants(gr, labels, G):
    n = len(labels)
    want = [-1 if (i == 0 or g < 0) else g for i, g in enumerate(labels)]
    assert gr.n_items == n and gr.n_groups == G
    for t, size in ((gr.order, sum(g >= 0 for g in want)), (gr.offsets, G + 1), (gr.pos_of, n), (gr.group_of, n)):
        assert t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == (size,)
    assert gr.group_of.tolist() == want
    order, offsets, pos_of = gr.order.tolist(), gr.offsets.tolist(), gr.pos_of.tolist()
    assert [(want[i], i) for i in order] == sorted((g, i) for i, g in enumerate(want) if g >= 0)  # sorted by (group, id)
    assert offsets[0] == 0 and offsets[-1] == len(order)
    for g in range(G):  # the offsets delimit exactly each group's members
        members = [i for i, lab in enumerate(want) if lab == g]
        assert order[offsets[g]:offsets[g + 1]] == members
        assert gr.members(g).tolist() == members
    assert all(pos_of[i] == p for p, i in enumerate(order))
    assert all(pos_of[i] == -1 for i in range(n) if i not in order)
    assert len(gr) == len(order)


def test_normalisation_on_a_hand_written_example():
    gr = ItemGroups(torch.tensor(LABELS))
    _check_invariants(gr, LABELS, 5)
    assert gr.order.tolist() == [3, 7, 9, 1, 6, 4, 8]
    assert gr.offsets.tolist() == [0, 3, 3, 5, 5, 7]
    assert gr.members(1).numel() == 0 and gr.members(3).numel() == 0


def test_explicit_n_groups_larger_than_the_labels():
    gr = ItemGroups(torch.tensor(LABELS, dtype=torch.int32), n_groups=8)
    _check_invariants(gr, LABELS, 8)
    assert gr.offsets.tolist()[5:] == [7, 7, 7, 7]


def test_no_grouped_item_and_a_single_item_catalogue():
    gr = ItemGroups(torch.tensor([5, -1, -1, -2]))
    _check_invariants(gr, [5, -1, -1, -2], 1)
    assert len(gr) == 0 and gr.offsets.tolist() == [0, 0]
    _check_invariants(ItemGroups(torch.tensor([0])), [0], 1)


def test_to_keeps_the_object_where_it_already_lives():
    gr = ItemGroups(torch.tensor(LABELS))
    assert gr.to("cpu") is gr
    src = torch.tensor(LABELS)
    ItemGroups(src)
    assert src.tolist() == LABELS  # the caller's tensor is not written


def test_constructor_errors():
    for bad in (torch.tensor([0.0, 1.0]), torch.tensor([[0, 1]]), torch.tensor([True, False]), torch.tensor(3),
                torch.zeros(0, dtype=torch.int64), [0, 1]):
        with pytest.raises(CarcaHipError, match="1-D integer tensor"):
            ItemGroups(bad)
    with pytest.raises(CarcaHipError, match=r"label 4 outside \[0, n_groups = 4\)"):
        ItemGroups(torch.tensor(LABELS), n_groups=4)
    with pytest.raises(CarcaHipError, match="must be positive"):
        ItemGroups(torch.tensor(LABELS), n_groups=0)
    with pytest.raises(CarcaHipError, match="65536 groups exceed 65535"):
        ItemGroups(torch.tensor([0, 65535]))
    with pytest.raises(CarcaHipError, match="exceed 65535"):
        ItemGroups(torch.tensor(LABELS), n_groups=70000)
    assert ItemGroups(torch.tensor([0, 65534])).n_groups == 65535  # the largest legal G
    with pytest.raises(CarcaHipError, match="outside"):
        ItemGroups(torch.tensor(LABELS)).members(5)


def test_entry_points_declared_and_bound():
    R, G, vp = C.POINTER(_lib.RecommendDesc), C.POINTER(_lib.ItemGroups), C.c_void_p
    assert _lib.SIGNATURES["carca_recommend_groups"] == (C.c_int, [R, G, vp])
    assert _lib.SIGNATURES["carca_recommend_capped"] == (C.c_int, [R, G, C.c_int, vp])
    declared = _lib.declared_symbols()
    assert "carca_recommend_groups" in declared and "carca_recommend_capped" in declared
    assert [f[0] for f in _lib.ItemGroups._fields_] == ["order", "offsets", "pos_of", "n", "n_groups"]
    assert "group_select.h" in _lib.HEADERS


def test_symbols_in_the_built_library_and_abi_version():
    lib = _lib.load()
    for name in ("carca_recommend_groups", "carca_recommend_capped"):
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SIGNATURES[name][1]
    assert lib.carca_abi_version() == 3


def test_python_surface():
    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    E = inspect.Parameter.empty
    assert params(CARCA.recommend_by_group) == [("self", E), ("profile", E), ("context", E), ("groups", E), ("k", 10),
                                                ("exclude", "profile"), ("allow_composed", False)]
    assert params(CARCA.recommend_capped) == [("self", E), ("profile", E), ("context", E), ("groups", E), ("k", 10),
                                              ("max_per_group", 1), ("exclude", "profile"), ("allow_composed", False)]
    assert params(ItemGroups.__init__) == [("self", E), ("group_of", E), ("n_groups", None), ("device", None)]
    assert CARCA.recommend_by_group.__doc__ and CARCA.recommend_capped.__doc__ and ItemGroups.__doc__
    assert catalogue.GROUPS_MAX == 65535 and catalogue.CAPPED_SCRATCH_MAX == 1 << 30


def test_argument_errors_before_any_launch(monkeypatch):
    """Every argument error is raised before the model side runs: carca_model_side, the first thing that launches, is
    replaced by a function that fails the test."""
    n, B, L = 50, 2, 8
    model = build_model(dict(d=64, H=4, n_blocks=1, embedding="id", decoder="dot"), n, 24, 0, 12, L).eval()

    def launched(*a, **kw):
        raise AssertionError("the model side ran before the arguments were checked")

    monkeypatch.setattr(catalogue, "carca_model_side", launched)
    prof = (torch.ones(B, L, dtype=torch.int64), None, torch.zeros(B, L, 0))
    gr = ItemGroups(torch.arange(n) % 4)
    for k in (0, 129):
        with pytest.raises(CarcaHipError, match=f"k = {k} outside 1..128"):
            model.recommend_by_group(prof, None, gr, k=k)
        with pytest.raises(CarcaHipError, match=f"k = {k} outside 1..128"):
            model.recommend_capped(prof, None, gr, k=k)
    with pytest.raises(CarcaHipError, match="max_per_group = 0 must be positive"):
        model.recommend_capped(prof, None, gr, k=10, max_per_group=0)
    other = ItemGroups(torch.arange(n + 1) % 4)
    for call in (model.recommend_by_group, model.recommend_capped):
        with pytest.raises(CarcaHipError, match=f"built for n_items = {n + 1}, the model has {n}"):
            call(prof, None, other)
        with pytest.raises(CarcaHipError, match="must be a catalogue.ItemGroups"):
            call(prof, None, torch.arange(n) % 4)
    big = (torch.ones(1 << 15, L, dtype=torch.int64), None, torch.zeros(1 << 15, L, 0))
    wide = ItemGroups(torch.arange(n) % 4, n_groups=65535)  # 2^15 x 65535 x 1 x 8 B > 1 GiB
    with pytest.raises(CarcaHipError, match=r"B = 32768 users x G = 65535 groups x m = 1 per group"):
        model.recommend_capped(big, None, wide, k=10, max_per_group=1)
    model.train()
    for call in (model.recommend_by_group, model.recommend_capped):
        with pytest.raises(CarcaHipError, match="training mode"):
            call(prof, None, gr)
