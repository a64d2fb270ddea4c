"""CPU checks of the KNN catalogue calls (csrc/knn_catalogue.hip): the int8 routing rule at its boundaries, the int8 copy
of a table, and the C ABI surface (entry points declared, exported and bound; ctypes structs matching the header)."""
import os
import re

import torch

from carca_replication_amd import _lib, ops
from carca_replication_amd.modules import KNN


def test_int8_rule_boundaries():
    assert ops.knn_int8_eligible(True, 1.0, 4096)
    assert ops.knn_int8_eligible(True, 127.0, 1000)  # 127^2 * 1000 = 16,129,000 < 2^24
    assert not ops.knn_int8_eligible(True, 128.0, 1)  # int8 holds -128, but not +128
    assert not ops.knn_int8_eligible(False, 1.0, 8)  # a non-integer entry
    assert ops.knn_int8_eligible(True, 64.0, 4095)  # 64^2 * 4095 = 2^24 - 4096
    assert not ops.knn_int8_eligible(True, 64.0, 4096)  # 64^2 * 4096 = 2^24: a sum could reach 2^24
    assert not ops.knn_int8_eligible(True, 127.0, 1041)  # 127^2 * 1041 > 2^24
    assert ops.knn_int8_eligible(True, 0.0, 10 ** 6)  # an all-zero table


def test_int8_table_copy():
    A = torch.tensor([[0.0, 1.0, -127.0], [3.0, 0.0, 5.0]])
    t8 = ops.knn_int8_table(A)
    assert t8.dtype == torch.int8 and t8.shape == (2, 64)
    assert torch.equal(t8[:, :3].float(), A) and not bool(t8[:, 3:].any())
    assert ops.knn_int8_table(A + 0.5) is None
    assert ops.knn_int8_table(torch.tensor([[128.0]])) is None
    assert ops.knn_int8_table(torch.tensor([[float("nan")]])) is None
    assert ops.knn_int8_table(torch.tensor([[float("inf")]])) is None
    assert ops.knn_int8_table(torch.full((3, 4096), 64.0)) is None
    assert ops.knn_int8_table(torch.full((3, 4095), 64.0)) is not None


def test_int8_cache_follows_the_table():
    m = KNN()
    A = torch.zeros(4, 8)
    A[1, 2] = 1.0
    m.register_attr_table(A.clone())
    t8 = m.int8_table()
    assert t8 is not None and m.int8_table() is t8  # cached
    m._attr_table[1, 3] = 0.5  # an in-place change bumps _version: the table no longer qualifies
    assert m.int8_table() is None
    m.register_attr_table(A)
    assert m.int8_table() is not None
    assert "_i8_cache" not in m.__getstate__()


def test_entry_points_declared_and_bound():
    for name in ("carca_knn_recommend", "carca_knn_rank_items"):
        assert name in _lib.declared_symbols()
        assert name in _lib.SIGNATURES
    assert hasattr(KNN, "recommend") and hasattr(KNN, "rank_items")


def _header_fields(struct):
    with open(os.path.join(os.path.dirname(_lib._HERE), "include", "carca_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
    names = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):  # "const int32_t* p_ids" / "int n_list, ld_items"
        first, *rest = decl.split(",")
        names.append(first.split()[-1].lstrip("*"))
        names += [n.strip() for n in rest]
    return names


def test_ctypes_structs_match_header():
    for struct, cls in (("CarcaKnnRecommendDesc", _lib.KnnRecommendDesc), ("CarcaKnnRankDesc", _lib.KnnRankDesc)):
        assert _header_fields(struct) == [f[0] for f in cls._fields_], struct
