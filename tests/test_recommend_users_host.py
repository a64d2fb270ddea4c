"""The k best users per listed item (CARCA.recommend_users, catalogue.AudienceTopK), the parts that
need no GPU: the C surface, the argument errors -- raised before anything is launched (the model here lives on the CPU)
-- and the pure-torch reference of the key state, tests/audience_ref.py, against brute force over (logit, user) pairs."""
import ctypes as C
import inspect
import math

import pytest
import torch

from carca_replication_amd import CarcaHipError, _lib, catalogue, train
from carca_replication_amd.catalogue import AudienceTopK, CandidateSet
from carca_replication_amd.modules import CARCA
from tests import audience_ref as R
from tests.model_util import build_model


# ---- the C surface ----------------------------------------------------------------------------------------------------
def test_entry_points_declared_and_bound():
    D, S, A, vp, i = C.POINTER(_lib.RecommendDesc), C.POINTER(_lib.Candidates), C.POINTER(_lib.Audience), C.c_void_p, C.c_int
    assert _lib.SIGNATURES["carca_recommend_users"] == (i, [D, S, A, vp])
    assert _lib.SIGNATURES["carca_audience_read"] == (i, [vp, i, i, i, i, vp, vp, vp])
    declared = _lib.declared_symbols()
    assert "carca_recommend_users" in declared and "carca_audience_read" in declared
    assert [f[0] for f in _lib.Audience._fields_] == ["keys", "ld_keys", "user_ids", "user_base"]
    assert "recommend_users.hip" in _lib.SOURCES and "recommend_score.h" in _lib.HEADERS


def test_symbols_in_the_built_library_and_abi_version():
    lib = _lib.load()
    for name in ("carca_recommend_users", "carca_audience_read"):
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SIGNATURES[name][1]
    assert lib.carca_abi_version() == 3


def test_python_surface():
    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    E = inspect.Parameter.empty
    assert params(CARCA.recommend_users) == [("self", E), ("profile", E), ("context", E), ("items", E), ("k", 10),
                                             ("exclude", "profile"), ("user_ids", None), ("allow_composed", False)]
    assert params(AudienceTopK.__init__) == [("self", E), ("items", E), ("k", E), ("n_items", E), ("device", None)]
    assert params(AudienceTopK.update)[:7] == [("self", E), ("model", E), ("profile", E), ("context", E), ("user_ids", None),
                                               ("exclude", "profile"), ("allow_composed", False)]
    assert params(train.audience) == [("model", E), ("loader", E), ("device", E), ("items", E), ("k", 10)]
    assert CARCA.recommend_users.__doc__ and AudienceTopK.__doc__ and train.audience.__doc__
    for name in ("result", "reset", "update"):
        assert callable(getattr(AudienceTopK, name))


# ---- argument errors --------------------------------------------------------------------------------------------------
def test_argument_errors_before_any_launch(monkeypatch):
    """Every argument error is raised before the model side runs: carca_model_side, the first thing that launches, is
    replaced by a function that fails the test."""
    n, B, L = 50, 3, 8
    model = build_model(dict(d=64, H=4, n_blocks=1, embedding="id", decoder="dot"), n, 24, 0, 12, L).eval()

    def launched(*a, **kw):
        raise AssertionError("the model side ran before the arguments were checked")

    monkeypatch.setattr(catalogue, "carca_model_side", launched)
    prof = (torch.ones(B, L, dtype=torch.int64), None, torch.zeros(B, L, 0))
    items = torch.tensor([3, 9, 4])
    for k in (0, 129):
        with pytest.raises(CarcaHipError, match=f"k = {k} outside 1..128"):
            model.recommend_users(prof, None, items, k=k)
        with pytest.raises(CarcaHipError, match=f"k = {k} outside 1..128"):
            AudienceTopK(items, k, n)
    with pytest.raises(CarcaHipError, match="1-D integer tensor"):
        model.recommend_users(prof, None, items.float())
    with pytest.raises(CarcaHipError, match="1-D integer tensor"):
        model.recommend_users(prof, None, items.view(1, 3))
    with pytest.raises(CarcaHipError, match="CandidateSet or a 1-D integer"):
        model.recommend_users(prof, None, [3, 9, 4])
    for bad in (torch.zeros(B + 1, dtype=torch.int64), torch.zeros(B, 1, dtype=torch.int64), torch.zeros(B),
                torch.zeros(B, dtype=torch.bool), torch.zeros(B, dtype=torch.int16), [0, 1, 2]):
        with pytest.raises(CarcaHipError, match=r"user_ids must be an int32 / int64 \[B = 3\] tensor"):
            model.recommend_users(prof, None, items, user_ids=bad)
    other = CandidateSet(items, n + 1)
    with pytest.raises(CarcaHipError, match=f"built for n_items = {n + 1}, the model has {n}"):
        model.recommend_users(prof, None, other)
    with pytest.raises(CarcaHipError, match=f"built for n_items = {n + 1}, the model has {n}"):
        AudienceTopK(other, 5, n)
    with pytest.raises(CarcaHipError, match=f"built for n_items = {n + 1}, the model has {n}"):
        AudienceTopK(items, 5, n + 1).update(model, prof, None)
    with pytest.raises(CarcaHipError, match="must be a CARCA"):
        AudienceTopK(items, 5, n).update(torch.nn.Linear(2, 2), prof, None)
    model.train()
    with pytest.raises(CarcaHipError, match="training mode"):
        model.recommend_users(prof, None, items)
    with pytest.raises(CarcaHipError, match="training mode"):
        AudienceTopK(items, 5, n).update(model, prof, None)


def test_state_layout_and_reset():
    st = AudienceTopK(torch.tensor([9, 3, 3, 0, 77, 4]), 7, 50)
    assert st.ids.tolist() == [3, 4, 9] and st.ids.dtype == torch.int32
    assert st.keys.dtype == torch.int64 and tuple(st.keys.shape) == (3, 7) and not bool(st.keys.any())
    assert st.k == 7 and st.n_items == 50 and st.rows_seen == 0
    st.keys += 5
    st.rows_seen = 11
    st.reset()
    assert not bool(st.keys.any()) and st.rows_seen == 0
    empty = AudienceTopK(torch.zeros(0, dtype=torch.int64), 3, 50)
    s, u, i = empty.result()  # (Q = 0: nothing to launch, on any device)
    assert tuple(s.shape) == (0, 3) and tuple(u.shape) == (0, 3) and tuple(i.shape) == (0,)
    assert s.dtype == torch.float32 and u.dtype == torch.int64 and i.dtype == torch.int64


# ---- the reference against brute force --------------------------------------------------------------------------------
def _brute(pairs, k):
    """pairs: (logit, user) of one item's eligible users -> its k best: logit descending, +0 before -0, then the smaller
    user; padded with (0.0, -1)."""
    best = sorted(pairs, key=lambda p: (-p[0], math.copysign(1.0, p[0]) < 0, p[1]))[:k]
    return best + [(0.0, -1)] * (k - len(best))


def _as_pairs(keys):
    logits, users, _ = R.unpack(keys)
    return [list(zip(lr, ur)) for lr, ur in zip(logits.tolist(), users.tolist())]


def _same(got, want):
    """Equal (logit, user) lists, the sign of a zero included."""
    return len(got) == len(want) and all(
        g[1] == w[1] and g[0] == w[0] and math.copysign(1.0, g[0]) == math.copysign(1.0, w[0]) for g, w in zip(got, want))


def _batch(B, Q, seed):
    g = torch.Generator().manual_seed(seed)
    # few distinct values: many ties; negative logits, both zeros, subnormals and infinities among them
    pool = torch.tensor([-3.5, -1.0, -0.0, 0.0, 1e-42, -1e-42, 0.25, 0.25, 2.0, float("inf"), float("-inf"), 7.5])
    logits = pool[torch.randint(0, pool.numel(), (B, Q), generator=g)]
    logits = torch.where(torch.rand(B, Q, generator=g) < 0.5, logits, torch.randn(B, Q, generator=g))
    eligible = torch.rand(B, Q, generator=g) < 0.8
    eligible[:, 0] = False  # a column every user is excluded from
    sent = torch.rand(B, Q, generator=g) < 0.1
    logits = torch.where(sent, torch.full((), R.SENTINEL_BITS, dtype=torch.int32).view(torch.float32), logits)
    return logits, eligible, sent


def test_pack_and_unpack_round_trip_and_order():
    x = torch.tensor([float("-inf"), -3.5, -1e-42, -0.0, 0.0, 1e-42, 0.25, 2.0, float("inf")])
    o = R.order_bits(x)
    assert bool((o[1:] > o[:-1]).all()) and int(o.min()) > 0 and int(o.max()) < 1 << 32
    assert torch.equal(R.unorder_bits(o).view(torch.int32), x.view(torch.int32))
    assert int(R.order_bits(torch.full((1,), -1, dtype=torch.int32).view(torch.float32))) == 0  # the sentinel
    users = torch.tensor([0, 1, 77, (1 << 31) - 1])
    keys = R.pack(x.view(-1, 1), users.view(1, -1))
    logits, got_users, empty = R.unpack(keys)
    assert not bool(empty.any())
    assert torch.equal(logits.view(torch.int32), x.view(-1, 1).expand(-1, 4).contiguous().view(torch.int32))
    assert torch.equal(got_users, users.view(1, -1).expand(9, -1))
    f = R.flip(keys)  # unsigned order: the logit first, then the SMALLER user
    assert bool((f[1:, :] > f[:-1, :]).all()) and bool((f[:, :-1] > f[:, 1:]).all())
    assert bool((f[1:, -1] > f[:-1, 0]).all())
    z = R.unpack(torch.zeros(2, 3, dtype=torch.int64))
    assert bool(z[2].all()) and not bool(z[0].any()) and bool((z[1] == -1).all())


@pytest.mark.parametrize("k", [1, 4, 40])
def test_merge_equals_brute_force(k):
    B, Q = 23, 6
    logits, eligible, sent = _batch(B, Q, seed=k)
    users = torch.randperm(1000, generator=torch.Generator().manual_seed(k))[:B]
    users[5], users[11] = -1, -9  # dropped rows
    got = _as_pairs(R.merge(torch.zeros(Q, k, dtype=torch.int64), logits, users, eligible))
    for q in range(Q):
        pairs = [(float(logits[b, q]), int(users[b])) for b in range(B)
                 if eligible[b, q] and not sent[b, q] and users[b] >= 0]
        assert _same(got[q], _brute(pairs, k)), q
    assert all(p == (0.0, -1) for p in got[0])  # the column nobody is eligible for: padding only
    if k == 40:
        assert any(p[1] == -1 for row in got[1:] for p in row)  # (k beyond the eligible count does pad)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_merge_is_split_and_order_invariant(seed):
    B, Q, k = 57, 5, 6
    logits, eligible, _ = _batch(B, Q, seed=100 + seed)
    users = torch.arange(B) * 3 + 1
    zero = torch.zeros(Q, k, dtype=torch.int64)
    whole = R.merge(zero, logits, users, eligible)
    g = torch.Generator().manual_seed(seed)
    for _ in range(4):
        cuts = sorted(set(torch.randint(1, B, (int(torch.randint(1, 8, (1,), generator=g)),), generator=g).tolist()))
        bounds = list(zip([0] + cuts, cuts + [B])) + [(B, B)]  # (an empty update among them)
        perm = torch.randperm(B, generator=g)  # which users share an update is random too
        for order in (bounds, bounds[::-1], [bounds[i] for i in torch.randperm(len(bounds), generator=g).tolist()]):
            state = zero
            for a, b in order:
                rows = perm[a:b]
                state = R.merge(state, logits[rows], users[rows], eligible[rows])
            assert torch.equal(state, whole)
    assert torch.equal(R.sort_desc(whole), whole)  # rows stay sorted


def test_link_is_applied_to_the_unpacked_logit():
    x = torch.tensor([[-2.0, 0.5]])
    keys = R.pack(x, torch.tensor([[4, 5]]))
    logits = R.unpack(keys)[0]
    assert torch.equal(R.link(logits, 0), torch.sigmoid(x)) and torch.equal(R.link(logits, 2), (x + 1) * 0.5)
