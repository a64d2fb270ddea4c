"""KNN.recommend / KNN.rank_items (full-catalogue top-k and exact ranks of the KNN baseline, csrc/knn_catalogue.hip)
against a float64 oracle: scores q_u . A^T with q_u the last profile slot's attribute row, items ordered by
(-score, id), id 0 and the excluded ids left out.

Integer tables with max|x|^2 F < 2^24 take the i8 MFMA path and are exact, so scores, ids and ranks are compared with
torch.equal.  Real-valued tables take the fp32 path: scores agree to 1e-6 * sum |a_i b_i| (test_hip_knn.py's bound), and
ids / ranks are compared wherever that bound does not make the order ambiguous."""
import math

import numpy as np
import pytest
import torch

from carca_replication_amd import CarcaHipError
from carca_replication_amd.modules import KNN

pytestmark = pytest.mark.gpu


def _multihot(n_items, F, density, seed):
    g = torch.Generator().manual_seed(seed)
    A = (torch.rand(n_items, F, generator=g) < density).float()
    A[0] = 0
    return A


def _real(n_items, F, seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.rand(n_items, F, generator=g) * 2 - 1
    A[0] = 0
    return A


def _model(A):
    m = KNN().cuda()
    m.register_attr_table(A.cuda())
    return m


def _query64(A64, p_x, p_a=None):
    """[B, F] float64 query rows on A64's device: p_a[:, -1], or A[p_x[:, -1]] with ids outside the table as zero rows."""
    if p_a is not None:
        return p_a[:, -1].to(A64.device, torch.float64)
    ids = p_x[:, -1].to(A64.device, torch.int64)
    ok = (ids >= 0) & (ids < A64.shape[0])
    return torch.where(ok[:, None], A64[ids.clamp(0, A64.shape[0] - 1)], torch.zeros((), dtype=torch.float64,
                                                                                       device=A64.device))


def _oracle(A, p_x, excl, p_a=None):
    """(S [B, n] float64, bound [B, n] = 1e-6 sum |a b|, eligible [B, n] bool), on the device."""
    A64 = A.cuda().double()
    q = _query64(A64, p_x, p_a)
    S = q @ A64.T
    bound = 1e-6 * (q.abs() @ A64.abs().T)
    elig = torch.ones_like(S, dtype=torch.bool)
    elig[:, 0] = False
    if excl is not None:
        e = excl.cuda().long()
        ok = (e > 0) & (e < A.shape[0])
        rows = torch.arange(e.shape[0], device=e.device)[:, None].expand_as(e)
        elig[rows[ok], e[ok]] = False
    return S, bound, elig


def _oracle_topk(S, elig, k):
    """ids [B, k] (0-padded) and scores [B, k] float64 by (-score, id) over the eligible items."""
    B, n = S.shape
    ids = torch.zeros(B, k, dtype=torch.int64)
    sc = torch.zeros(B, k, dtype=torch.float64)
    Sc, Ec = S.cpu().numpy(), elig.cpu().numpy()
    for u in range(B):
        cand = np.nonzero(Ec[u])[0]
        order = cand[np.lexsort((cand, -Sc[u, cand]))][:k]
        ids[u, :len(order)] = torch.from_numpy(order)
        sc[u, :len(order)] = torch.from_numpy(Sc[u, order])
    return sc, ids


def _oracle_ranks(S, elig, items):
    """0-based rank of every listed item among the eligible ones; -1 for ids 0 / outside [0, n)."""
    n = S.shape[1]
    it = items.cuda().long()
    valid = (it >= 1) & (it < n)
    itc = it.clamp(0, n - 1)
    s_t = S.gather(1, itc)  # [B, N]
    ids = torch.arange(n, device=S.device)
    before = (S[:, None, :] > s_t[:, :, None]) | ((S[:, None, :] == s_t[:, :, None]) & (ids[None, None, :] < itc[:, :, None]))
    r = (before & elig[:, None, :]).sum(-1)
    return torch.where(valid, r, torch.full_like(r, -1)).cpu()


def _batch(B, L, n_items, seed, lo=0):
    g = torch.Generator().manual_seed(seed)
    p_x = torch.randint(lo, n_items, (B, L), generator=g, dtype=torch.int64)
    p_x[:, -1] = torch.randint(1, n_items, (B,), generator=g)
    return p_x


def _targets(B, N, n_items, p_x, seed):
    """random targets, some taken from the profile (excluded items keep their position), one repeat per user"""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(1, n_items, (B, N), generator=g)
    if N >= 4:
        t[:, 1] = p_x[:, 0].clamp(min=1)
        t[:, 2] = t[:, 3]
    return t


# ---- integer tables: the i8 path, exact ----------------------------------------------------------------------------
@pytest.mark.parametrize("F,n_items,B,density", [(37, 1000, 5, 0.3), (64, 3000, 70, 0.1), (4096, 12102, 128, 0.01),
                                                   (260, 300, 70, 0.1)])  # int8 rows of 320 bytes: five chunks
def test_multihot_exact(F, n_items, B, density):
    A = _multihot(n_items, F, density, F)
    model = _model(A)
    assert model.int8_table() is not None  # the routing rule admits a 0/1 table
    p_x = _batch(B, 50, n_items, F + 1)
    prof = (p_x.cuda(), None, None)
    S, _, elig = _oracle(A, p_x, p_x)
    for k in (10, 128):
        sc, ids = model.recommend(prof, None, k=k)
        want_s, want_i = _oracle_topk(S, elig, k)
        assert torch.equal(ids.cpu(), want_i)
        assert torch.equal(sc.cpu(), want_s.float())
    items = _targets(B, 64, n_items, p_x, F + 2)
    sc, ranks = model.rank_items(prof, None, items.cuda())
    assert torch.equal(ranks.cpu(), _oracle_ranks(S, elig, items))
    assert torch.equal(sc.cpu(), S.gather(1, items.cuda()).float().cpu())


# ---- real-valued tables: the fp32 path ------------------------------------------------------------------------------
@pytest.mark.parametrize("F,n_items,B", [(37, 2000, 9), (64, 3000, 66), (516, 5000, 17), (256, 300, 70), (260, 300, 70)])
def test_real_valued_within_bound(F, n_items, B):
    A = _real(n_items, F, F)
    model = _model(A)
    assert model.int8_table() is None
    p_x = _batch(B, 20, n_items, F + 1)
    prof = (p_x.cuda(), None, None)
    S, bound, elig = _oracle(A, p_x, p_x)
    sc, ids = model.recommend(prof, None, k=128)
    got = S.gather(1, ids.cuda())
    assert bool(((sc.cuda().double() - got).abs() <= bound.gather(1, ids.cuda()) + 1e-30).all())
    want_s, want_i = _oracle_topk(S, elig, 128)
    tol = 2 * bound.max().item()
    gap = torch.full_like(want_s, math.inf)  # a position is unambiguous when its oracle neighbours are farther than tol
    gap[:, 1:] = (want_s[:, 1:] - want_s[:, :-1]).abs()
    amb = (gap <= tol) | torch.cat([gap[:, 1:] <= tol, torch.zeros(B, 1, dtype=torch.bool)], 1)
    assert amb.float().mean() < 0.05
    assert torch.equal(ids.cpu()[~amb], want_i[~amb])
    items = _targets(B, 32, n_items, p_x, F + 2)
    sc, ranks = model.rank_items(prof, None, items.cuda())
    want_r = _oracle_ranks(S, elig, items)
    s_t = S.gather(1, items.cuda())
    near = ((S[:, None, :] - s_t[:, :, None]).abs() <= tol) & elig[:, None, :]
    slack = near.sum(-1).cpu()  # items whose order against the target the bound leaves open
    assert bool(((ranks.cpu() - want_r).abs() <= slack).all())
    assert bool(((sc.cuda().double() - s_t).abs() <= bound.gather(1, items.cuda()) + 1e-30).all())


# ---- recommend and rank_items agree bit for bit ---------------------------------------------------------------------
@pytest.mark.parametrize("table", ["multihot", "real"])
def test_recommend_rank_agreement(table):
    n_items, F, B = 4000, 96, 12
    A = _multihot(n_items, F, 0.05, 7) if table == "multihot" else _real(n_items, F, 7)
    model = _model(A)
    assert (model.int8_table() is not None) == (table == "multihot")
    p_x = _batch(B, 30, n_items, 8)
    g = torch.Generator().manual_seed(9)
    excl = torch.randint(0, n_items, (B, 300), generator=g)
    prof = (p_x.cuda(), None, None)
    for ex in ("profile", excl.cuda()):
        sc, ids = model.recommend(prof, None, k=128, exclude=ex)
        items = torch.cat([ids[:, :64], ids[:, :64]], 1)  # every listed item twice
        rs, ranks = model.rank_items(prof, None, items, exclude=ex)
        want = torch.arange(64, device="cuda").repeat(2)[None].expand(B, -1)
        assert torch.equal(ranks, want)
        assert torch.equal(rs.view(torch.int32), torch.cat([sc[:, :64], sc[:, :64]], 1).view(torch.int32))
        rs, ranks = model.rank_items(prof, None, ids, exclude=ex)
        assert torch.equal(ranks, torch.arange(128, device="cuda")[None].expand(B, -1))
        assert torch.equal(rs.view(torch.int32), sc.view(torch.int32))


# ---- agreement with KNN.forward, and dense mode with table mode -----------------------------------------------------
@pytest.mark.parametrize("table", ["multihot", "integer", "real"])
def test_forward_and_dense_agreement(table):
    n_items, F, B, L = 3000, 200, 20, 12
    g = torch.Generator().manual_seed(11)
    if table == "multihot":
        A = _multihot(n_items, F, 0.1, 11)
    elif table == "integer":  # max|x| = 20: 400 * 200 < 2^24
        A = torch.randint(-20, 21, (n_items, F), generator=g).float()
        A[0] = 0
    else:
        A = _real(n_items, F, 11)
    model = _model(A)
    assert (model.int8_table() is None) == (table == "real")
    p_x = _batch(B, L, n_items, 12)
    sc, ids = model.recommend((p_x.cuda(), None, None), None, k=100)
    y = model((p_x.cuda(), None, None), [(ids, None, None)])
    Ad = A.cuda()
    yd = model((p_x.cuda(), Ad[p_x.cuda()], None), [(ids, Ad[ids], None)])
    if table == "real":
        S, bound, _ = _oracle(A, p_x, p_x)
        b = bound.gather(1, ids).float()
        assert bool(((sc - y).abs() <= 2 * b + 1e-30).all()) and bool(((sc - yd).abs() <= 2 * b + 1e-30).all())
    else:
        assert torch.equal(sc, y) and torch.equal(sc, yd)
    # dense mode (the last slot's row of p_a; the fp32 path) against table mode (the i8 path for integer tables)
    p_a = Ad[p_x.cuda()]
    sc2, ids2 = model.recommend((p_x.cuda(), p_a, None), None, k=100)
    items = ids[:, :50]
    r1 = model.rank_items((p_x.cuda(), None, None), None, items)
    r2 = model.rank_items((p_x.cuda(), p_a, None), None, items)
    if table != "real":
        assert torch.equal(sc2, sc) and torch.equal(ids2, ids)
        assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])
    # rank_items in train mode gives the eval-mode result (KNN has no dropout)
    model.train()
    assert torch.equal(model.rank_items((p_x.cuda(), None, None), None, items)[1], r1[1])


# ---- ties: thousands of equal scores, ordered by id -----------------------------------------------------------------
def test_ties_order_by_id():
    n_items, F, B = 5000, 6, 16
    A = _multihot(n_items, F, 0.5, 21)
    model = _model(A)
    p_x = _batch(B, 10, n_items, 22)
    S, _, elig = _oracle(A, p_x, p_x)
    assert int((S == S.max(1, keepdim=True).values).sum(1).max()) > 100  # the top score is shared by many items
    sc, ids = model.recommend((p_x.cuda(), None, None), None, k=128)
    want_s, want_i = _oracle_topk(S, elig, 128)
    assert torch.equal(ids.cpu(), want_i) and torch.equal(sc.cpu(), want_s.float())
    for u in range(B):  # within a score, ascending id
        s, i = sc[u].cpu(), ids[u].cpu()
        same = s[1:] == s[:-1]
        assert bool((i[1:][same] > i[:-1][same]).all())
    items = torch.randint(1, n_items, (B, 128), generator=torch.Generator().manual_seed(23))
    assert torch.equal(model.rank_items((p_x.cuda(), None, None), None, items.cuda())[1].cpu(),
                       _oracle_ranks(S, elig, items))


# ---- edges ----------------------------------------------------------------------------------------------------------
def test_padding_and_everything_excluded():
    A = _multihot(50, 8, 0.5, 31)
    model = _model(A)
    p_x = _batch(3, 4, 50, 32)
    prof = (p_x.cuda(), None, None)
    sc, ids = model.recommend(prof, None, k=100, exclude=None)  # 49 eligible items
    S, _, elig = _oracle(A, p_x, None)
    want_s, want_i = _oracle_topk(S, elig, 100)
    assert torch.equal(ids.cpu(), want_i) and torch.equal(sc.cpu(), want_s.float())
    assert bool((ids[:, 49:] == 0).all()) and bool((sc[:, 49:] == 0).all())
    everything = torch.arange(50).repeat(3, 1).cuda()
    sc, ids = model.recommend(prof, None, k=10, exclude=everything)
    assert bool((ids == 0).all()) and bool((sc == 0).all())
    sc, ranks = model.rank_items(prof, None, torch.tensor([[1, 2], [3, 49], [7, 7]]).cuda(), exclude=everything)
    assert bool((ranks == 0).all())  # nothing eligible orders before anything


def test_empty_profile_gives_ids_one_to_k():
    A = _real(700, 40, 41)
    model = _model(A)
    p_x = torch.zeros(4, 8, dtype=torch.int64).cuda()
    sc, ids = model.recommend((p_x, None, None), None, k=128)
    assert torch.equal(ids, torch.arange(1, 129).repeat(4, 1).cuda()) and bool((sc == 0).all())
    _, ranks = model.rank_items((p_x, None, None), None, torch.tensor([[5, 699]] * 4).cuda())
    assert torch.equal(ranks.cpu(), torch.tensor([[4, 698]] * 4))


def test_invalid_ids_repeat_calls_and_long_profiles():
    n_items = 900
    A = _multihot(n_items, 64, 0.2, 51)
    model = _model(A)
    p_x = _batch(6, 200, n_items, 52)  # L = 200: only the last slot is scored
    p_x[0, -1] = n_items + 5  # an id outside the table: a zero query row
    prof = (p_x.cuda(), None, None)
    items = torch.tensor([[0, -1, n_items, 2 ** 31 + 3, -(2 ** 33), 5]] * 6, dtype=torch.int64)
    sc, ranks = model.rank_items(prof, None, items.cuda())
    assert bool((ranks[:, :5] == -1).all()) and bool((sc[:, :5] == 0).all())
    S, _, elig = _oracle(A, p_x, p_x)
    assert torch.equal(ranks[:, 5:].cpu(), _oracle_ranks(S, elig, items[:, 5:]))
    assert bool((S[0] == 0).all())
    a = model.recommend(prof, None, k=128)
    b = model.recommend(prof, None, k=128)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    want_s, want_i = _oracle_topk(S, elig, 128)
    assert torch.equal(a[1].cpu(), want_i)
    c = model.rank_items(prof, None, a[1])
    d = model.rank_items(prof, None, a[1])
    assert torch.equal(c[0], d[0]) and torch.equal(c[1], d[1])


# ---- a table past 2^32 bytes ----------------------------------------------------------------------------------------
def test_large_table_64bit_offsets():
    n_items, F, B = 270_000, 4096, 4
    assert n_items * F * 4 > 2 ** 32
    g = torch.Generator(device="cuda").manual_seed(61)
    A = torch.rand(n_items, F, generator=g, device="cuda")
    A[-3:] += 1  # the last rows win for every user: their scores are read through the largest offsets
    A[0] = 0
    model = KNN().cuda()
    model.register_attr_table(A)
    assert model.int8_table() is None
    p_x = torch.tensor([[1, 17], [2, 200_000], [3, 269_998], [4, 123_457]], device="cuda")
    sc, ids = model.recommend((p_x, None, None), None, k=10, exclude=None)
    q = A[p_x[:, -1]].double()
    S = torch.cat([q @ A[i:i + 32768].double().T for i in range(0, n_items, 32768)], 1)  # chunked fp64
    bound = 1e-6 * S  # entries >= 0: sum |a b| = the score
    got = S.gather(1, ids)
    assert bool(((sc.double() - got).abs() <= bound.gather(1, ids) + 1e-30).all())
    assert set(ids[:, :3].flatten().tolist()) == {n_items - 3, n_items - 2, n_items - 1}
    S[:, 0] = -math.inf
    assert torch.equal(ids[:, 0], S.argmax(1))
    items = torch.tensor([[n_items - 3, n_items - 2, n_items - 1, 1]] * B, device="cuda")
    rs, ranks = model.rank_items((p_x, None, None), None, items, exclude=None)
    top = torch.argsort(S[:, -3:], 1, descending=True)  # column j of items is row n_items - 3 + j
    assert torch.equal(ranks[:, :3].gather(1, top), torch.arange(3, device="cuda").repeat(B, 1))
    assert bool(((rs.double() - S.gather(1, items)).abs() <= bound.gather(1, items) + 1e-30).all())


# ---- the full-ranking evaluators ------------------------------------------------------------------------------------
def test_evaluators_on_knn():
    from carca_replication_amd.device_data import DeviceInteractions, DeviceLoader
    from carca_replication_amd.train import evaluate_full, evaluate_full_ranks, full_rank_metrics

    n_items, n_ctx, L, F = 300, 4, 12, 48
    rng = np.random.default_rng(71)
    profiles, ctxd = {}, {}
    for u in range(40):
        profiles[u] = [int(v) for v in rng.integers(1, n_items, size=int(rng.integers(3, 20)))]
        for it in profiles[u]:
            ctxd[(u, it)] = rng.random(n_ctx).astype(np.float32)
    A = _multihot(n_items, F, 0.15, 72)
    model = _model(A)
    loader = DeviceLoader(DeviceInteractions(profiles, ctxd, n_items), "test", batch_size=16, profile_seq_len=L,
                          target_seq_len=10)
    want = []
    for p_x, _, _, o_x, _, _, _ in loader:
        pos = o_x[:, :1].long()
        excl = torch.where(p_x.long() == pos, torch.zeros_like(pos), p_x.long())
        S, _, elig = _oracle(A, p_x.cpu(), excl)
        want.append(_oracle_ranks(S, elig, pos.cpu()))
    want = torch.cat(want).reshape(-1)
    ks = (1, 5, 10, 20)
    got = evaluate_full_ranks(model, loader, "cuda", ks=ks)
    ref = full_rank_metrics(want, ks)
    assert got["users"] == ref["users"] == len(want) and got["mean_rank"] == ref["mean_rank"]
    for k in ks:  # (hit counts are exact; the NDCG / MRR sums differ only in their float64 summation order)
        assert got[f"HR@{k}"] == ref[f"HR@{k}"]
        assert abs(got[f"NDCG@{k}"] - ref[f"NDCG@{k}"]) < 1e-12
    assert abs(got["MRR"] - ref["MRR"]) < 1e-12
    hr, ndcg = evaluate_full(model, loader, "cuda", 10)
    assert hr == got["HR@10"]
    assert abs(ndcg - got["NDCG@10"]) < 1e-6


# ---- errors ---------------------------------------------------------------------------------------------------------
def test_errors():
    model = KNN().cuda()
    p_x = torch.ones(2, 3, dtype=torch.int64).cuda()
    with pytest.raises(CarcaHipError, match="register_attr_table"):
        model.recommend((p_x, None, None), None, k=5)
    with pytest.raises(CarcaHipError, match="register_attr_table"):
        model.rank_items((p_x, None, None), None, p_x)
    model.register_attr_table(_multihot(20, 8, 0.5, 81).cuda())
    with pytest.raises(CarcaHipError, match="128"):
        model.recommend((p_x, None, None), None, k=129)
    with pytest.raises(CarcaHipError, match="128"):
        model.rank_items((p_x, None, None), None, torch.ones(2, 129, dtype=torch.int64).cuda())
