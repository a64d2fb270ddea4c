"""GPU tests of the diversity re-rank (csrc/mmr_rerank.hip): lam = 1 is recommend bit for bit; the tie
rule and the arithmetic on tables where every intermediate is exact; determinism and batch independence; the kernel's own
selection walked in float64 (tests/mmr_ref.py); the evaluator."""
import functools

import numpy as np
import pytest
import torch

from carca_replication_amd import CarcaHipError, catalogue, ops, train
from carca_replication_amd.catalogue import CandidateSet
from carca_replication_amd.modules import KNN
from tests import mmr_ref as R
from tests.test_hip_candidates import _prof
from tests.test_hip_recommend import _log, _setup

pytestmark = pytest.mark.gpu


# ---- 1. lam = 1 is recommend(k) ---------------------------------------------------------------------------------------
# name -> (d, H, embedding, decoder, n_ctx)
LAM1_MODELS = {"ca": (64, 2, "all", "ca", 6), "dot": (64, 2, "id", "dot", 0)}


@functools.lru_cache(maxsize=None)
def _model(name, n, B=6, L=16):
    d, H, emb, dec, n_ctx = LAM1_MODELS[name]
    _, _, _, batch, model = _setup(d, H, emb, dec, "identity", True, L, B, n, n_ctx, 1)
    prof, ctx = _prof(batch)
    return model, prof, ctx


def _same(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("name", list(LAM1_MODELS))
def test_lam_one_is_recommend(name):
    n = 300
    model, prof, ctx = _model(name, n)
    S = CandidateSet(torch.arange(3, n, 4), n, device="cuda")
    for k, pool in ((10, 128), (1, 1), (40, 40), (7, 64)):
        for metric in ("cosine", "dot"):
            for kw in (dict(), dict(exclude=None), dict(candidates=S), dict(exclude=None, candidates=S)):
                s, i, ild = model.recommend_diverse(prof, ctx, k=k, pool=pool, lam=1.0, metric=metric, **kw)
                _same((s, i), model.recommend(prof, ctx, k=k, **kw))
                assert ild.shape == (6,) and ild.dtype == torch.float32 and bool(torch.isfinite(ild).all())
    # fewer than k eligible items: six candidates (fewer still where the profile holds some), k = 10 of a pool of 16
    few = CandidateSet(torch.tensor([2, 5, 9, 11, 200, 299]), n, device="cuda")
    s, i, ild = model.recommend_diverse(prof, ctx, k=10, pool=16, lam=1.0, candidates=few)
    _same((s, i), model.recommend(prof, ctx, k=10, candidates=few))
    assert int((i != 0).sum(1).max()) <= 6 and not bool(s[i == 0].any())
    # ... and at another lam the same items come back, padded alike, with the scores recommend gave them
    s2, i2, _ = model.recommend_diverse(prof, ctx, k=10, pool=16, lam=0.3, candidates=few)
    assert torch.equal(i2.sort(1).values, i.sort(1).values) and torch.equal(s2.sort(1).values, s.sort(1).values)
    assert bool(((i2 != 0).to(torch.int64).diff(dim=1) <= 0).all())  # the padding comes last


def test_lam_one_with_a_tiny_catalogue():
    n = 9  # eight items, the profile's excluded: fewer than k = 10 eligible
    model, prof, ctx = _model("dot", n, 4, 6)
    s, i, ild = model.recommend_diverse(prof, ctx, k=10, pool=12, lam=1.0)
    _same((s, i), model.recommend(prof, ctx, k=10))
    assert bool((i == 0).any(1).all())


def _multihot(n, F, density, seed):
    g = torch.Generator().manual_seed(seed)
    A = (torch.rand(n, F, generator=g) < density).float()
    A[0] = 0
    return A


@pytest.mark.parametrize("F", [37, 512])
def test_knn_lam_one_is_recommend(F):
    n, B, L = 300, 8, 6
    A = _multihot(n, F, 0.2, F)
    model = KNN().cuda()
    model.register_attr_table(A.cuda())
    p_x = torch.from_numpy(np.random.default_rng(F).integers(1, n, size=(B, L))).cuda()
    for k, pool in ((10, 128), (128, 128), (5, 5)):
        for kw in (dict(), dict(exclude=None)):
            s, i, ild = model.recommend_diverse((p_x, None, None), k=k, pool=pool, lam=1.0, **kw)
            _same((s, i), model.recommend((p_x, None, None), None, k=k, **kw))
    # at any lam > 0 the first item is recommend's first (M = 0 at the first step, ties to the better pool position)
    s, i, ild = model.recommend_diverse((p_x, None, None), k=10, lam=0.5)
    s1, i1 = model.recommend((p_x, None, None), None, k=1)
    assert torch.equal(i[:, :1], i1) and torch.equal(s[:, :1], s1)


# ---- 2. tie rule and arithmetic, exact ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _int_table(n_cols):
    """A {0, 1} table [300, round4(n_cols) + 4] whose columns past n_cols hold 9 (they must not reach a product); rows
    40 .. 59 duplicate rows 20 .. 39."""
    n = 300
    X = torch.full((n, (n_cols + 3) // 4 * 4 + 4), 9.0)
    X[:, :n_cols] = _multihot(n, n_cols, 0.3, 100 + n_cols)
    X[40:60] = X[20:40]
    return X, X.cuda()


def _int_pool(n, B, P, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, 80, (B, P), generator=g)  # a narrow range: repeated ids and the duplicated rows are common
    s = torch.randint(0, 4, (B, P), generator=g).float()
    if P >= 5:
        ids[:, P // 2] = 0  # the padding id in the middle of the pool
        ids[:, 1] = n + 5  # out of range
        ids[::2, 3] = -4
        ids[:, P - 1] = ids[:, 0]  # a repeated id
    return s, ids


@pytest.mark.parametrize("P", [1, 5, 64, 128])
@pytest.mark.parametrize("n_cols", [37, 128, 130, 512])
def test_integer_tables_give_the_exact_path(n_cols, P):
    X, Xd = _int_table(n_cols)
    B = 16
    s, ids = _int_pool(X.shape[0], B, P, 7 * n_cols + P)
    for k in sorted({1, P}):
        want = R.greedy_int(X, ids, s, n_cols, k)
        ws, wi = R.gather_outputs(s, ids, want)
        gs, gi, ild = ops.mmr_rerank(s.cuda(), ids.cuda(), Xd, n_cols, k, lam=0.5, metric="dot", normalize=False)
        assert gs.dtype == torch.float32 and gi.dtype == torch.int64 and ild.dtype == torch.float32
        assert torch.equal(gi.cpu(), wi), (n_cols, P, k)
        assert torch.equal(gs.cpu(), ws)
        # the ILD sum is an integer below 2^24 here: one rounding, in the division
        G, valid = R.pool_sims(X, ids, n_cols, "dot")
        ild64 = R.greedy(G, s, valid, k, 0.5, normalize=False, forced=want)["ild"]
        assert bool(((ild.cpu().double() - ild64).abs() <= 2.0 ** -23 * ild64.abs()).all())
        if P >= 5:
            assert bool(((want >= 0).sum(1) < P).all())  # the invalid entries were there to skip
    # int32 pool ids are taken too
    gi32 = ops.mmr_rerank(s.cuda(), ids.cuda().to(torch.int32), Xd, n_cols, 1, lam=0.5, metric="dot", normalize=False)[1]
    assert torch.equal(gi32.cpu(), R.gather_outputs(s, ids, R.greedy_int(X, ids, s, n_cols, 1))[1])


# ---- 3. determinism and independence ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gauss(n_cols, seed=0, n=600, B=64, P=128):
    """(X [n, round4(n_cols)] rows N(0, 0.3^2), scores [B, P] = sigmoid of logits of std 1 in recommend's order, ids [B, P]
    distinct per user; user 3 carries an id 0 and an out-of-range id."""
    g = torch.Generator().manual_seed(1000 * seed + n_cols)
    X = torch.zeros(n, (n_cols + 3) // 4 * 4)
    X[:, :n_cols] = 0.3 * torch.randn(n, n_cols, generator=g)
    X[0] = 0
    ids = torch.stack([torch.randperm(n - 1, generator=g)[:P] + 1 for _ in range(B)])
    s = torch.sigmoid(torch.randn(B, P, generator=g)).sort(1, descending=True).values
    ids[3, 5], ids[3, 17] = 0, n + 2
    return X, s, ids


@pytest.mark.parametrize("n_cols", [90, 512])
def test_two_calls_and_a_permuted_batch(n_cols):
    X, s, ids = _gauss(n_cols)
    Xd, sd, idd = X.cuda(), s.cuda(), ids.cuda()
    a = ops.mmr_rerank(sd, idd, Xd, n_cols, 40, lam=0.5)
    b = ops.mmr_rerank(sd, idd, Xd, n_cols, 40, lam=0.5)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    perm = torch.randperm(s.shape[0], generator=torch.Generator().manual_seed(4)).cuda()
    c = ops.mmr_rerank(sd[perm], idd[perm], Xd, n_cols, 40, lam=0.5)
    assert all(torch.equal(x[perm], y) for x, y in zip(a, c))
    one = ops.mmr_rerank(sd[5:6], idd[5:6], Xd, n_cols, 40, lam=0.5)  # a user alone
    assert all(torch.equal(x[5:6], y) for x, y in zip(a, one))
    # a caller's reciprocal norms are the ones computed here
    d = ops.mmr_rerank(sd, idd, Xd, n_cols, 40, lam=0.5, rnorm=catalogue.row_rnorm(Xd, n_cols))
    assert all(torch.equal(x, y) for x, y in zip(a, d))


@pytest.mark.parametrize("n_cols", [37, 90, 130, 512])
def test_equal_rows_with_equal_scores_go_in_pool_order(n_cols):
    X, s, ids = _gauss(n_cols)
    X = X.clone()
    X[500:520] = X[7]  # twenty bitwise copies of one row
    B, P = 8, 64
    g = torch.Generator().manual_seed(n_cols)
    ids = ids[:B, :P].clone().clamp(1, 499)
    s = s[:B, :P].clone()
    at = torch.stack([torch.randperm(P, generator=g)[:20].sort().values for _ in range(B)])  # the copies' pool positions
    ids.scatter_(1, at, torch.stack([torch.randperm(20, generator=g) + 500 for _ in range(B)]))  # ... in a shuffled id order
    s.scatter_(1, at, torch.full((B, 20), 0.625))
    _, gi, _ = ops.mmr_rerank(s.cuda(), ids.cuda(), X.cuda(), n_cols, P, lam=0.4)
    gi = gi.cpu()
    for b in range(B):
        out = [int(v) for v in gi[b] if v >= 500]
        assert out == [int(v) for v in ids[b, at[b]]], b  # every copy returned, in pool order (neither id nor score order)


# ---- 4. the kernel's own selection, walked in float64 -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gauss_ref(n_cols):
    X, s, ids = _gauss(n_cols)
    G, valid = R.pool_sims(X, ids, n_cols, "cosine")
    return G, valid


@pytest.mark.parametrize("k", [10, 40, 128])
@pytest.mark.parametrize("lam", [0.3, 0.7])
@pytest.mark.parametrize("n_cols", [37, 64, 90, 130, 512])
def test_selection_is_optimal_at_every_step(n_cols, lam, k):
    X, s, ids = _gauss(n_cols)
    G, valid = _gauss_ref(n_cols)
    B, P = s.shape
    m = R.margin(n_cols)
    gs, gi, ild = (t.cpu() for t in ops.mmr_rerank(s.cuda(), ids.cuda(), X.cuda(), n_cols, k, lam=lam, metric="cosine"))
    pos = R.positions_of(gi, ids)
    n_valid = valid.sum(1)
    assert torch.equal((pos >= 0).sum(1), n_valid.clamp(max=k))
    assert bool(((pos >= 0).to(torch.int64).diff(dim=1) <= 0).all())  # padding last
    ws, wi = R.gather_outputs(s, ids, pos)
    assert torch.equal(gs, ws) and torch.equal(gi, wi)  # the pool's bits at the returned positions
    walk = R.greedy(G, s, valid, k, lam, forced=pos)  # (asserts that every step takes a live entry)
    worst = float(walk["deficit"].max())
    print(f"n_cols {n_cols} lam {lam} k {k}: worst deficit {worst:.3e}, margin {m:.3e}, "
          f"ild err {float((ild.double() - walk['ild']).abs().max()):.3e}")
    assert worst <= m
    assert bool(((ild.double() - walk["ild"]).abs() <= m).all())
    if k == P:
        for b in range(B):
            assert sorted(gi[b][gi[b] != 0].tolist()) == sorted(ids[b][valid[b]].tolist())
    if k == 10 and n_cols <= 130:
        ref = R.greedy(G, s, valid, k, lam)
        near = float((ref["gap"] <= m).any(1).float().mean())
        same = float((ref["pos"] == pos).all(1).float().mean())
        print(f"  near-tie users in the reference {near:.3f}, identical paths {same:.3f}")
        assert near <= 0.10
        assert same >= 0.90


# ---- 5. the evaluator ---------------------------------------------------------------------------------------------------
def test_evaluate_full_diverse():
    from carca_replication_amd.device_data import DeviceInteractions, DeviceLoader

    n, n_ctx, L, k = 300, 6, 16, 10
    model, _, _ = _model("ca", n)
    profiles, ctxd = _log(24, n, n_ctx, 3)
    loader = DeviceLoader(DeviceInteractions(profiles, ctxd, n), "test", batch_size=8, profile_seq_len=L, target_seq_len=10)
    hr, ndcg = train.evaluate_full(model, loader, "cuda", k)
    got = train.evaluate_full_diverse(model, loader, "cuda", k, lam=1.0)
    assert got[f"HR@{k}"] == hr and got[f"NDCG@{k}"] == ndcg and got["users"] == 24
    for c in (None, CandidateSet(torch.arange(1, n, 2), n, device="cuda")):
        kw = {} if c is None else dict(candidates=c)
        got = train.evaluate_full_diverse(model, loader, "cuda", k, pool=64, lam=0.5, **kw)
        assert set(got) == {f"HR@{k}", f"NDCG@{k}", f"ILD@{k}", f"coverage@{k}", "users"}
        ild_sum, users, seen = 0.0, 0, set()
        for p_x, p_a, p_c, o_x, _, o_c, _ in loader:
            pos = o_x[:, :1].long()
            excl = torch.where(p_x.long() == pos, torch.zeros_like(pos), p_x.long())
            _, ids, ild = model.recommend_diverse((p_x, p_a, p_c), o_c[:, 0], k=k, pool=64, lam=0.5, exclude=excl, **kw)
            inside = torch.ones_like(pos, dtype=torch.bool) if c is None else c.contains(pos)
            ild_sum += float(ild[inside.reshape(-1)].double().sum())
            users += int(inside.sum())
            seen |= set(ids[inside.reshape(-1)].reshape(-1).tolist())
        assert got["users"] == users
        assert abs(got[f"ILD@{k}"] - ild_sum / users) <= 1e-6
        assert got[f"coverage@{k}"] == len(seen - {0}) / (n - 1)
        lam1 = train.evaluate_full_diverse(model, loader, "cuda", k, pool=64, lam=1.0, **kw)
        assert (lam1[f"HR@{k}"], lam1[f"NDCG@{k}"]) == train.evaluate_full(model, loader, "cuda", k, **kw)
    knn = KNN().cuda()
    knn.register_attr_table(_multihot(n, 48, 0.2, 1).cuda())
    with pytest.raises(CarcaHipError, match="candidate"):
        train.evaluate_full_diverse(knn, loader, "cuda", k, candidates=torch.arange(1, 50))
    got = train.evaluate_full_diverse(knn, loader, "cuda", k, lam=1.0)
    assert (got[f"HR@{k}"], got[f"NDCG@{k}"]) == train.evaluate_full(knn, loader, "cuda", k)
