"""CARCA.score_items / recommend_from (a candidate list of its own per user: carca_score_lists / carca_recommend_lists,
DESIGN.md section 21) and train.evaluate_listed.  Three references: the fp64 CPU oracle of tests/test_hip_recommend.py
with every id outside a user's list added to that user's exclusion set; the existing calls themselves (rank_items' scores
and the single-user recommend(candidates=...), bit for bit); and tests/lists_ref.py over score_items' own output
(selection alone, exact)."""
import numpy as np
import pytest
import torch

from carca_replication_amd import CarcaHipError, catalogue
from tests.lists_ref import lists_topk, positive_rank
from tests.test_hip_candidates import MODELS, _model, _skipped_share
from tests.test_hip_recommend import _check, _excl_sets, _log, _oracle_scores, _oracle_topk, _setup

pytestmark = pytest.mark.gpu


def _draw_lists(n, B, N, p_x=None):
    """[B, N] ids drawn with replacement (duplicates occur by themselves), then an id 0, an id outside the catalogue, a
    forced duplicate and a negative id, then a profile item that exclude="profile" must drop -- each where the shape has
    the entry."""
    it = torch.from_numpy(np.random.default_rng(23).integers(1, n, size=(B, N)))
    if N >= 4:
        it[0, 0], it[0, 1], it[0, 2], it[B - 1, N - 1] = 0, n + 3, it[0, 3], -7
    if p_x is not None and B > 3 and N > 5:
        it[3, 5] = p_x[3, -1]
    return it


def _prof(batch):
    p_x, p_c, ctx = batch
    return (p_x.cuda(), None, p_c.float().cuda()), ctx.float().cuda()


def _uniq(row, n):
    """the distinct valid ids of one list row, ascending"""
    return torch.unique(row[(row >= 1) & (row < n)])


def _single_user(model, prof, ctx, u, k, exclude, cand, **kw):
    ex = exclude[u:u + 1] if isinstance(exclude, torch.Tensor) else exclude
    return model.recommend((prof[0][u:u + 1], None, prof[2][u:u + 1]), None if ctx is None else ctx[u:u + 1], k=k, exclude=ex,
                           candidates=cand.cuda(), **kw)


def _equals_single_user_calls(model, prof, ctx, items, n, k, exclude, **kw):
    s, i = model.recommend_from(prof, ctx, items.cuda(), k=k, exclude=exclude, **kw)
    for u in range(items.shape[0]):
        ws, wi = _single_user(model, prof, ctx, u, k, exclude, _uniq(items[u], n), **kw)
        assert torch.equal(s[u], ws[0]) and torch.equal(i[u], wi[0]), (u, k, exclude if isinstance(exclude, str) else "tensor")
    return s, i


# ---- 1. the oracle ---------------------------------------------------------------------------------------------------
# (d, H, embedding, decoder, encoding, residual_ca, L, B, n_items, k, n_ctx, n_blocks, l2, N)
ORACLE_CASES = [
    (64, 4, "all", "ca", "identity", True, 16, 5, 300, 10, 6, 1, False, 101),
    (90, 3, "all", "ca", "identity", True, 50, 5, 4097, 100, 6, 2, False, 1025),
    (62, 2, "id", "ca", "positional", True, 17, 5, 300, 128, 0, 1, False, 256),
    (128, 4, "all", "ca", "learnable", True, 64, 5, 300, 128, 6, 1, False, 1024),
    (64, 2, "id", "dot", "identity", True, 16, 5, 300, 100, 0, 1, False, 257),
    (96, 2, "all", "wdot", "positional", True, 17, 5, 4097, 128, 6, 1, True, 3000),
]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=[f"{c[0]}x{c[1]}-{c[2]}-{c[3]}{'-l2' if c[12] else ''}-n{c[8]}-k{c[9]}-"
                                                    f"N{c[13]}" for c in ORACLE_CASES])
def test_lists_match_oracle(case):
    d, H, emb, dec, enc, res, L, B, n, k, n_ctx, nb, l2, N = case
    cfg, P, attrs, batch, model = _setup(d, H, emb, dec, enc, res, L, B, n, n_ctx, nb, l2)
    p_x = batch[0]
    items = _draw_lists(n, B, N, p_x)
    y = _oracle_scores(cfg, P, attrs, batch, n)
    everything = set(range(1, n))
    excl = [e | (everything - set(items[b].tolist())) for b, e in enumerate(_excl_sets(p_x))]
    ws, wi, full = _oracle_topk(y, excl, k)
    share = _skipped_share(full, k)
    print(f"skipped share of compared positions: {share:.4f}; eligible per user: {[s.numel() for s in full]}")
    assert share <= 0.10, share  # the id comparison below must cover at least 90 % of the positions
    prof, ctx = _prof(batch)
    got = model.recommend_from(prof, ctx, items.cuda(), k=k)
    _check(got, (ws, wi), full, k)
    assert int(p_x[3, -1]) not in got[1][3].tolist()
    s = model.score_items(prof, ctx, items.cuda()).cpu()
    assert s.shape == (B, N) and s.dtype == torch.float32
    valid = (items >= 1) & (items < n)
    want = torch.gather(y, 1, (items.clamp(1, n - 1) - 1))
    err = float((s.double() - want)[valid].abs().max())
    print(f"score_items: largest error at a valid entry {err:.3e}")
    assert err < 2e-5
    assert not bool(s[~valid].any()) and int((~valid).sum()) >= 3


# ---- 2. bits against the existing calls --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODELS))
def test_scores_are_rank_items_bits(name):
    n = 4097
    model, prof, ctx, p_x = _model(name, n)
    items = _draw_lists(n, 5, 101, p_x).cuda()
    assert torch.equal(model.score_items(prof, ctx, items), model.rank_items(prof, ctx, items, exclude=None)[0])
    items = _draw_lists(n, 5, 300, p_x).cuda()
    want = torch.cat([model.rank_items(prof, ctx, items[:, lo:lo + 100].contiguous(), exclude=None)[0]
                      for lo in (0, 100, 200)], 1)
    assert torch.equal(model.score_items(prof, ctx, items), want)
    assert torch.equal(model.score_items(prof, ctx, items.to(torch.int32)), want)


@pytest.mark.parametrize("N", [101, 300])
@pytest.mark.parametrize("name", list(MODELS))
def test_rows_are_single_user_recommend_bits(name, N):
    n = 4097
    model, prof, ctx, p_x = _model(name, n)
    items = _draw_lists(n, 5, N, p_x)
    ex = items[:, 10:17].clone()  # an explicit list: ids of the user's own list, a zero, an id outside the catalogue
    ex[:, 0], ex[:, 1] = 0, n + 1
    for exclude in ("profile", None, ex.cuda()):
        for k in (10, 128):
            _equals_single_user_calls(model, prof, ctx, items, n, k, exclude)


@pytest.mark.parametrize("name", list(MODELS))
def test_one_list_for_everybody_is_recommend_among(name):
    n = 4097
    model, prof, ctx, p_x = _model(name, n)
    S = torch.from_numpy(np.random.default_rng(5).choice(np.arange(1, n), size=200, replace=False))
    for k in (10, 128):
        a = model.recommend_from(prof, ctx, S.expand(5, -1).contiguous().cuda(), k=k)
        b = model.recommend(prof, ctx, k=k, candidates=S.cuda())
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 3. the two paths agree ------------------------------------------------------------------------------------------
def _both_paths(monkeypatch, call):
    assert catalogue.LIST_FUSED_MAX == 1024
    a = call()
    monkeypatch.setattr(catalogue, "LIST_FUSED_MAX", 0)
    b = call()
    monkeypatch.undo()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    return a


@pytest.mark.parametrize("N", [1, 255, 256, 257, 1024])
@pytest.mark.parametrize("name", list(MODELS))
def test_fused_and_split_paths_agree(monkeypatch, name, N):
    n = 4097
    model, prof, ctx, p_x = _model(name, n)
    items = _draw_lists(n, 5, N, p_x).cuda()
    for k in (10, 128):
        s, i = _both_paths(monkeypatch, lambda: model.recommend_from(prof, ctx, items, k=k))
        assert int((i != 0).sum()) >= min(k, N) - 1  # (the draw leaves at least that many eligible in some row)


@pytest.mark.parametrize("name", list(MODELS))
def test_natural_boundary(name):
    n = 4097
    model, prof, ctx, p_x = _model(name, n)
    items = _draw_lists(n, 5, 1024, p_x)
    longer = torch.cat([items, items[:, :1]], 1)  # 1025 columns: the split path, the same distinct ids
    for k in (10, 128):
        a = model.recommend_from(prof, ctx, items.cuda(), k=k)
        b = model.recommend_from(prof, ctx, longer.cuda(), k=k)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 4. edge lists ---------------------------------------------------------------------------------------------------
def test_edge_lists(monkeypatch):
    n, B, k = 300, 5, 10
    model, prof, ctx, p_x = _model("ca", n)
    # one id repeated: one result and k - 1 pads
    rep = torch.full((B, 40), 17)
    s, i = _both_paths(monkeypatch, lambda: model.recommend_from(prof, ctx, rep.cuda(), k=k, exclude=None))
    assert torch.equal(i[:, 0].cpu(), rep[:, 0]) and not bool(i[:, 1:].any()) and not bool(s[:, 1:].any())
    assert torch.equal(s[:, 0], model.score_items(prof, ctx, rep.cuda())[:, 0])
    # only invalid ids
    bad = torch.tensor([[0, -3, n, n + 5, 0, -(2 ** 40)]] * B)
    s, i = _both_paths(monkeypatch, lambda: model.recommend_from(prof, ctx, bad.cuda(), k=k))
    assert not bool(s.any()) and not bool(i.any())
    assert not bool(model.score_items(prof, ctx, bad.cuda()).any())
    # every valid id excluded
    lst = torch.tensor([[5, 9, 9, 0, 250, 31]] * B)
    s, i = _both_paths(monkeypatch, lambda: model.recommend_from(prof, ctx, lst.cuda(), k=k, exclude=lst.cuda()))
    assert not bool(s.any()) and not bool(i.any())
    # fewer eligible items than k
    ex = torch.tensor([[9, 0]] * B)
    s, i = _both_paths(monkeypatch, lambda: model.recommend_from(prof, ctx, lst.cuda(), k=k, exclude=ex.cuda()))
    assert all(sorted(i[b, :3].tolist()) == [5, 31, 250] for b in range(B))
    assert not bool(i[:, 3:].any()) and not bool(s[:, 3:].any()) and bool((s[:, :3] > 0).all())
    assert bool((s[:, :2] >= s[:, 1:3]).all())


def test_tie_goes_to_the_smaller_id(monkeypatch):
    """Two items whose attribute rows are equal, under an embedding that reads no id: equal table rows, equal logit bits."""
    n, B, k = 300, 5, 30
    cfg, P, attrs, batch, model = _setup(64, 4, "attr", "ca", "identity", True, 16, B, n, 6, 1)
    twin = attrs.clone()
    twin[40] = twin[7]
    model.embeds.register_attr_table(twin.float().cuda())
    prof, ctx = _prof(batch)
    items = _draw_lists(n, B, 30, batch[0])
    items[:, 8], items[:, 20] = 40, 7  # the larger id first in caller order
    sc = model.score_items(prof, ctx, items.cuda())
    assert torch.equal(sc[:, 8], sc[:, 20])
    s, i = _both_paths(monkeypatch, lambda: model.recommend_from(prof, ctx, items.cuda(), k=k, exclude=None))
    for b in range(B):
        row = i[b].tolist()
        assert row.index(40) == row.index(7) + 1, row


# ---- 5. long profiles ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [300, 1100])
@pytest.mark.parametrize("L", [65, 130])
def test_long_profiles(L, N):
    n, B = 300, 3
    cfg, P, attrs, batch, model = _setup(64, 4, "all", "ca", "identity", True, L, B, n, 6, 1)
    p_x, p_c, ctx = batch
    if L == 130:  # one user with every slot valid (three chunks); user 1 has none
        rng = np.random.default_rng(9)
        p_x[0] = torch.from_numpy(rng.integers(1, n, size=L))
        p_c[0] = torch.from_numpy(rng.random((L, 6)))
        assert int((p_x[0] != 0).sum()) == 130
    assert not bool(p_x[1].any())
    prof, c = _prof((p_x, p_c, ctx))
    items = _draw_lists(n, B, N, None)
    got = model.score_items(prof, c, items.cuda(), allow_composed=True)
    want = torch.cat([model.rank_items(prof, c, chunk.contiguous().cuda(), exclude=None, allow_composed=True)[0]
                      for chunk in items.split(128, dim=1)], 1)
    assert torch.equal(got, want)
    for exclude in ("profile", None):
        _equals_single_user_calls(model, prof, c, items, n, 20, exclude, allow_composed=True)


# ---- 6. more users than CUs ------------------------------------------------------------------------------------------
def test_more_users_than_cus():
    """Selection alone, against tests/lists_ref.py over score_items' own output.  On the MI355X 2 of the 2600 compared
    positions lie inside a tie of linked scores (two logits that round to one sigmoid), and those two ids differ from the
    reference's; every other id is compared exactly."""
    n, B, N, k = 300, 260, 40, 10
    model, prof, ctx, p_x = _model("dot", n, B)
    items = _draw_lists(n, B, N, p_x)
    sc = model.score_items(prof, ctx, items.cuda()).cpu()
    excluded = _excl_sets(p_x)
    ws, wi = lists_topk(sc, items, n, k + 1, excluded=excluded)  # (one more: the neighbour below position k - 1)
    s, i = (t.cpu() for t in model.recommend_from(prof, ctx, items.cuda(), k=k))
    # The link is monotone, so the score sequence is the reference's exactly.  The reference orders by the LINKED score,
    # the kernel by the logit: two logits that round to one linked score are a tie to the reference alone, so an id is
    # compared wherever its linked score differs from both neighbours' -- and everywhere the id must be an eligible
    # one of the user's list, taken once, carrying exactly the score reported for it.
    assert torch.equal(s, ws[:, :k])
    tied = differ = 0
    for u in range(B):
        own = {int(items[u, j]): float(sc[u, j]) for j in range(N)}
        row = [int(v) for v in i[u] if int(v) != 0]
        assert len(set(row)) == len(row) == int((wi[u, :k] != 0).sum())
        for r, v in enumerate(row):
            assert 1 <= v < n and v not in excluded[u] and own[v] == float(s[u, r]), (u, r)
            clear = (r == 0 or ws[u, r - 1] != ws[u, r]) and (ws[u, r] != ws[u, r + 1] or wi[u, r + 1] == 0)
            tied += not clear
            differ += v != int(wi[u, r])
            assert not clear or v == int(wi[u, r]), (u, r)
    print(f"positions inside a tie of linked scores: {tied} of {B * k}; ids that differ from the reference's there: {differ}")


# ---- 7. housekeeping -------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits(monkeypatch):
    n = 4097
    model, prof, ctx, p_x = _model("ca", n)
    for N in (300, 1500):
        items = _draw_lists(n, 5, N, p_x).cuda()
        a, b = model.recommend_from(prof, ctx, items, k=50), model.recommend_from(prof, ctx, items, k=50)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert torch.equal(model.score_items(prof, ctx, items), model.score_items(prof, ctx, items))


def test_follows_weight_updates():
    from carca_replication_amd.optim import Adam

    n, k, N = 300, 10, 60
    cfg, P, attrs, batch, model = _setup(64, 4, "all", "ca", "learnable", True, 16, 5, n, 6, 1)
    prof, ctx = _prof(batch)
    items = _draw_lists(n, 5, N, batch[0])
    everything = set(range(1, n))
    excl = [e | (everything - set(items[b].tolist())) for b, e in enumerate(_excl_sets(batch[0]))]

    def want(params):
        return _oracle_topk(_oracle_scores(cfg, params, attrs, batch, n), excl, k)

    ws, wi, full = want(P)
    _check(model.recommend_from(prof, ctx, items.cuda(), k=k), (ws, wi), full, k)
    model.train()
    opt = Adam(model.parameters(), lr=1e-2)
    with torch.no_grad():
        for p in model.parameters():
            p.grad = torch.randn_like(p) * 0.1
    opt.step()
    model.eval()
    P2 = {k_: v.detach().double().cpu() for k_, v in model.state_dict().items()}
    ws2, wi2, full2 = want(P2)
    assert not torch.equal(wi, wi2)
    _check(model.recommend_from(prof, ctx, items.cuda(), k=k), (ws2, wi2), full2, k)


def test_argument_errors_at_the_call():
    n, B = 300, 5
    model, prof, ctx, p_x = _model("ca", n)
    items = _draw_lists(n, B, 20, p_x).cuda()
    for call in (lambda it: model.score_items(prof, ctx, it), lambda it: model.recommend_from(prof, ctx, it)):
        model.train()
        try:
            with pytest.raises(CarcaHipError, match="eval"):
                call(items)
        finally:
            model.eval()
        for bad in (items.float(), items[0], items[:B - 1], items[:, :0]):
            with pytest.raises(CarcaHipError, match="items"):
                call(bad)
    for k in (0, 129):
        with pytest.raises(CarcaHipError, match="128"):
            model.recommend_from(prof, ctx, items, k=k)
    with pytest.raises(CarcaHipError, match="exclude"):
        model.recommend_from(prof, ctx, items, exclude="history")
    long = (torch.ones(B, 65, dtype=torch.int64).cuda(), None, torch.zeros(B, 65, 6).cuda())
    with pytest.raises(CarcaHipError, match="64"):
        model.recommend_from(long, ctx, items)
    with pytest.raises(CarcaHipError, match="64"):
        model.score_items(long, ctx, items)


# ---- 8. the loader's own protocol --------------------------------------------------------------------------------------
def test_evaluate_listed_matches_reference_and_evaluate():
    """HR@10 / NDCG@10 of train.evaluate_listed against (a) sums this test takes from score_items over o_x with
    tests/lists_ref.py, exact up to the fp32 sum of 24 terms, and (b) train.evaluate over the users whose positive is more
    than 1e-5 away from every other candidate in forward's scores (observed share of such users: 1.00 of 24, log seed 3)."""
    from carca_replication_amd import train
    from carca_replication_amd.device_data import DeviceInteractions, DeviceLoader

    n_items, n_ctx, L, k = 200, 6, 16, 10
    cfg, P, attrs, _, model = _setup(64, 2, "all", "ca", "identity", True, L, 2, n_items, n_ctx, 1)
    profiles, ctxd = _log(24, n_items, n_ctx, 3)
    log = DeviceInteractions(profiles, ctxd, n_items)
    loader = DeviceLoader(log, "test", batch_size=8, profile_seq_len=L, target_seq_len=10)
    batches = [tuple(None if t is None else t.clone() for t in b) for b in loader]  # epoch 0's negatives
    hr = ndcg = 0.0
    users, clear_batches, n_clear = 0, [], 0
    for p_x, _, p_c, o_x, _, o_c, y in batches:
        sc = model.score_items((p_x, None, p_c), o_c[:, 0], o_x).cpu()
        _, ids = lists_topk(sc, o_x.cpu(), n_items, k)
        rank = positive_rank(ids, o_x[:, 0].cpu())
        hr += float((rank >= 0).sum())
        ndcg += float((1.0 / torch.log2(rank[rank >= 0].float() + 2.0)).sum())
        users += p_x.shape[0]
        with torch.no_grad():
            yf = model((p_x, None, p_c), [(o_x, None, o_c)]).reshape(p_x.shape[0], -1)
        clear = ((yf[:, 1:] - yf[:, :1]).abs() > 1e-5).all(dim=1)
        n_clear += int(clear.sum())
        if bool(clear.any()):
            clear_batches.append(tuple(None if t is None else t[clear] for t in (p_x, None, p_c, o_x, None, o_c, y)))
    share = n_clear / users
    print(f"users whose positive is clear of its neighbours: {n_clear} of {users} ({share:.2f})")
    assert users == 24 and share >= 0.9
    loader.epoch = 0  # (negatives are re-drawn per epoch: the same draw as `batches`)
    got = train.evaluate_listed(model, loader, "cuda", k)
    print(f"evaluate_listed: HR@{k} {got[0]:.6f} NDCG@{k} {got[1]:.6f}; reference {hr / users:.6f} {ndcg / users:.6f}")
    assert abs(got[0] - hr / users) <= 1e-6 and abs(got[1] - ndcg / users) <= 1e-6
    assert train.evaluate_listed(model, batches, "cuda", k) == got
    a = train.evaluate_listed(model, clear_batches, "cuda", k)
    b = train.evaluate(model, clear_batches, "cuda", k)
    assert abs(a[0] - b[0]) <= 1e-6 and abs(a[1] - b[1]) <= 1e-6
