"""CARCA.recommend / rank_items restricted to a candidate set S (carca_recommend_among / carca_rank_items_among, DESIGN.md
section 15) and train.evaluate_full / evaluate_full_ranks with candidates=S.  Two references: the fp64 CPU oracle of
tests/test_hip_recommend.py with the complement of S added to its exclusion sets (top-k), and the UNRESTRICTED calls
themselves (bits of the scores; exact ranks among S as counts over each item's unrestricted rank, no tolerance)."""
import functools

import numpy as np
import pytest
import torch

from carca_replication_amd import CarcaHipError
from carca_replication_amd.catalogue import CandidateSet
from tests.test_hip_recommend import _check, _excl_sets, _oracle_scores, _oracle_topk, _setup

pytestmark = pytest.mark.gpu


def _draw(n_items, c, seed):
    """c distinct ids of [1, n_items), ids 1 and n_items - 1 among them (as far as c allows), in a shuffled order."""
    rng = np.random.default_rng(seed)
    forced = [1, n_items - 1][:min(2, c)]
    rest = rng.choice(np.arange(2, n_items - 1), size=c - len(forced), replace=False)
    ids = np.concatenate([np.array(forced, dtype=np.int64), rest.astype(np.int64)])
    rng.shuffle(ids)
    return torch.from_numpy(ids)


def _skipped_share(full, k):
    """The share of compared positions at which tests.test_hip_recommend._check does not compare ids (an oracle neighbour
    within 1e-5)."""
    skipped = total = 0
    for s in full:
        for r in range(min(k, s.numel())):
            lo = float(s[r - 1] - s[r]) if r > 0 else 1.0
            hi = float(s[r] - s[r + 1]) if r + 1 < s.numel() else 1.0
            total += 1
            skipped += min(lo, hi) <= 1e-5
    return skipped / max(total, 1)


def _prof(batch):
    p_x, p_c, ctx = batch
    return (p_x.cuda(), None, p_c.float().cuda()), ctx.float().cuda()


# ---- 1. the oracle ---------------------------------------------------------------------------------------------------
# (d, H, embedding, decoder, encoding, residual_ca, L, B, n_items, k, n_ctx, n_blocks, l2, |S|)
ORACLE_CASES = [
    (64, 4, "all", "ca", "identity", True, 16, 5, 300, 10, 6, 1, False, 40),
    (90, 3, "all", "ca", "identity", True, 50, 5, 4097, 100, 6, 2, False, 257),
    (62, 2, "id", "ca", "positional", True, 17, 5, 300, 128, 0, 1, False, 256),
    (128, 4, "all", "ca", "learnable", True, 64, 5, 300, 128, 6, 1, False, 1),
    (64, 2, "id", "dot", "identity", True, 16, 5, 300, 100, 0, 1, False, 255),
    (96, 2, "all", "wdot", "positional", True, 17, 5, 4097, 128, 6, 1, True, 600),
]
S_SEED = 11


def _oracle_want(cfg, P, attrs, batch, n, S, k):
    p_x = batch[0]
    outside = set(range(1, n)) - set(S.tolist())
    excl = [e | outside for e in _excl_sets(p_x)]
    return _oracle_topk(_oracle_scores(cfg, P, attrs, batch, n), excl, k)


@pytest.mark.parametrize("case", ORACLE_CASES, ids=[f"{c[0]}x{c[1]}-{c[2]}-{c[3]}{'-l2' if c[12] else ''}-n{c[8]}-k{c[9]}-"
                                                    f"S{c[13]}" for c in ORACLE_CASES])
def test_recommend_among_matches_oracle(case):
    d, H, emb, dec, enc, res, L, B, n, k, n_ctx, nb, l2, c = case
    cfg, P, attrs, batch, model = _setup(d, H, emb, dec, enc, res, L, B, n, n_ctx, nb, l2)
    S = _draw(n, c, S_SEED)
    ws, wi, full = _oracle_want(cfg, P, attrs, batch, n, S, k)
    share = _skipped_share(full, k)
    print(f"skipped share of compared positions: {share:.4f}")
    assert share <= 0.10, share  # the id comparison below must cover at least 90 % of the positions
    prof, ctx = _prof(batch)
    got = model.recommend(prof, ctx, k=k, candidates=S.cuda())
    _check(got, (ws, wi), full, k)
    inside = set(S.tolist()) | {0}
    assert set(got[1].cpu().reshape(-1).tolist()) <= inside


# ---- the three models of the bit tests -------------------------------------------------------------------------------
MODELS = {
    "ca": (64, 4, "all", "ca", "identity", True, 16, 6, False),
    "dot": (64, 2, "id", "dot", "identity", True, 16, 0, False),
    "wdot-l2": (96, 2, "all", "wdot", "positional", True, 17, 6, True),
}


@functools.lru_cache(maxsize=None)
def _model(name, n, B=5):
    d, H, emb, dec, enc, res, L, n_ctx, l2 = MODELS[name]
    cfg, P, attrs, batch, model = _setup(d, H, emb, dec, enc, res, L, B, n, n_ctx, 1, l2)
    prof, ctx = _prof(batch)
    return model, prof, ctx, batch[0]


def _targets(n, B, N, seed):
    it = torch.from_numpy(np.random.default_rng(seed).integers(1, n, size=(B, N)))
    it[0, 0], it[0, 1], it[0, 2], it[B - 1, N - 1] = 0, n + 3, it[0, 3], -7
    return it


# ---- 2. the whole catalogue as the candidate set: today's bits ---------------------------------------------------------
@pytest.mark.parametrize("n", [300, 4097])
@pytest.mark.parametrize("name", list(MODELS))
def test_all_items_as_candidates_keeps_the_bits(name, n):
    model, prof, ctx, p_x = _model(name, n)
    S = torch.arange(1, n).cuda()
    for k in (10, 128):
        a, b = model.recommend(prof, ctx, k=k), model.recommend(prof, ctx, k=k, candidates=S)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    items = _targets(n, 5, 101, 3).cuda()
    for excl in ("profile", None):
        a = model.rank_items(prof, ctx, items, exclude=excl)
        b = model.rank_items(prof, ctx, items, exclude=excl, candidates=S)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 3. a returned item's score is the unrestricted call's, bit for bit ------------------------------------------------
@pytest.mark.parametrize("name", list(MODELS))
def test_scores_keep_their_bits(name):
    n = 4097
    model, prof, ctx, p_x = _model(name, n)
    S = _draw(n, 128, 5).cuda()
    s, i = model.recommend(prof, ctx, k=128, candidates=S)
    s_all, _ = model.rank_items(prof, ctx, i)
    live = i != 0
    assert int(live.sum()) >= 5 * 100
    assert torch.equal(s[live], s_all[live]) and not bool(s[~live].any())


# ---- 4. exact ranks among S from the unrestricted ranks ----------------------------------------------------------------
def _unrestricted_ranks(model, prof, ctx, n, exclude):
    """[B, n] int64 on the CPU: rank_items' rank of every id (column 0: -1), from ceil(n / 128) calls."""
    B = prof[0].shape[0]
    ids = torch.zeros((n + 127) // 128 * 128, dtype=torch.int64)
    ids[:n] = torch.arange(n)
    cols = [model.rank_items(prof, ctx, chunk.expand(B, -1).contiguous().cuda(), exclude=exclude)[1].cpu()
            for chunk in ids.split(128)]
    return torch.cat(cols, 1)[:, :n]


def _ranks_among(ur, excluded, S, items):
    """rank_among(t) = #{s in S, not excluded : ur(s) < ur(t)}; -1 for id 0 and ids outside the catalogue."""
    B, n = ur.shape
    in_s = torch.zeros(n, dtype=torch.bool)
    in_s[S] = True
    want = torch.full(items.shape, -1, dtype=torch.int64)
    for b in range(B):
        elig = in_s.clone()
        if excluded[b]:
            elig[sorted(excluded[b])] = False
        for j, t in enumerate(items[b].tolist()):
            if 1 <= t < n:
                want[b, j] = int((elig & (ur[b] < ur[b, t])).sum())
    return want


@functools.lru_cache(maxsize=None)
def _rank_fixture(mode):
    n, B = 300, 5
    model, prof, ctx, p_x = _model("ca", n)
    rng = np.random.default_rng(21)
    if mode == "profile":
        exclude, excluded = "profile", _excl_sets(p_x)
    else:  # an explicit [B, 7] list: zeros, a duplicate, ids inside and outside S (S always holds 1 and n - 1)
        ex = torch.from_numpy(rng.integers(1, n, size=(B, 7)))
        ex[:, 0], ex[:, 1], ex[:, 2], ex[:, 3] = 0, 1, ex[:, 4], n - 1
        exclude, excluded = ex.cuda(), [set(ex[b].tolist()) - {0} for b in range(B)]
    return model, prof, ctx, p_x, exclude, excluded, _unrestricted_ranks(model, prof, ctx, n, exclude)


@pytest.mark.parametrize("c", [1, 40, 256, 257, 299])
@pytest.mark.parametrize("mode", ["profile", "list"])
def test_exact_ranks_among_candidates(mode, c):
    n, B = 300, 5
    model, prof, ctx, p_x, exclude, excluded, ur = _rank_fixture(mode)
    assert not bool(p_x[1].any()) and int((p_x[2] != 0).sum()) == 1  # an empty and a one-item profile
    S = _draw(n, c, 30 + c)
    in_s = set(S.tolist())
    out_s = sorted(set(range(1, n)) - in_s) or [0]
    items = _targets(n, B, 24, 40 + c)
    for b in range(B):  # targets inside S, outside S, excluded (in and out of S), repeated; 0 and out of range are in
        items[b, 5], items[b, 6], items[b, 7] = S[b % c], S[(b + 3) % c], out_s[b % len(out_s)]
        ex = sorted(excluded[b])
        if ex:
            items[b, 8], items[b, 9] = ex[0], ex[-1]
        items[b, 10] = items[b, 5]
    want = _ranks_among(ur, excluded, S, items)
    scores, ranks = model.rank_items(prof, ctx, items.cuda(), exclude=exclude, candidates=CandidateSet(S.cuda(), n))
    assert ranks.dtype == torch.int64 and torch.equal(ranks.cpu(), want)
    assert int(want[0, 0]) == -1 and int(want[0, 1]) == -1 and int(want.max()) <= c
    s_all, _ = model.rank_items(prof, ctx, items.cuda(), exclude=exclude)
    assert torch.equal(scores, s_all)


# ---- 5. recommend and rank_items agree under the same set --------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODELS))
def test_recommend_and_rank_items_agree(name):
    n, k = 4097, 100
    model, prof, ctx, p_x = _model(name, n)
    S = CandidateSet(_draw(n, 600, 8).cuda(), n)
    s, i = model.recommend(prof, ctx, k=k, candidates=S)
    s2, r = model.rank_items(prof, ctx, i, candidates=S)
    assert bool((i != 0).all())
    assert torch.equal(r, torch.arange(k, device=r.device).expand_as(r)) and torch.equal(s, s2)


# ---- 6. edges ----------------------------------------------------------------------------------------------------------
def test_fewer_eligible_candidates_than_k():
    n = 300
    model, prof, ctx, p_x = _model("ca", n)
    S = torch.tensor([7, 50, 120, 200, 299])
    ex = torch.tensor([[50, 0, 299]] * 5).cuda()
    s, i = model.recommend(prof, ctx, k=10, exclude=ex, candidates=S.cuda())
    assert all(sorted(i[b, :3].tolist()) == [7, 120, 200] for b in range(5))
    assert not bool(i[:, 3:].any()) and not bool(s[:, 3:].any()) and bool((s[:, :3] > 0).all())
    _, r = model.rank_items(prof, ctx, i[:, :3].contiguous(), exclude=ex, candidates=S.cuda())
    assert torch.equal(r.cpu(), torch.arange(3).expand(5, 3))


def test_empty_candidate_set():
    n = 300
    model, prof, ctx, p_x = _model("ca", n)
    for S in (torch.zeros(0, dtype=torch.int64).cuda(), CandidateSet(torch.tensor([0, n, -3]).cuda(), n)):
        s, i = model.recommend(prof, ctx, k=10, candidates=S)
        assert s.shape == (5, 10) and not bool(s.any()) and not bool(i.any())
        items = _targets(n, 5, 9, 2).cuda()
        s2, r = model.rank_items(prof, ctx, items, candidates=S)
        valid = (items >= 1) & (items < n)
        assert torch.equal(r, torch.where(valid, 0, -1)) and torch.equal(s2, model.rank_items(prof, ctx, items)[0])


def test_more_users_than_user_chunks():
    n, B = 300, 300
    model, prof, ctx, p_x = _model("ca", n, B)
    S = torch.sort(_draw(n, 40, 9)).values
    # S in the unrestricted order, from one rank_items call over S (no exclusion: 40 distinct ranks per user)
    s_all, r_all = model.rank_items(prof, ctx, S.expand(B, -1).contiguous().cuda(), exclude=None)
    order = torch.argsort(r_all, dim=1)
    s, i = model.recommend(prof, ctx, k=40, exclude=None, candidates=S.cuda())
    assert torch.equal(i, S.cuda()[order]) and torch.equal(s, torch.gather(s_all, 1, order))
    _, r = model.rank_items(prof, ctx, i, exclude=None, candidates=S.cuda())
    assert torch.equal(r, torch.arange(40, device=r.device).expand(B, 40))


def test_reproducible_and_raw_tensor_equals_candidate_set():
    n = 4097
    model, prof, ctx, p_x = _model("wdot-l2", n)
    raw = _draw(n, 257, 4)
    S = CandidateSet(raw.cuda(), n)
    items = _targets(n, 5, 33, 6).cuda()
    mask = torch.zeros(n, dtype=torch.bool)
    mask[raw] = True
    a, ra = model.recommend(prof, ctx, k=128, candidates=S), model.rank_items(prof, ctx, items, candidates=S)
    for other in (S, raw.cuda(), raw.to(torch.int32).cuda(), mask.cuda(), raw):  # (a CPU tensor is moved to the device)
        b, rb = model.recommend(prof, ctx, k=128, candidates=other), model.rank_items(prof, ctx, items, candidates=other)
        assert all(torch.equal(x, y) for x, y in zip(a + ra, b + rb))


def test_argument_errors_at_the_call():
    n = 300
    model, prof, ctx, p_x = _model("ca", n)
    with pytest.raises(CarcaHipError, match="n_items = 301"):
        model.recommend(prof, ctx, k=10, candidates=CandidateSet(torch.tensor([1, 2]).cuda(), n + 1))
    for bad in (torch.tensor([1.0, 2.0]), torch.tensor([[1, 2]]), torch.zeros(n - 1, dtype=torch.bool)):
        with pytest.raises(CarcaHipError):
            model.rank_items(prof, ctx, torch.ones(5, 1, dtype=torch.int64).cuda(), candidates=bad.cuda())


def test_follows_weight_updates():
    from carca_replication_amd.optim import Adam

    n, k, c = 300, 10, 40
    cfg, P, attrs, batch, model = _setup(64, 4, "all", "ca", "learnable", True, 16, 5, n, 6, 1)
    prof, ctx = _prof(batch)
    S = _draw(n, c, 12)
    cand = CandidateSet(S.cuda(), n)
    ws, wi, full = _oracle_want(cfg, P, attrs, batch, n, S, k)
    _check(model.recommend(prof, ctx, k=k, candidates=cand), (ws, wi), full, k)
    model.train()
    opt = Adam(model.parameters(), lr=1e-2)
    with torch.no_grad():
        for p in model.parameters():
            p.grad = torch.randn_like(p) * 0.1
    opt.step()
    model.eval()
    P2 = {k_: v.detach().double().cpu() for k_, v in model.state_dict().items()}
    ws2, wi2, full2 = _oracle_want(cfg, P2, attrs, batch, n, S, k)
    assert not torch.equal(wi, wi2)
    _check(model.recommend(prof, ctx, k=k, candidates=cand), (ws2, wi2), full2, k)


# ---- 7. evaluation -----------------------------------------------------------------------------------------------------
def test_evaluators_among_candidates():
    from carca_replication_amd import train
    from carca_replication_amd.modules import KNN

    n, B, L, n_ctx, ks = 300, 5, 16, 6, (1, 5, 10, 50)
    cfg, P, attrs, batch, model = _setup(64, 4, "all", "ca", "identity", True, L, B, n, n_ctx, 1)
    rng = np.random.default_rng(17)
    S = _draw(n, 150, 13)
    in_s = torch.zeros(n, dtype=torch.bool)
    in_s[S] = True
    loader, want = [], []
    for seed in (0, 1, 2):
        p_x = torch.from_numpy(rng.integers(1, n, size=(B, L)))
        p_x[0, :L - 2] = 0
        p_c = torch.from_numpy(rng.random((B, L, n_ctx))).float() * (p_x != 0).unsqueeze(-1)
        o_x = torch.from_numpy(rng.integers(1, n, size=(B, 3)))
        o_x[1, 0] = p_x[1, -1]  # a positive that is also a profile item: not excluded
        o_c = torch.from_numpy(rng.random((B, 3, n_ctx))).float()
        loader.append((p_x, attrs.float()[p_x], p_c, o_x, attrs.float()[o_x], o_c, torch.zeros_like(o_x)))
        prof = (p_x.cuda(), None, p_c.cuda())
        pos = o_x[:, :1]
        excl = torch.where(p_x == pos, torch.zeros_like(pos), p_x)
        ur = _unrestricted_ranks(model, prof, o_c[:, 0].cuda(), n, excl.cuda())
        r = _ranks_among(ur, [set(excl[b].tolist()) - {0} for b in range(B)], S, pos)
        want.append(torch.where(in_s[pos], r, torch.full_like(r, -1)))
    want = torch.cat(want)
    n_in = int((want >= 0).sum())
    assert 0 < n_in < want.numel()  # some positives are outside S
    exp = train.full_rank_metrics(want, ks)
    cand = CandidateSet(S, n)  # (a CPU set: the evaluators move it)
    for c in (cand, S.cuda()):
        got = train.evaluate_full_ranks(model, loader, "cuda", ks, candidates=c)
        assert got["users"] == exp["users"] == n_in
        assert all(abs(got[key] - exp[key]) <= 1e-12 * max(1.0, abs(exp[key])) for key in exp), (got, exp)
        for k in (5, 50):  # (fp32 sums of at most 15 terms <= 1, each within 1e-7 relative: well inside 1e-6)
            hr, ndcg = train.evaluate_full(model, loader, "cuda", k, candidates=c)
            assert abs(hr - exp[f"HR@{k}"]) <= 1e-6 and abs(ndcg - exp[f"NDCG@{k}"]) <= 1e-6
    # candidates=None is today's call; the whole catalogue as the set changes nothing
    base = train.evaluate_full_ranks(model, loader, "cuda", ks)
    assert base["users"] == want.numel()
    assert train.evaluate_full_ranks(model, loader, "cuda", ks, candidates=None) == base
    assert train.evaluate_full_ranks(model, loader, "cuda", ks, candidates=torch.arange(1, n)) == base
    assert train.evaluate_full(model, loader, "cuda", 10, candidates=torch.arange(1, n)) == \
        train.evaluate_full(model, loader, "cuda", 10)
    with pytest.raises(CarcaHipError, match="KNN"):
        train.evaluate_full_ranks(KNN().cuda(), loader, "cuda", ks, candidates=cand)
