"""CARCA.recommend_by_group / recommend_capped (carca_recommend_groups / carca_recommend_capped).
No tolerance anywhere: every comparison is torch.equal against calls that tests/test_hip_recommend.py and
tests/test_hip_candidates.py pin to the fp64 oracle -- recommend(candidates=) per group, rank_items for the exact order
behind the capped list, score_items for a listed item's score."""
import functools

import numpy as np
import pytest
import torch

from carca_replication_amd.catalogue import CandidateSet, ItemGroups
from tests.test_hip_candidates import MODELS, _model, _prof
from tests.test_hip_recommend import _excl_sets, _setup

pytestmark = pytest.mark.gpu


# ---- the layouts: membership scattered over the ids by a seeded permutation ---------------------------------------------
def _scatter(n, sizes, ungrouped, seed):
    """group_of [n]: 1 .. n - 1 permuted, with id 1 first and id n - 1 last, dealt out in order -- sizes[g] ids to group g
    (-1: a gap of `ungrouped` ids without a label; None: everything that is left)."""
    rng = np.random.default_rng(seed)
    ids = [1] + (rng.permutation(np.arange(2, n - 1))).tolist() + [n - 1]
    fixed = sum(s for s in sizes if s not in (None, -1)) + ungrouped
    group_of = torch.full((n,), -1, dtype=torch.int64)
    at, g = 0, 0
    for s in sizes:
        if s == -1:
            at += ungrouped
            continue
        take = len(ids) - fixed if s is None else s
        group_of[torch.tensor(ids[at:at + take], dtype=torch.int64)] = g
        at, g = at + take, g + 1
    assert at == len(ids)
    return group_of


@functools.lru_cache(maxsize=None)
def _layout(name):
    """-> (n_items, ItemGroups on the GPU, sizes by group)."""
    if name == "A":  # 0, 1, 9, 10, 11, 64, 0 and the rest minus 20 ungrouped ids; id 1 in group 1, id 299 in group 7
        n, G = 300, 8
        group_of = _scatter(n, (1, 9, 10, 11, 64, -1, None), 20, 5)
        group_of[group_of >= 0] += 1  # group 0 is empty
        group_of[group_of == 6] = 7   # and so is group 6, the last but one
        sizes = [0, 1, 9, 10, 11, 64, 0, 299 - 95 - 20]
        assert int(group_of[1]) == 1 and int(group_of[299]) == 7
    elif name == "B":  # both selection regimes and their boundary in one call
        n, G = 4097, 5
        group_of = _scatter(n, (1024, 1025, 256, 257, None), 0, 6)
        sizes = [1024, 1025, 256, 257, 4096 - 2562]
    elif name == "C":  # one group holding every item
        n, G = 300, 1
        group_of, sizes = torch.zeros(n, dtype=torch.int64), [299]
    else:  # "D": every item is its own group
        n, G = 300, 299
        group_of, sizes = torch.arange(n) - 1, [1] * 299
    gr = ItemGroups(group_of.cuda(), n_groups=G)
    assert [gr.members(g).numel() for g in range(G)] == sizes
    return n, gr, sizes


def _explicit(n, gr, B):
    """[B, 5] exclusion rows: a grouped id, an ungrouped one (where the layout has any: else a second grouped id), 0 and a
    duplicate."""
    labels = gr.group_of.cpu()
    grouped = torch.nonzero(labels >= 0).reshape(-1)
    loose = torch.nonzero(labels < 0).reshape(-1)[1:]  # (without id 0)
    rng = np.random.default_rng(31)
    ex = torch.zeros(B, 5, dtype=torch.int64)
    for b in range(B):
        ex[b, 0] = grouped[rng.integers(len(grouped))]
        ex[b, 1] = loose[rng.integers(len(loose))] if len(loose) else grouped[rng.integers(len(grouped))]
        ex[b, 3] = ex[b, 0]
        ex[b, 4] = grouped[rng.integers(len(grouped))]
    return ex


def _per_group(model, prof, ctx, gr, k, exclude, **kw):
    """[B, G, k] from G calls of the merged API."""
    rows = [model.recommend(prof, ctx, k=k, exclude=exclude, candidates=CandidateSet(gr.members(g), gr.n_items), **kw)
            for g in range(gr.n_groups)]
    return torch.stack([r[0] for r in rows], 1), torch.stack([r[1] for r in rows], 1)


def _same(got, want):
    return got[0].dtype == torch.float32 and got[1].dtype == torch.int64 and got[0].shape == want[0].shape and \
        torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- 1. by group against the merged API ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODELS))
@pytest.mark.parametrize("layout,ks", [("A", (10,)), ("B", (10, 128))])
def test_by_group_equals_recommend_per_group(layout, ks, name):
    n, gr, sizes = _layout(layout)
    model, prof, ctx, p_x = _model(name, n)
    B = p_x.shape[0]
    for exclude in ("profile", None, _explicit(n, gr, B).cuda()):
        for k in ks:
            got = model.recommend_by_group(prof, ctx, gr, k=k, exclude=exclude)
            assert tuple(got[0].shape) == (B, gr.n_groups, k)
            assert _same(got, _per_group(model, prof, ctx, gr, k, exclude))
            for g, size in enumerate(sizes):
                if size == 0:  # an empty group is all padding
                    assert not bool(got[0][:, g].any()) and not bool(got[1][:, g].any())
                elif exclude is None:  # nothing excluded: min(k, size) items, all of the group, then padding
                    ids = got[1][:, g]
                    assert bool((ids[:, :min(k, size)] != 0).all()) and not bool(ids[:, min(k, size):].any())
                    assert bool((gr.group_of[ids[:, :min(k, size)]] == g).all())


def test_excluding_a_whole_group_leaves_padding():
    n, gr, sizes = _layout("A")
    model, prof, ctx, p_x = _model("ca", n)
    B = p_x.shape[0]
    ex = torch.zeros(B, 9, dtype=torch.int64, device="cuda")
    ex[0] = gr.members(2)
    s, i = model.recommend_by_group(prof, ctx, gr, k=10, exclude=ex)
    assert not bool(s[0, 2].any()) and not bool(i[0, 2].any())
    assert bool((i[1:, 2, :9] != 0).all()) and not bool(i[1:, 2, 9:].any())
    assert _same((s, i), _per_group(model, prof, ctx, gr, 10, ex))


# ---- 2. one group, and one group per item -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODELS))
def test_one_group_is_recommend(name):
    n, gr, _ = _layout("C")
    model, prof, ctx, p_x = _model(name, n)
    for k in (10, 128):
        s, i = model.recommend_by_group(prof, ctx, gr, k=k)
        ws, wi = model.recommend(prof, ctx, k=k)
        assert torch.equal(s, ws.unsqueeze(1)) and torch.equal(i, wi.unsqueeze(1))


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("name", list(MODELS))
def test_one_group_per_item(name, k):
    n, gr, _ = _layout("D")
    model, prof, ctx, p_x = _model(name, n)
    B = p_x.shape[0]
    s, i = model.recommend_by_group(prof, ctx, gr, k=k)  # (exclude="profile")
    want = torch.arange(1, n).expand(B, -1).clone()
    for b, e in enumerate(_excl_sets(p_x)):
        want[b, torch.tensor(sorted(e), dtype=torch.int64) - 1] = 0
    assert int((want == 0).sum()) > 0
    assert torch.equal(i[:, :, 0].cpu(), want)
    assert torch.equal(s[:, :, 0], model.score_items(prof, ctx, want.cuda()))
    assert not bool(s[:, :, 1:].any()) and not bool(i[:, :, 1:].any())


# ---- 3. / 6. ties -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _twins():
    """Items 7 and 40 with equal attribute rows under an embedding that reads no id: equal table rows, equal logit bits."""
    n, B = 300, 5
    cfg, P, attrs, batch, model = _setup(64, 4, "attr", "ca", "identity", True, 16, B, n, 6, 1)
    twin = attrs.clone()
    twin[40] = twin[7]
    model.embeds.register_attr_table(twin.float().cuda())
    prof, ctx = _prof(batch)
    both = torch.tensor([[7, 40]] * B).cuda()
    sc = model.score_items(prof, ctx, both)
    assert torch.equal(sc[:, 0], sc[:, 1])
    return n, B, model, prof, ctx


def test_tie_inside_a_group_goes_to_the_smaller_id():
    n, B, model, prof, ctx = _twins()
    group_of = torch.full((n,), -1, dtype=torch.int64)
    group_of[1:] = torch.arange(1, n) % 10  # 7 and 40 do not share a residue:
    group_of[40] = 7                        # ... so 40 joins 7's group, of 31 items
    gr = ItemGroups(group_of.cuda())
    assert gr.members(7).numel() == 31
    s, i = model.recommend_by_group(prof, ctx, gr, k=31, exclude=None)
    for b in range(B):
        row = i[b, 7].tolist()
        assert row.index(40) == row.index(7) + 1, row


def test_tie_across_groups_goes_to_the_smaller_id():
    """40's group has the smaller index, so 40 comes first in the grouped order: a merge keyed on the position would put it
    in front of 7.  Four large groups give at most 20 of the list, so both twins are in it for every user."""
    n, B, model, prof, ctx = _twins()
    group_of = 2 + torch.arange(n) % 4
    group_of[40], group_of[7] = 0, 1
    gr = ItemGroups(group_of.cuda())
    assert int(gr.pos_of[40]) < int(gr.pos_of[7])
    s, i = model.recommend_capped(prof, ctx, gr, k=30, max_per_group=5, exclude=None)
    for b in range(B):
        row = i[b].tolist()
        assert row.index(40) == row.index(7) + 1, row
        assert row[22:] == [0] * 8 and 0 not in row[:22]


# ---- 4. capped against an exact order -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _exact_ranks(layout, name, mode):
    """-> (excluded sets, ranks [B, C] on the CPU of the grouped ids, in gr.order's order): rank_items' integer position
    of each id among the grouped items, in recommend's order with its id tie rule (an excluded id still gets one)."""
    n, gr, _ = _layout(layout)
    model, prof, ctx, p_x = _model(name, n)
    B = p_x.shape[0]
    if mode == "profile":
        exclude, excluded = "profile", _excl_sets(p_x)
    else:
        ex = _explicit(n, gr, B)
        exclude, excluded = ex.cuda(), [set(ex[b].tolist()) - {0} for b in range(B)]
    cand = CandidateSet(gr.order, n)
    cols = [model.rank_items(prof, ctx, chunk.expand(B, -1).contiguous(), exclude=exclude, candidates=cand)[1].cpu()
            for chunk in gr.order.split(128)]
    return exclude, excluded, torch.cat(cols, 1)


def _walk(ranks, order, group_of, excluded, k, m):
    """The capped list from the exact order, on the CPU: ids [B, k], padded with 0."""
    want = torch.zeros(ranks.shape[0], k, dtype=torch.int64)
    for b in range(ranks.shape[0]):
        elig = sorted((int(r), i) for r, i in zip(ranks[b].tolist(), order) if i not in excluded[b])
        assert len({r for r, _ in elig}) == len(elig)  # a strict order
        taken, row = {}, []
        for _, i in elig:
            g = group_of[i]
            if taken.get(g, 0) < m:
                taken[g] = taken.get(g, 0) + 1
                row.append(i)
                if len(row) == k:
                    break
        want[b, :len(row)] = torch.tensor(row, dtype=torch.int64)
    return want


@pytest.mark.parametrize("mode", ["profile", "list"])
@pytest.mark.parametrize("name", list(MODELS))
@pytest.mark.parametrize("layout", ["A", "B"])
def test_capped_matches_the_walk_over_the_exact_order(layout, name, mode):
    n, gr, _ = _layout(layout)
    model, prof, ctx, p_x = _model(name, n)
    exclude, excluded, ranks = _exact_ranks(layout, name, mode)
    order, group_of = gr.order.tolist(), gr.group_of.tolist()
    for m in (1, 2, 10):
        s, i = model.recommend_capped(prof, ctx, gr, k=10, max_per_group=m, exclude=exclude)
        want = _walk(ranks, order, group_of, excluded, 10, m)
        assert i.dtype == torch.int64 and torch.equal(i.cpu(), want), (m, i.cpu(), want)
        assert torch.equal(s, model.score_items(prof, ctx, want.cuda()))  # (id 0 scores 0)
    assert int((want != 0).sum()) == want.numel()  # m = 10: no cap, ten items each


# ---- 5. capped identities -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODELS))
@pytest.mark.parametrize("layout", ["A", "B"])
def test_inactive_cap_is_recommend_among_the_grouped_items(layout, name):
    n, gr, _ = _layout(layout)
    model, prof, ctx, p_x = _model(name, n)
    cand = CandidateSet(torch.sort(gr.order).values, n)
    for k, m in ((10, 10), (10, 500), (128, 128)):
        assert _same(model.recommend_capped(prof, ctx, gr, k=k, max_per_group=m), model.recommend(prof, ctx, k=k, candidates=cand))


@pytest.mark.parametrize("name", list(MODELS))
def test_cap_on_one_group_truncates_recommend(name):
    n, gr, _ = _layout("C")
    model, prof, ctx, p_x = _model(name, n)
    k, m = 10, 4
    s, i = model.recommend_capped(prof, ctx, gr, k=k, max_per_group=m)
    ws, wi = model.recommend(prof, ctx, k=m)
    assert torch.equal(s[:, :m], ws) and torch.equal(i[:, :m], wi) and bool((wi != 0).all())
    assert not bool(s[:, m:].any()) and not bool(i[:, m:].any())


@pytest.mark.parametrize("name", list(MODELS))
def test_cap_of_one_on_singleton_groups_is_recommend(name):
    n, gr, _ = _layout("D")
    model, prof, ctx, p_x = _model(name, n)
    for k in (10, 128):
        assert _same(model.recommend_capped(prof, ctx, gr, k=k, max_per_group=1), model.recommend(prof, ctx, k=k))


# ---- 7. reproducible; many users; long profiles; weight updates ---------------------------------------------------------
@pytest.mark.parametrize("layout", ["A", "B"])
def test_two_calls_are_identical(layout):
    n, gr, _ = _layout(layout)
    model, prof, ctx, p_x = _model("wdot-l2", n)
    assert _same(model.recommend_by_group(prof, ctx, gr, k=128), model.recommend_by_group(prof, ctx, gr, k=128))
    for m in (1, 3):
        assert _same(model.recommend_capped(prof, ctx, gr, k=128, max_per_group=m),
                     model.recommend_capped(prof, ctx, gr, k=128, max_per_group=m))


def test_more_users_than_a_sweep_user_chunk():
    n, gr, _ = _layout("A")
    model, prof, ctx, p_x = _model("ca", n, 70)
    got = model.recommend_by_group(prof, ctx, gr, k=10)
    assert _same(got, _per_group(model, prof, ctx, gr, 10, "profile"))
    cand = CandidateSet(torch.sort(gr.order).values, n)
    assert _same(model.recommend_capped(prof, ctx, gr, k=10, max_per_group=10), model.recommend(prof, ctx, k=10, candidates=cand))
    # the cap: no group more than twice, best first, and the first two items are the uncapped call's
    s, i = model.recommend_capped(prof, ctx, gr, k=10, max_per_group=2)
    labels = gr.group_of.cpu()
    assert bool((i != 0).all()) and bool((s[:, 1:] <= s[:, :-1]).all())
    assert all(int(np.bincount(labels[i[b].cpu()].numpy()).max()) <= 2 for b in range(70))
    assert torch.equal(i[:, :2], model.recommend(prof, ctx, k=2, candidates=cand)[1])


def test_long_profile_composed():
    n, gr, _ = _layout("A")
    cfg, P, attrs, batch, model = _setup(64, 4, "all", "ca", "identity", True, 65, 3, n, 6, 1)
    prof, ctx = _prof(batch)
    got = model.recommend_by_group(prof, ctx, gr, k=10, allow_composed=True)
    assert _same(got, _per_group(model, prof, ctx, gr, 10, "profile", allow_composed=True))
    cand = CandidateSet(torch.sort(gr.order).values, n)
    assert _same(model.recommend_capped(prof, ctx, gr, k=10, max_per_group=10, allow_composed=True),
                 model.recommend(prof, ctx, k=10, candidates=cand, allow_composed=True))


def test_follows_weight_updates():
    from carca_replication_amd.optim import Adam

    n, gr, _ = _layout("A")
    cfg, P, attrs, batch, model = _setup(64, 4, "all", "ca", "learnable", True, 16, 5, n, 6, 1)
    prof, ctx = _prof(batch)
    before = model.recommend_by_group(prof, ctx, gr, k=10), model.recommend_capped(prof, ctx, gr, k=10, max_per_group=2)
    assert _same(before[0], _per_group(model, prof, ctx, gr, 10, "profile"))
    model.train()
    opt = Adam(model.parameters(), lr=1e-2)
    with torch.no_grad():
        for p in model.parameters():
            p.grad = torch.randn_like(p) * 0.1
    opt.step()
    model.eval()
    after = model.recommend_by_group(prof, ctx, gr, k=10), model.recommend_capped(prof, ctx, gr, k=10, max_per_group=2)
    assert not torch.equal(before[0][1], after[0][1]) and not torch.equal(before[1][1], after[1][1])
    assert _same(after[0], _per_group(model, prof, ctx, gr, 10, "profile"))
    cand = CandidateSet(torch.sort(gr.order).values, n)
    assert _same(model.recommend_capped(prof, ctx, gr, k=10, max_per_group=10), model.recommend(prof, ctx, k=10, candidates=cand))
