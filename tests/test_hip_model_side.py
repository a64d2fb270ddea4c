"""One catalogue.ModelSide serves several descriptors: the shared calls of catalogue.py, each handed
the SAME side, return the bits of the public CARCA methods, which build a side of their own -- and those are pinned to the
fp64 oracle by tests/test_hip_recommend.py and its siblings.  No tolerance: every comparison is torch.equal.  The shapes
are the smallest at which a full profile, left padding with an interior zero, an empty profile and every optional
model-side pointer (item_w, user_q, user_off, user_m) all take part."""
import functools

import pytest
import torch

from carca_replication_amd import _lib, catalogue
from tests.model_util import build_model

pytestmark = pytest.mark.gpu

N_ITEMS, N_CTX, N_ATTRS, G, B, L, K, M_TOP = 50, 6, 12, 24, 3, 8, 5, 3
MODELS = {"ca": dict(decoder="ca", residual_ca=True), "dot": dict(decoder="dot"),
          "wdot-l2": dict(decoder="wdot", l2_norm=True)}


@functools.lru_cache(maxsize=None)
def _setup(name):
    torch.manual_seed(5)
    model = build_model(dict(d=64, H=4, n_blocks=1, embedding="all", **MODELS[name]), N_ITEMS, G, N_CTX, N_ATTRS, L)
    model = model.cuda().eval()
    gen = torch.Generator().manual_seed(9)
    attrs = torch.rand(N_ITEMS, N_ATTRS, generator=gen)
    attrs[0] = 0
    model.embeds.register_attr_table(attrs.cuda())
    p_x = torch.tensor([[4, 9, 31, 2, 49, 17, 9, 23],   # full
                        [0, 0, 0, 12, 0, 7, 40, 1],     # left-padded, an interior zero
                        [0, 0, 0, 0, 0, 0, 0, 0]])      # all padding
    p_c = torch.rand(B, L, N_CTX, generator=gen) * (p_x != 0).unsqueeze(-1)
    ctx = torch.rand(B, N_CTX, generator=gen) + 0.25  # nonzero: the optional context rows change every score
    items = torch.tensor([[3, 0, N_ITEMS, 7, 7, 12, 49],  # 0, n_items (no item) and a repeated id
                          [1, 49, 20, 20, 0, 33, 5],
                          [N_ITEMS, 8, 8, 0, 41, 2, 19]])
    group_of = torch.arange(N_ITEMS) % 4  # groups 0..2; label 3 becomes "no group"
    group_of[group_of == 3] = -1
    groups = catalogue.ItemGroups(group_of.cuda(), n_groups=3)
    return model, (p_x.cuda(), None, p_c.cuda()), ctx.cuda(), items.cuda(), groups


def _equal(got, want):
    got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
    return len(got) == len(want) and all(g.dtype == w.dtype and torch.equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("name", list(MODELS))
def test_the_context_reaches_every_score(name):
    # (so a context row that desc() dropped could not hide behind context-free scores.  Per user with a profile, not per
    # pair: a dot decoder's context term is one small shift of the user's logits, which the sigmoid's fp32 rounding may
    # absorb for a single item but not for the whole list; the empty profile of a dot decoder scores with a zero row)
    model, prof, ctx, items, _ = _setup(name)
    a, b = model.score_items(prof, ctx, items)[:2], model.score_items(prof, torch.zeros_like(ctx), items)[:2]
    assert bool((a != b).any(dim=1).all())


@pytest.mark.parametrize("name", list(MODELS))
def test_one_side_serves_every_shared_call(name):
    model, prof, ctx, items, groups = _setup(name)
    with torch.no_grad():
        side = catalogue.carca_model_side(model, prof, ctx, "test")
    before = dict(side.fields)

    def one():
        return side

    first = catalogue.recommend("recommend", _lib.RecommendDesc, "carca_recommend", one, prof, K, "profile")
    assert _equal(first, model.recommend(prof, ctx, k=K))
    assert _equal(catalogue.rank_items("rank_items", _lib.RankDesc, "carca_rank_items", one, prof, items, "profile"),
                  model.rank_items(prof, ctx, items))
    assert _equal(catalogue.score_items("score_items", one, prof, items), model.score_items(prof, ctx, items))
    assert _equal(catalogue.recommend_from("recommend_from", one, prof, items, K, "profile"),
                  model.recommend_from(prof, ctx, items, k=K))
    assert _equal(catalogue.recommend_by_group("recommend_by_group", one, prof, groups, K, "profile"),
                  model.recommend_by_group(prof, ctx, groups, k=K))
    if name == "ca":
        assert _equal(catalogue.explain_top_slots("explain_top_slots", one, prof, items, M_TOP),
                      model.explain_top_slots(prof, ctx, items, m=M_TOP))
    # no call wrote into the side: the same fields, and the first call's bits again
    assert side.fields == before
    again = catalogue.recommend("recommend", _lib.RecommendDesc, "carca_recommend", one, prof, K, "profile")
    assert _equal(again, first) and _equal(again, model.recommend(prof, ctx, k=K))
