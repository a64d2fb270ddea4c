"""CARCA.score_items_at / best_context / recommend_at (several request contexts per user: carca_score_lists_at /
carca_recommend_at / carca_recommend_among_at).  Two references: the single-context calls themselves,
bit for bit (slice c of a result is the call at contexts[:, c]), and the fp64 CPU oracle of tests/test_hip_recommend.py
run once per context."""
import functools

import numpy as np
import pytest
import torch

from carca_replication_amd import CarcaHipError
from carca_replication_amd.catalogue import CandidateSet
from tests.test_hip_candidates import _skipped_share
from tests.test_hip_recommend import _check, _excl_sets, _oracle_scores, _oracle_topk, _setup
from tests.test_hip_recommend_lists import _draw_lists

pytestmark = pytest.mark.gpu

B, N_CTX = 5, 6
# (d, H, embedding, decoder, encoding, residual_ca, L, n_blocks, l2)
MODELS = {
    "64x4-all-ca": (64, 4, "all", "ca", "identity", True, 16, 1, False),
    "90x3-all-ca": (90, 3, "all", "ca", "identity", True, 50, 2, False),
    "128x1-attrctx-ca": (128, 1, "attrctx", "ca", "learnable", False, 64, 1, False),
    "64x2-all-dot": (64, 2, "all", "dot", "identity", True, 16, 1, False),
    "96x2-all-wdot-l2": (96, 2, "all", "wdot", "positional", True, 17, 1, True),
}
CONTEXT_COUNTS = (1, 3, 8, 9)  # 9 crosses a pass boundary of eight contexts


@functools.lru_cache(maxsize=None)
def _case(name, n):
    """(cfg, P, attrs, batch, model, the profile on the device) of a model over n items: built once, never changed."""
    d, H, emb, dec, enc, res, L, nb, l2 = MODELS[name]
    cfg, P, attrs, batch, model = _setup(d, H, emb, dec, enc, res, L, B, n, N_CTX, nb, l2)
    p_x, p_c, _ = batch
    return cfg, P, attrs, batch, model, (p_x.cuda(), None, p_c.float().cuda())


def _contexts(ctx, C, seed=41):
    cs = np.random.default_rng(seed).random((ctx.shape[0], C, ctx.shape[1]))
    cs[:, 0] = ctx
    if C > 2:
        cs[:, 2] = cs[:, 0]  # a duplicate
    if C > 3:
        cs[:, 3] = 0  # an all-zero context
    return cs


def _device_contexts(batch, C):
    """the contexts as float64 for the oracle and as float32 on the device"""
    X64 = torch.from_numpy(_contexts(batch[2].numpy(), C))
    return X64, X64.float().cuda()


# ---- 1. bits against the single-context calls -------------------------------------------------------------------------
@pytest.mark.parametrize("C", CONTEXT_COUNTS)
@pytest.mark.parametrize("name", list(MODELS))
def test_score_items_at_slices_are_score_items_bits(name, C):
    n = 4097
    _, _, _, batch, model, prof = _case(name, n)
    _, X = _device_contexts(batch, C)
    for N in (101, 300):  # 300: two rounds of 256
        items = _draw_lists(n, B, N, batch[0]).cuda()
        S = model.score_items_at(prof, X, items)
        assert tuple(S.shape) == (B, C, N) and S.dtype == torch.float32
        for c in range(C):
            assert torch.equal(S[:, c], model.score_items(prof, X[:, c], items)), (N, c)
        assert torch.equal(model.score_items_at(prof, X, items.to(torch.int32)), S)


def _explicit_exclusion(n):
    ex = torch.from_numpy(np.random.default_rng(3).integers(1, n, size=(B, 7)))
    ex[:, 0], ex[:, 1] = 0, n + 1  # no entry, and an id outside the catalogue
    return ex.cuda()


@pytest.mark.parametrize("C", CONTEXT_COUNTS)
@pytest.mark.parametrize("name", list(MODELS))
def test_recommend_at_slices_are_recommend_bits(name, C):
    for n in (300, 4097):
        _, _, _, batch, model, prof = _case(name, n)
        _, X = _device_contexts(batch, C)
        some = CandidateSet(torch.from_numpy(np.random.default_rng(5).choice(np.arange(1, n), size=257, replace=False)), n,
                            device="cuda")
        empty = CandidateSet(torch.zeros(0, dtype=torch.int64), n, device="cuda")
        for exclude in ("profile", None, _explicit_exclusion(n)):
            for cand in (None, some, empty):
                for k in (10, 128):
                    s, i = model.recommend_at(prof, X, k=k, exclude=exclude, candidates=cand)
                    assert tuple(s.shape) == (B, C, k) and tuple(i.shape) == (B, C, k)
                    assert s.dtype == torch.float32 and i.dtype == torch.int64
                    for c in range(C):
                        ws, wi = model.recommend(prof, X[:, c], k=k, exclude=exclude, candidates=cand)
                        assert torch.equal(s[:, c], ws) and torch.equal(i[:, c], wi), (n, k, c, len(cand or ()))
                    # one user per chunk of the logit scratch: the same result
                    n_slots = n if cand is None else len(cand)
                    s1, i1 = model.recommend_at(prof, X, k=k, exclude=exclude, candidates=cand,
                                                max_scratch_bytes=4 * C * max(n_slots, 1))
                    assert torch.equal(s1, s) and torch.equal(i1, i)
        with pytest.raises(CarcaHipError, match="max_scratch_bytes"):
            model.recommend_at(prof, X, max_scratch_bytes=4 * C * n - 1)


# ---- 2. best_context ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["90x3-all-ca", "96x2-all-wdot-l2"])
def test_best_context(name):
    n, C = 4097, 5
    _, _, _, batch, model, prof = _case(name, n)
    _, X = _device_contexts(batch, C)
    for N in (101, 300):
        items = _draw_lists(n, B, N, batch[0])
        valid = ((items >= 1) & (items < n)).cuda()
        S = model.score_items_at(prof, X, items.cuda())
        scores, which = model.best_context(prof, X, items.cuda())
        assert tuple(scores.shape) == (B, N) and scores.dtype == torch.float32 and which.dtype == torch.int64
        assert torch.equal(scores, S.max(dim=1).values)
        picked = S.gather(1, which.clamp(min=0).unsqueeze(1)).squeeze(1)
        assert torch.equal(picked[valid], scores[valid])
        assert bool(((which >= 0) & (which < C))[valid].all())
        assert not bool((which == 2).any())  # context 2 repeats context 0: the tie goes to the smaller index
        assert int((~valid).sum()) >= 3
        assert not bool(scores[~valid].any()) and bool((which[~valid] == -1).all())


# ---- 3. the oracle, fp64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [("90x3-all-ca", 100), ("96x2-all-wdot-l2", 128)])
def test_contexts_match_oracle(name, k):
    n, C, N = 4097, 5, 300
    cfg, P, attrs, batch, model, prof = _case(name, n)
    p_x, p_c, _ = batch
    X64, X = _device_contexts(batch, C)
    items = _draw_lists(n, B, N, p_x)
    valid = (items >= 1) & (items < n)
    S = model.score_items_at(prof, X, items.cuda()).cpu()
    got_s, got_i = model.recommend_at(prof, X, k=k)
    ys = {}
    for c in range(C):
        y = ys[0] if c == 2 else _oracle_scores(cfg, P, attrs, (p_x, p_c, X64[:, c]), n)  # (context 2 is context 0)
        ys[c] = y
        want = torch.gather(y, 1, items.clamp(1, n - 1) - 1)
        err = float((S[:, c].double() - want)[valid].abs().max())
        ws, wi, full = _oracle_topk(y, _excl_sets(p_x), k)
        share = _skipped_share(full, k)
        print(f"context {c}: score_items_at error {err:.3e}; skipped share of compared positions {share:.4f}")
        assert err < 2e-5
        assert not bool(S[:, c][~valid].any())
        assert share <= 0.10, share
        _check((got_s[:, c], got_i[:, c]), (ws, wi), full, k)
    # the contexts do change the scores: a kernel that read the wrong context would miss the bound above
    assert float((ys[0] - ys[1]).abs().max()) > 1e-3


# ---- 4. the envelope ------------------------------------------------------------------------------------------------
def test_envelope_errors():
    _, _, _, batch, model, prof = _case("64x4-all-ca", 300)
    _, X = _device_contexts(batch, 2)
    items = _draw_lists(300, B, 101).cuda()
    # an embedding without a context matrix: the score does not depend on the candidate's context
    _, _, _, (p_x, p_c, _), id_model = _setup(62, 2, "id", "ca", "positional", True, 17, B, 300, 0, 1)
    id_prof = (p_x.cuda(), None, p_c.float().cuda())
    none = torch.zeros(B, 2, 0, device="cuda")
    with pytest.raises(CarcaHipError, match="IdEmbedding has no context matrix.*call score_items"):
        id_model.score_items_at(id_prof, none, items)
    with pytest.raises(CarcaHipError, match="IdEmbedding has no context matrix.*call score_items"):
        id_model.best_context(id_prof, none, items)
    with pytest.raises(CarcaHipError, match="IdEmbedding has no context matrix.*call recommend"):
        id_model.recommend_at(id_prof, none)
    # a cross-attention decoder over more than 64 slots, with the wider encoder envelope asked for
    _, _, _, (p_x, p_c, ctx), long_model = _setup(64, 4, "all", "ca", "identity", True, 65, B, 300, N_CTX, 1)
    long_prof = (p_x.cuda(), None, p_c.float().cuda())
    with pytest.raises(CarcaHipError, match="L = 65 exceeds CARCA_MAX_L = 64.*call score_items per context"):
        long_model.score_items_at(long_prof, X, items, allow_composed=True)
    with pytest.raises(CarcaHipError, match="L = 65 exceeds CARCA_MAX_L = 64.*call recommend per context"):
        long_model.recommend_at(long_prof, X, allow_composed=True)
    with pytest.raises(CarcaHipError, match="L = 65 exceeds CARCA_MAX_L = 64.*call score_items per context"):
        long_model.best_context(long_prof, X, items)  # (with or without the wider encoder envelope)
    # training mode
    twin = _setup(64, 4, "all", "ca", "identity", True, 16, B, 300, N_CTX, 1)[4].train()
    for call in (lambda: twin.score_items_at(prof, X, items), lambda: twin.best_context(prof, X, items),
                 lambda: twin.recommend_at(prof, X)):
        with pytest.raises(CarcaHipError, match="training mode.*model.eval()"):
            call()


# ---- 5. reproducibility -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["90x3-all-ca", "96x2-all-wdot-l2"])
def test_two_runs_give_the_same_bits(name):
    n, C = 4097, 9
    _, _, _, batch, model, prof = _case(name, n)
    _, X = _device_contexts(batch, C)
    items = _draw_lists(n, B, 300, batch[0]).cuda()
    assert torch.equal(model.score_items_at(prof, X, items), model.score_items_at(prof, X, items))
    a, b = model.best_context(prof, X, items), model.best_context(prof, X, items)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    a, b = model.recommend_at(prof, X, k=128), model.recommend_at(prof, X, k=128)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
