"""CARCA.retrieve / KNN.retrieve (the deep top-k, csrc/deep_select.h + retrieve.hip).

The new selection is never its own judge.  What a result is compared with:
  * recommend (k <= 128) and shorter retrieve calls: the prefix property, torch.equal in both outputs;
  * rank_items, 128 returned ids at a time: the id in column j must have rank j exactly (the counting sweep shares no
    code with the selection), its score rank_items' bits; columns past the eligible count hold id 0 and score 0;
  * score_items: the score bits;
  * the result with the row split into S = 1, 2, 3, 7 and 64 parts (ops.TUNE_RETRIEVE_PARTS): equal for every S;
  * the fp64 oracle: the returned scores against the descending-sorted eligible oracle scores at recommend's tolerance,
    2e-5 (sorted order statistics move by at most the per-score error, so nothing is skipped as ambiguous).
Shapes: n_items 2 (k above the eligible count), 300 (one read, sorted whole), 4097 (the radix regime begins, k about n),
9001 (more than two key blocks, k below n); B 1 and 5 (B = 5 holds _setup's empty and one-slot profiles)."""
import numpy as np
import pytest
import torch

from carca_replication_amd import CarcaHipError, _lib, catalogue, ops
from carca_replication_amd.modules import KNN
from oracle import carca_oracle as O
from tests.model_util import build_model

pytestmark = pytest.mark.gpu

G, N_ATTRS = 24, 12
KS = (1, 128, 129, 1000, 4096)
PARTS = (1, 2, 3, 7, 64)


# ---- tests/test_hip_recommend.py's model helper (copied: test modules do not import each other) ----------------------
def _setup(d, H, emb, dec, enc, res_ca, L, B, n_items, n_ctx, nb, l2=False, seed=0):
    cfg = O.CarcaConfig(d=d, H=H, n_blocks=nb, residual_ca=res_ca, encoding=enc, embedding=emb, decoder=dec, l2_norm=l2)
    n_attrs = N_ATTRS
    P = O.perturb_params(O.init_params(cfg, n_items, G, n_ctx, n_attrs, L, seed=seed, dtype=torch.float64), seed=seed + 1)
    rng = np.random.default_rng(seed + 7)
    attrs = torch.from_numpy(rng.random((n_items, n_attrs))).double()
    attrs[0] = 0
    p_x = torch.zeros(B, L, dtype=torch.int64)
    for b in range(B):
        ell = 0 if (b == 1 and B > 2) else 1 if (b == 2 and B > 2) else int(rng.integers(1, L + 1))
        if ell:
            p_x[b, L - ell:] = torch.from_numpy(rng.integers(1, n_items, size=ell))
    p_c = torch.from_numpy(rng.random((B, L, n_ctx))).double() * (p_x != 0).unsqueeze(-1)
    ctx = torch.from_numpy(rng.random((B, n_ctx))).double()
    model = build_model(dict(d=d, H=H, n_blocks=nb, encoding=enc, residual_ca=res_ca, embedding=emb, decoder=dec,
                             l2_norm=l2), n_items, G, n_ctx, n_attrs, L)
    model.load_state_dict({k: v.float() for k, v in P.items()}, strict=True)
    model = model.cuda().eval()
    if hasattr(model.embeds, "register_attr_table"):
        model.embeds.register_attr_table(attrs.float().cuda())
    return cfg, P, attrs, (p_x, p_c, ctx), model


def _oracle_scores(cfg, P, attrs, batch, n_items):
    p_x, p_c, ctx = batch
    B = p_x.shape[0]
    ids = torch.cat([torch.arange(1, n_items), torch.zeros(1, dtype=torch.int64)]).expand(B, -1)
    o_c = ctx.unsqueeze(1).expand(B, n_items, ctx.shape[1])
    y = O.carca_forward(P, cfg, (p_x, attrs[p_x], p_c), [(ids, attrs[ids], o_c)], training=False)
    return y.reshape(B, n_items)[:, :-1]


# name -> (d, H, embedding, decoder, encoding, residual_ca, n_ctx, n_blocks, l2)
GEOS = {
    "ca64x4-all": (64, 4, "all", "ca", "identity", True, 6, 1, False),
    "ca90x3-attrctx-res": (90, 3, "attrctx", "ca", "positional", True, 6, 1, False),
    "ca128x1-id": (128, 1, "id", "ca", "learnable", False, 0, 1, False),
    "dot64x2": (64, 2, "all", "dot", "identity", True, 6, 1, False),
    "wdot96x2-l2": (96, 2, "all", "wdot", "positional", True, 6, 1, True),
}


def _model(geo, L, B, n, seed=0):
    d, H, emb, dec, enc, res, n_ctx, nb, l2 = GEOS[geo]
    cfg, P, attrs, batch, model = _setup(d, H, emb, dec, enc, res, L, B, n, n_ctx, nb, l2, seed)
    p_x, p_c, ctx = batch
    return cfg, P, attrs, batch, model, (p_x.cuda(), None, p_c.float().cuda()), ctx.float().cuda()


class _forced_parts:
    """TUNE_RETRIEVE_PARTS = S inside the block, 0 again behind it."""

    def __init__(self, S):
        self.S = S

    def __enter__(self):
        _lib.check(_lib.load().carca_set_tuning(ops.TUNE_RETRIEVE_PARTS, self.S), "set_tuning")

    def __exit__(self, *exc):
        _lib.load().carca_set_tuning(ops.TUNE_RETRIEVE_PARTS, 0)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _excl_sets(p_x, kind, extra):
    B = p_x.shape[0]
    if kind == "profile":
        return [set(p_x[b].tolist()) - {0} for b in range(B)]
    if kind is None:
        return [set() for _ in range(B)]
    return [set(extra[b].tolist()) - {0} for b in range(B)]


def _extra_list(n, B, top):
    """An explicit exclusion list [B, E]: each user's best few items, a duplicate, zeros, random ids, ids outside."""
    g = torch.Generator().manual_seed(5)
    e = torch.randint(1, max(n, 2), (B, 40), generator=g)
    e[:, :4] = top[:, :4].cpu()
    e[:, 4] = e[:, 0]
    e[:, 5:8] = 0
    e[:, 8] = n + 3
    return e.to(torch.int32)


def _prefix_checks(retrieve, recommend):
    """Assertion 1: -> {k: retrieve(k)} for k in KS."""
    out = {k: retrieve(k) for k in KS}
    for k, (s, i) in out.items():
        assert s.shape == (s.shape[0], k) and i.shape == s.shape and s.dtype == torch.float32 and i.dtype == torch.int64
    r1, r128 = recommend(1), recommend(128)
    assert _same(out[1], r1) and _same(out[128], r128)
    for k in (129, 1000, 4096):
        assert _same((out[k][0][:, :128], out[k][1][:, :128]), r128), k
    assert _same((out[4096][0][:, :1000], out[4096][1][:, :1000]), out[1000])
    assert _same((out[1000][0][:, :129], out[1000][1][:, :129]), out[129])
    return out


def _order_checks(got, eligible, rank_fn, score_fn=None):
    """Assertions 2 and 3 over one result: eligible[b] is user b's set of eligible ids; rank_fn(ids [B, <= 128]) ->
    (scores, ranks) of rank_items under the call's exclusion; score_fn(ids) -> score_items' scores."""
    s, i = got
    B, k = i.shape
    ic, sc = i.cpu(), s.cpu()
    m = torch.tensor([min(k, len(e)) for e in eligible])
    col = torch.arange(k)
    live = col[None, :] < m[:, None]
    assert bool((ic[~live] == 0).all()) and bool((sc[~live] == 0).all())
    for b in range(B):
        row = ic[b, :int(m[b])].tolist()
        assert len(set(row)) == len(row) and set(row) <= eligible[b], b  # distinct, none excluded, none 0
    for lo in range(0, max(int(m.max()), 1), 128):
        hi = min(lo + 128, k)
        rs, rr = rank_fn(i[:, lo:hi].contiguous())
        want = torch.where(live[:, lo:hi], col[lo:hi].expand(B, -1), torch.full((B, hi - lo), -1))
        assert torch.equal(rr.cpu(), want), lo  # column j holds the item of rank j; padding (id 0) ranks -1
        assert torch.equal(rs, s[:, lo:hi]), lo
    if score_fn is not None:
        assert torch.equal(score_fn(i).cpu()[live], sc[live])


def _split_checks(retrieve, out, ks=KS):
    """Assertion 4: every forced number of parts gives the bits of `out` (taken with the shipped choice)."""
    for S in PARTS:
        with _forced_parts(S):
            for k in ks:
                assert _same(retrieve(k), out[k]), (S, k)
    assert ops.get_tuning(ops.TUNE_RETRIEVE_PARTS) == 0


# (n_items, B, L) -- every geometry runs all four; the exclusion form rotates with the geometry
SHAPES = [(2, 1, 1), (300, 5, 17), (4097, 5, 64), (9001, 1, 17)]
EXCLUDES = ("profile", None, "tensor")


@pytest.mark.parametrize("shape", range(len(SHAPES)), ids=[f"n{n}-B{B}-L{L}" for n, B, L in SHAPES])
@pytest.mark.parametrize("geo", list(GEOS))
def test_retrieve_prefix_order_scores_and_split(geo, shape):
    n, B, L = SHAPES[shape]
    if n == 9001 and list(GEOS).index(geo) % 2:
        B = 5
    kind = EXCLUDES[(list(GEOS).index(geo) + shape) % 3]
    _, _, _, batch, model, prof, c = _model(geo, L, B, n)
    extra = None
    exclude = kind
    if kind == "tensor":
        extra = _extra_list(n, B, model.recommend(prof, c, k=8, exclude=None)[1])
        exclude = extra.cuda()
    out = _prefix_checks(lambda k: model.retrieve(prof, c, k=k, exclude=exclude),
                         lambda k: model.recommend(prof, c, k=k, exclude=exclude))
    excl = _excl_sets(batch[0], kind, extra)
    eligible = [set(range(1, n)) - e for e in excl]
    for k in (129, 4096):
        _order_checks(out[k], eligible, lambda ids: model.rank_items(prof, c, ids, exclude=exclude),
                      lambda ids: model.score_items(prof, c, ids))
    if n >= 4097:
        _split_checks(lambda k: model.retrieve(prof, c, k=k, exclude=exclude), out)
    # the ids go unchanged into the second-stage calls: id 0 scores 0 there
    s2, i2 = model.recommend_from(prof, c, out[1000][1], k=20, exclude=exclude)
    assert _same((s2, i2), (out[1000][0][:, :20], out[1000][1][:, :20]))


@pytest.mark.parametrize("geo", ["ca64x4-all", "dot64x2"])
def test_candidates(geo):
    n, B, L = 9001, 5, 17
    _, _, _, batch, model, prof, c = _model(geo, L, B, n)
    g = torch.Generator().manual_seed(3)
    perm = torch.randperm(n - 1, generator=g) + 1
    for size in (0, 1, 200, 5000):
        S = catalogue.CandidateSet(perm[:size].cuda(), n)
        assert len(S) == size
        want = model.recommend(prof, c, k=128, candidates=S)
        excl = _excl_sets(batch[0], "profile", None)
        eligible = [set(perm[:size].tolist()) - e for e in excl]
        out = {}
        for k in (128, 1000, 4096):
            out[k] = model.retrieve(prof, c, k=k, candidates=S)
            assert _same((out[k][0][:, :128], out[k][1][:, :128]), want), (size, k)
        if size == 0:
            assert not bool(out[4096][0].any()) and not bool(out[4096][1].any())
        _order_checks(out[4096], eligible, lambda ids: model.rank_items(prof, c, ids, candidates=S),
                      lambda ids: model.score_items(prof, c, ids))
        for parts in (3, 64):
            with _forced_parts(parts):
                for k in (1000, 4096):
                    assert _same(model.retrieve(prof, c, k=k, candidates=S), out[k]), (size, parts, k)
    # a raw tensor and a mask build the set for the call
    raw = model.retrieve(prof, c, k=1000, candidates=perm[:200].cuda())
    mask = torch.zeros(n, dtype=torch.bool)
    mask[perm[:200]] = True
    assert _same(raw, model.retrieve(prof, c, k=1000, candidates=mask.cuda()))
    assert _same(raw, model.retrieve(prof, c, k=1000, candidates=catalogue.CandidateSet(perm[:200].cuda(), n)))


def test_composed_route():
    n, B, L = 300, 3, 65
    _, _, _, batch, model, prof, c = _model("ca64x4-all", L, B, n)
    want = model.recommend(prof, c, k=128, allow_composed=True)
    got = model.retrieve(prof, c, k=1000, allow_composed=True)
    assert _same((got[0][:, :128], got[1][:, :128]), want)
    excl = _excl_sets(batch[0], "profile", None)
    _order_checks(got, [set(range(1, n)) - e for e in excl],
                  lambda ids: model.rank_items(prof, c, ids, allow_composed=True),
                  lambda ids: model.score_items(prof, c, ids, allow_composed=True))


@pytest.mark.parametrize("boundary", [129, 1000])
def test_ties_across_the_depth(boundary):
    """701 ids spread over the catalogue share one embedding row of an "id" model, so their logits are bit-equal for every
    user.  The source is the item user 0 ranks boundary - 79 places from the top and the copies go over items it ranks
    below that and that no profile holds, so for user 0 the tied ids lie on both sides of column `boundary` -- asserted
    below from rank_items and score_items, not from retrieve.  The tied ids must come out ascending for every user, and a
    k that cuts the tie keeps the smaller ids.  (Other items may tie with them too -- a user with one profile slot or none
    scores many items alike -- which the assertions allow for: ties of any size go to the smaller id.)"""
    n, B, L = 4097, 5, 17
    _, _, _, batch, model = _setup(64, 4, "id", "ca", "identity", True, L, B, n, 0, 1)
    p_x, p_c, ctx = batch
    prof, c = (p_x.cuda(), None, p_c.float().cuda()), ctx.float().cuda()
    r0 = boundary - 79
    order0 = model.retrieve(prof, c, k=4096, exclude=None)[1][0].cpu()
    assert int((order0 != 0).sum()) == n - 1
    src = int(order0[r0])
    in_profiles = set(p_x.flatten().tolist())
    below = [int(v) for v in order0[r0 + 1:].tolist() if v not in in_profiles]
    over = below[::len(below) // 700][:700]
    assert len(over) == 700 and src not in in_profiles
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    W = sd["embeds.items_embed.weight"]
    W[torch.tensor(over, device=W.device)] = W[src].clone()
    model.load_state_dict(sd)
    tied = torch.tensor(sorted(over + [src]))
    assert int(tied.max()) - int(tied.min()) > n // 2  # spread over the catalogue
    # the premise: equal score bits for every user, ranks that differ by the ties between them, user 0's across the boundary
    sc = model.score_items(prof, c, tied.expand(B, -1).contiguous().cuda())
    assert bool((sc == sc[:, :1]).all())
    ends = torch.stack([tied[:1], tied[-1:]], 1).reshape(1, 2).expand(B, -1).contiguous().cuda()
    rr = model.rank_items(prof, c, ends, exclude=None)[1].cpu()
    assert bool((rr[:, 1] - rr[:, 0] >= 700).all())  # (== 700 where no other item shares the logit)
    assert int(rr[0, 0]) < boundary <= int(rr[0, 1])
    print(f"boundary {boundary}: ranks of the smallest / largest tied id per user {rr.tolist()}")
    ks = (boundary, 4096)
    out = {k: model.retrieve(prof, c, k=k, exclude=None) for k in ks}
    assert _same((out[4096][0][:, :boundary], out[4096][1][:, :boundary]), out[boundary])
    where = torch.full((n,), -1, dtype=torch.int64)
    for b in range(B):
        row = out[4096][1][b].cpu()
        where[row] = torch.arange(4096)
        at = where[tied]
        assert bool((at[1:] > at[:-1]).all()) and int(at[0]) == int(rr[b, 0]) and int(at[-1]) == int(rr[b, 1]), b
    cut = out[boundary][1][0].cpu()
    kept = sorted(set(cut.tolist()) & set(tied.tolist()))
    assert 0 < len(kept) < 701 and kept == tied[:len(kept)].tolist()  # cut by k inside the tie: the smaller ids stay
    if boundary == 129:
        assert _same((out[129][0][:, :128], out[129][1][:, :128]), model.recommend(prof, c, k=128, exclude=None))
    _order_checks(out[4096], [set(range(1, n))] * B, lambda ids: model.rank_items(prof, c, ids, exclude=None))
    _split_checks(lambda k: model.retrieve(prof, c, k=k, exclude=None), out, ks)


# ---- the KNN baseline: ties for free ---------------------------------------------------------------------------------
def _knn_table(kind, n_items, F):
    g = torch.Generator().manual_seed(31)
    if kind == "multihot":  # integers: the i8 path
        A = (torch.rand(n_items, F, generator=g) < 0.3).float()
    else:  # a float table, the fp32 path.  Entries are multiples of 1/8 in [-1, 1]: every product is a multiple of 1/64
        #    and every partial sum below 2^6, so an fp32 sum is exact in any order -- which is what lets this test ask for
        #    EQUAL bits between retrieve's GEMM and forward's per-pair kernel, two different summation orders
        A = torch.randint(-8, 9, (n_items, F), generator=g).float() / 8
    A[0] = 0
    return A


@pytest.mark.parametrize("kind", ["multihot", "float"])
def test_knn_retrieve(kind):
    n, F, B, L = 5000, 37, 5, 3
    A = _knn_table(kind, n, F)
    model = KNN().cuda()
    model.register_attr_table(A.cuda())
    assert (model.int8_table() is not None) == (kind == "multihot")
    g = torch.Generator().manual_seed(32)
    p_x = torch.randint(0, n, (B, L), generator=g)
    p_x[:, -1] = torch.randint(1, n, (B,), generator=g)
    prof = (p_x.cuda(), None, None)
    extra = _extra_list(n, B, model.recommend(prof, None, k=8, exclude=None)[1])
    for kind_x, exclude in (("profile", "profile"), (None, None), ("tensor", extra.cuda())):
        out = _prefix_checks(lambda k: model.retrieve(prof, None, k=k, exclude=exclude),
                             lambda k: model.recommend(prof, None, k=k, exclude=exclude))
        eligible = [set(range(1, n)) - e for e in _excl_sets(p_x, kind_x, extra)]
        s, i = out[4096]
        _order_checks(out[4096], eligible, lambda ids: model.rank_items(prof, None, ids, exclude=exclude))
        assert torch.equal(model(prof, [(i, None, None)]).reshape(B, -1), s)  # forward's scores for the returned pairs
        ties = s[:, 1:] == s[:, :-1]
        assert int(ties.sum()) > 1000 and bool((i[:, 1:][ties] > i[:, :-1][ties]).all())  # inside a tie, ascending ids
    _split_checks(lambda k: model.retrieve(prof, None, k=k, exclude=exclude), out)
    model.train()  # train and eval mode alike
    assert _same(model.retrieve(prof, None, k=1000, exclude=exclude), out[1000])


# ---- the oracle --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", ["ca64x4-all", "wdot96x2-l2"])
def test_scores_match_the_sorted_oracle_scores(geo):
    n, B, L, k = 4097, 5, 17, 4096
    cfg, P, attrs, batch, model, prof, c = _model(geo, L, B, n)
    y = _oracle_scores(cfg, P, attrs, batch, n)  # [B, n - 1] for ids 1 .. n - 1
    s, _ = model.retrieve(prof, c, k=k)
    excl = _excl_sets(batch[0], "profile", None)
    for b in range(B):
        keep = torch.tensor([i not in excl[b] for i in range(1, n)])
        want = torch.zeros(k, dtype=torch.float64)
        srt = torch.sort(y[b][keep], descending=True).values[:k]
        want[:srt.numel()] = srt
        err = float((s[b].cpu().double() - want).abs().max())
        print(f"{geo} user {b}: max |score - sorted oracle score| = {err:.3e}")
        assert err < 2e-5


# ---- the envelope ------------------------------------------------------------------------------------------------------
def test_envelope_errors():
    _, _, _, batch, model, prof, c = _model("ca64x4-all", 16, 2, 300)
    with pytest.raises(CarcaHipError, match=r"^retrieve: k = 4097 outside 1\.\.4096"):
        model.retrieve(prof, c, k=4097)
    model.train()
    with pytest.raises(CarcaHipError, match="^retrieve: the model is in training mode"):
        model.retrieve(prof, c, k=10)
    model.eval()
    long = torch.ones(2, 65, dtype=torch.int64).cuda()
    with pytest.raises(CarcaHipError, match="^retrieve: profile length L = 65 exceeds CARCA_MAX_L = 64"):
        model.retrieve((long, None, torch.zeros(2, 65, 6).cuda()), c, k=10)
    other = catalogue.CandidateSet(torch.arange(1, 50).cuda(), 301)
    with pytest.raises(CarcaHipError, match="^retrieve: the candidate set was built for n_items = 301, the model has 300"):
        model.retrieve(prof, c, k=10, candidates=other)
