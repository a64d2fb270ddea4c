"""CARCA.explain_items / explain_top_slots / recommend_explained (carca_explain_lists) on the GPU.
References: the fp64 CPU oracle's trace through tests/explain_ref.py; the reference's own return_w weights and scores
(fixture G1); score_items / recommend for the bits; tests/explain_ref.top_slots over explain_items' own contrib for the
selection (exact)."""
import numpy as np
import pytest
import torch

from carca_replication_amd import CarcaHipError, catalogue
from tests.explain_ref import oracle_explain, top_slots
from tests.golden_util import load
from tests.model_util import model_from_fixture
from tests.test_hip_candidates import _model
from tests.test_hip_recommend import _setup
from tests.test_hip_recommend_lists import _draw_lists, _prof

pytestmark = pytest.mark.gpu


def _cpu(ts):
    return tuple(t.cpu() for t in ts)


def _oracle_check(cfg, P, attrs, batch, items, model, **kw):
    """explain_items and explain_top_slots(m=3) against the float64 oracle; returns the observed errors."""
    p_x = batch[0]
    B, N = items.shape
    L, H = p_x.shape[1], cfg.H
    y, base, contrib, w, live = oracle_explain(cfg, P, attrs, batch, items)
    assert int((~live).sum()) >= 3  # an id 0, an id past the catalogue, a negative id
    prof, ctx = _prof(batch)
    s, b, c, ww = _cpu(model.explain_items(prof, ctx, items.cuda(), **kw))
    assert s.shape == (B, N) and b.shape == (B, N) and c.shape == (B, N, L) and ww.shape == (B, H, N, L)
    assert all(t.dtype == torch.float32 for t in (s, b, c, ww))
    scale = max(1.0, float(contrib.abs().max()))
    tol = 1e-4 * scale
    errs = dict(scores=float((s.double() - y).abs().max()), weights=float((ww.double() - w).abs().max()),
                contrib=float((c.double() - contrib).abs().max()), base=float((b.double() - base).abs().max()))
    print(f"largest |contrib| {float(contrib.abs().max()):.4f}; errors " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert errs["scores"] < 2e-5 and errs["weights"] < 1e-5 and errs["contrib"] < tol and errs["base"] < tol, errs

    # the three largest slots, wherever the oracle's neighbouring contributions are more than 2 tol apart
    ts, tb, slots, sitems, vals = _cpu(model.explain_top_slots(prof, ctx, items.cuda(), m=3, **kw))
    assert slots.shape == (B, N, 3) and slots.dtype == torch.int64 and sitems.dtype == torch.int64
    assert vals.dtype == torch.float32 and torch.equal(ts, s) and torch.equal(tb, b)
    want_slots, want_items, want_vals = top_slots(contrib, p_x, 3, live)
    total = skipped = 0
    for u in range(B):
        v = torch.nonzero(p_x[u] != 0).reshape(-1)
        nv = v.numel()
        srt = torch.sort(contrib[u][:, v], dim=1, descending=True).values if nv else None
        for r in range(3):
            if r >= nv:  # fewer valid slots than m: padding
                assert bool((slots[u, :, r] == -1).all()) and not bool(sitems[u, :, r].any()) and not bool(vals[u, :, r].any())
                continue
            one = torch.ones(N, dtype=torch.float64)
            lo = srt[:, r - 1] - srt[:, r] if r > 0 else one
            hi = srt[:, r] - srt[:, r + 1] if r + 1 < nv else one
            clear = (torch.minimum(lo, hi) > 2 * tol) & live[u]
            total += int(live[u].sum())
            skipped += int((live[u] & ~clear).sum())
            assert torch.equal(slots[u, :, r][clear], want_slots[u, :, r][clear]), (u, r)
            assert torch.equal(sitems[u, :, r][clear], want_items[u, :, r][clear]), (u, r)
            assert bool(((vals[u, :, r].double() - want_vals[u, :, r])[clear].abs() < tol).all())
        dead = ~live[u]
        assert bool((slots[u][dead] == -1).all()) and not bool(sitems[u][dead].any()) and not bool(vals[u][dead].any())
    share = skipped / max(total, 1)
    print(f"top-3 positions compared: {total}, skipped (neighbours within 2 tol): {skipped} ({share:.4f})")
    assert total > 0 and share <= 0.10, share
    return errs


def _bit_checks(model, prof, ctx, p_x, items, n, **kw):
    """scores against score_items, explain_top_slots against the selection over explain_items' own contrib, two calls."""
    dev = items.cuda()
    want = model.score_items(prof, ctx, dev, **kw)
    s, b, c, w = model.explain_items(prof, ctx, dev, **kw)
    assert torch.equal(s, want)
    live = (items >= 1) & (items < n)
    for m in (1, 3, 8):
        ts, tb, slots, sitems, vals = model.explain_top_slots(prof, ctx, dev, m=m, **kw)
        assert torch.equal(ts, want) and torch.equal(tb, b)
        ws, wi, wv = top_slots(c.cpu(), p_x, m, live)
        assert torch.equal(slots.cpu(), ws) and torch.equal(sitems.cpu(), wi) and torch.equal(vals.cpu(), wv), m
    again = model.explain_items(prof, ctx, dev, **kw)
    assert all(torch.equal(a, t) for a, t in zip(again, (s, b, c, w)))
    a3, b3 = model.explain_top_slots(prof, ctx, dev, m=3, **kw), model.explain_top_slots(prof, ctx, dev, m=3, **kw)
    assert all(torch.equal(a, t) for a, t in zip(a3, b3))
    return s, b, c, w


def _structure(p_x, items, n, s, b, c, w):
    """exact zeros, weights that sum to 1, and the decomposition itself"""
    s, b, c, w = _cpu((s, b, c, w))
    live = (items >= 1) & (items < n)
    pad = p_x == 0  # [B, L]
    assert not bool(w.permute(0, 3, 1, 2)[pad].any()) and not bool(c.permute(0, 2, 1)[pad].any())
    assert not bool(w.permute(0, 2, 1, 3)[~live].any()) and not bool(c[~live].any())
    assert not bool(s[~live].any()) and not bool(b[~live].any())
    some = (~pad).any(dim=1)  # users with a valid slot
    full = live & some.unsqueeze(1)
    sums = w.sum(-1).permute(0, 2, 1)[full]  # [entries, H]
    assert sums.numel() and float((sums - 1).abs().max()) < 1e-5
    assert float((torch.sigmoid(b + c.sum(-1)) - s)[live].abs().max()) < 2e-5
    assert bool((s[live] > 0).all())


# ---- 1. the fp64 oracle ------------------------------------------------------------------------------------------------
# (d, H, embedding, encoding, residual_ca, L, n_items, n_ctx, n_blocks, N)
ORACLE_CASES = [
    (64, 4, "all", "identity", True, 16, 300, 6, 1, 101),
    (90, 3, "all", "identity", True, 50, 4097, 6, 2, 300),
    (62, 2, "id", "positional", True, 17, 300, 0, 1, 256),
    (128, 4, "all", "learnable", False, 64, 300, 6, 1, 130),
    (96, 2, "attrctx", "identity", False, 17, 300, 6, 1, 101),
    (64, 1, "mlpid", "learnable", True, 50, 300, 0, 1, 101),
]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=[f"{c[0]}x{c[1]}-{c[2]}-{c[3][:3]}-res{int(c[4])}-L{c[5]}-n{c[6]}-N{c[9]}"
                                                    for c in ORACLE_CASES])
def test_explanations_match_oracle(case):
    """Observed on the MI355X (errors of scores / weights / contrib / base, share of top-3 positions skipped): see
    DESIGN.md section 22."""
    d, H, emb, enc, res, L, n, n_ctx, nb, N = case
    cfg, P, attrs, batch, model = _setup(d, H, emb, "ca", enc, res, L, 5, n, n_ctx, nb)
    _oracle_check(cfg, P, attrs, batch, _draw_lists(n, 5, N, batch[0]), model)


# ---- 2. the reference itself: fixture G1's return_w weights and scores -------------------------------------------------
@pytest.mark.parametrize("name", ["g1_d90h3", "g1_d64h2", "g1_d128h4", "g1_d90h2"])
def test_weights_are_the_references_return_w(name):
    fx = load(name)
    model = model_from_fixture(fx).eval()
    i = fx.ins
    table = torch.zeros(int(fx.dim["n_items"]), int(fx.dim["n_attrs"]))
    table[i["p_x"].long()] = i["p_a"].float()
    table[i["o_x"].long()] = i["o_a"].float()
    table[0] = 0
    model.embeds.register_attr_table(table.cuda())
    prof = (i["p_x"].cuda(), None, i["p_c"].float().cuda())
    s, b, c, w = _cpu(model.explain_items(prof, i["o_c"][:, 0].float().cuda(), i["o_x"].cuda()))
    e_w, e_s = float((w - fx.outs["dec_w0"]).abs().max()), float((s - fx.outs["y"]).abs().max())
    print(f"{name}: weights against dec_w0 {e_w:.3e}, scores against y {e_s:.3e}")
    assert w.shape == fx.outs["dec_w0"].shape and e_w < 1e-5 and e_s < 2e-5
    valid = (i["p_x"] != 0).sum(1).tolist()
    assert valid[0] == 0 and valid[1] == 1  # the all-padding user and the one-slot user
    assert not bool(w[0].any()) and not bool(c[0].any())
    at = int(torch.nonzero(i["p_x"][1] != 0)[0])
    assert bool((w[1, :, :, at] == 1).all()) and int((w[1] != 0).sum()) == w.shape[1] * w.shape[2]
    _structure(i["p_x"].long(), i["o_x"].long(), int(fx.dim["n_items"]), s, b, c, w)


# ---- 3. bits -----------------------------------------------------------------------------------------------------------
def test_bits_against_score_items_and_the_selection():
    n = 4097
    model, prof, ctx, p_x = _model("ca", n)
    items = _draw_lists(n, 5, 300, p_x)
    out = _bit_checks(model, prof, ctx, p_x, items, n)
    _structure(p_x, items, n, *out)


def test_recommend_explained_is_recommend_then_explain_top_slots():
    n, k, m = 4097, 10, 3
    model, prof, ctx, p_x = _model("ca", n)
    few = catalogue.CandidateSet(torch.tensor([5, 9, 250, 31, 77, 1000]), n, device="cuda")  # fewer than k: every row pads
    for kw in (dict(), dict(exclude=None), dict(candidates=few)):
        s, i, sit, con = model.recommend_explained(prof, ctx, k=k, m=m, **kw)
        ws, wi = model.recommend(prof, ctx, k=k, **kw)
        assert torch.equal(s, ws) and torch.equal(i, wi)
        ts, tb, slots, witems, wcon = model.explain_top_slots(prof, ctx, i, m=m)
        assert torch.equal(ts, s)  # (the padding id 0 scores 0 in both)
        assert sit.shape == (5, k, m) and sit.dtype == torch.int64 and con.dtype == torch.float32
        assert torch.equal(sit, witems) and torch.equal(con, wcon)
        padded = i == 0
        assert not bool(sit[padded].any()) and not bool(con[padded].any())
        if "candidates" in kw:
            assert int(padded.sum()) == 5 * (k - 6)
    assert bool((sit[0] != 0).any())


# ---- 4. structure ------------------------------------------------------------------------------------------------------
def test_zeros_sums_and_the_decomposition():
    n, B, N = 300, 5, 101
    cfg, P, attrs, (p_x, p_c, ctx), model = _setup(64, 4, "all", "ca", "identity", True, 16, B, n, 6, 1)
    rng = np.random.default_rng(4)
    p_x[0], p_c[0] = 0, 0
    p_x[0, 3:] = torch.from_numpy(rng.integers(1, n, size=13))
    p_c[0, 3:] = torch.from_numpy(rng.random((13, 6)))
    p_x[0, 7], p_x[0, 12] = 0, 0  # interior padding slots
    p_c[0, 7], p_c[0, 12] = 0, 0
    assert not bool(p_x[1].any()) and int((p_x[2] != 0).sum()) == 1
    prof, c_ = _prof((p_x, p_c, ctx))
    items = _draw_lists(n, B, N, p_x)
    out = model.explain_items(prof, c_, items.cuda())
    _structure(p_x, items, n, *out)
    w = out[3].cpu()
    assert not bool(w[0, :, :, 7].any()) and not bool(w[0, :, :, 12].any()) and bool((w[0, :, 5, 8] > 0).all())
    ts, tb, slots, sitems, vals = _cpu(model.explain_top_slots(prof, c_, items.cuda(), m=8))
    live = (items >= 1) & (items < n)
    assert bool((slots[1] == -1).all()) and not bool(sitems[1].any()) and not bool(vals[1].any())  # the empty profile
    assert bool((slots[2][live[2]][:, 0] == 15).all()) and bool((slots[2][:, 1:] == -1).all())  # one slot, seven pads
    assert not bool(sitems[2][:, 1:].any()) and not bool(vals[2][:, 1:].any())
    assert bool((slots[0][~live[0]] == -1).all()) and not bool(sitems[0][~live[0]].any())
    picked = slots[0][live[0]]
    assert not bool(((picked == 7) | (picked == 12)).any()) and bool((picked >= 3).all())
    assert torch.equal(torch.where(slots >= 0, p_x.unsqueeze(1).expand(B, N, 16).gather(2, slots.clamp(min=0)),
                                   torch.zeros_like(slots)), sitems)


# ---- 5. a constructed tie ----------------------------------------------------------------------------------------------
def test_tie_goes_to_the_later_slot():
    """No encoder block and the identity encoding: a slot's K and value rows depend on its (item, context) alone, so the
    same pair in two slots gives equal weights and contributions, bit for bit."""
    n, B, N = 300, 5, 101
    cfg, P, attrs, (p_x, p_c, ctx), model = _setup(64, 4, "all", "ca", "identity", True, 16, B, n, 6, 0)
    rng = np.random.default_rng(11)
    p_x[0], p_c[0] = 0, 0
    p_x[0, 10:] = torch.from_numpy(rng.choice(np.arange(1, n), size=6, replace=False))
    p_c[0, 10:] = torch.from_numpy(rng.random((6, 6)))
    p_x[0, 11], p_c[0, 11] = p_x[0, 14], p_c[0, 14]
    prof, c_ = _prof((p_x, p_c, ctx))
    items = _draw_lists(n, B, N, p_x)
    s, b, c, w = _cpu(model.explain_items(prof, c_, items.cuda()))
    assert torch.equal(w[0, :, :, 11], w[0, :, :, 14]) and torch.equal(c[0, :, 11], c[0, :, 14])
    assert bool((w[0, :, 5, 11] > 0).all())
    slots = model.explain_top_slots(prof, c_, items.cuda(), m=8)[2].cpu()
    live = (items[0] >= 1) & (items[0] < n)
    rows = slots[0][live]
    assert rows.shape[0] >= 90 and bool((rows[:, 6:] == -1).all())
    at14, at11 = (rows == 14).int().argmax(1), (rows == 11).int().argmax(1)
    assert bool(((rows == 14).sum(1) == 1).all()) and bool(((rows == 11).sum(1) == 1).all())
    assert bool((at11 == at14 + 1).all())  # the later slot first, its twin right behind


# ---- 6. shapes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 257, 1025])
def test_list_lengths(N):
    n = 300
    model, prof, ctx, p_x = _model("ca", n)
    items = _draw_lists(n, 5, N, p_x)
    out = _bit_checks(model, prof, ctx, p_x, items, n)
    _structure(p_x, items, n, *out)
    a = model.explain_items(prof, ctx, items.to(torch.int32).cuda())
    assert all(torch.equal(x, y) for x, y in zip(a, out))
    t64 = model.explain_top_slots(prof, ctx, items.cuda(), m=3)
    t32 = model.explain_top_slots(prof, ctx, items.to(torch.int32).cuda(), m=3)
    assert all(torch.equal(x, y) for x, y in zip(t64, t32))


def test_more_users_than_cus():
    n, B = 300, 260
    model, prof, ctx, p_x = _model("ca", n, B)
    items = _draw_lists(n, B, 3, p_x)
    out = _bit_checks(model, prof, ctx, p_x, items, n)
    _structure(p_x, items, n, *out)


# ---- 7. long profiles --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [65, 130])
@pytest.mark.parametrize("geom", [(64, 4), (90, 3)], ids=["64x4", "90x3"])
def test_long_profiles(geom, L):
    """The oracle comparison of test 1 over the set-up's own users, then the bit checks over the same users with user 0
    given every slot (at L = 130: three chunks).  The set-up's seed at L = 130 is chosen by the float64 reference alone:
    slots of a long profile contribute little each and lie close, and with seed 0 (users of 115, 87 and 57 slots) the
    reference itself leaves 13.4 % of the top-3 positions at d 64 / H 4 within twice the tolerance of a neighbour; with
    seed 2 (120, 67 and 58 slots: two chunks, two chunks, one) it leaves 7.2 % and 8.2 %, with seed 0 at L = 65 4.4 % and
    2.9 % (computed on the CPU from oracle.carca_forward's trace with the lists drawn here).  With the full 130-slot user
    the share is 14 %, so that user is covered by the bit checks and the decomposition."""
    d, H = geom
    n, B, N = 300, 5, 300
    cfg, P, attrs, (p_x, p_c, ctx), model = _setup(d, H, "all", "ca", "identity", True, L, B, n, 6, 1, seed=2 if L == 130 else 0)
    print("valid slots per user:", (p_x != 0).sum(1).tolist())
    items = _draw_lists(n, B, N, p_x)
    _oracle_check(cfg, P, attrs, (p_x, p_c, ctx), items, model, allow_composed=True)
    rng = np.random.default_rng(9)
    p_x[0] = torch.from_numpy(rng.integers(1, n, size=L))
    p_c[0] = torch.from_numpy(rng.random((L, 6)))
    prof, c_ = _prof((p_x, p_c, ctx))
    out = _bit_checks(model, prof, c_, p_x, items, n, allow_composed=True)
    _structure(p_x, items, n, *out)


# ---- 8. errors ---------------------------------------------------------------------------------------------------------
def test_argument_errors_at_the_call():
    n, B = 300, 5
    model, prof, ctx, p_x = _model("ca", n)
    items = _draw_lists(n, B, 20, p_x).cuda()
    calls = (lambda it: model.explain_items(prof, ctx, it), lambda it: model.explain_top_slots(prof, ctx, it))
    model.train()
    try:
        for call in calls + (lambda it: model.recommend_explained(prof, ctx),):
            with pytest.raises(CarcaHipError, match="eval"):
                call(items)
    finally:
        model.eval()
    for call in calls:
        for bad in (items.float(), items[0], items[:B - 1], items[:, :0]):
            with pytest.raises(CarcaHipError, match="items"):
                call(bad)
    for m in (0, 9):
        with pytest.raises(CarcaHipError, match="1..8"):
            model.explain_top_slots(prof, ctx, items, m=m)
        with pytest.raises(CarcaHipError, match="1..8"):
            model.recommend_explained(prof, ctx, m=m)
    dot, dprof, dctx, _ = _model("dot", n)
    for call in (lambda: dot.explain_items(dprof, dctx, items), lambda: dot.explain_top_slots(dprof, dctx, items),
                 lambda: dot.recommend_explained(dprof, dctx)):
        with pytest.raises(CarcaHipError, match="DotProduct"):
            call()
    long = (torch.ones(B, 65, dtype=torch.int64).cuda(), None, torch.zeros(B, 65, 6).cuda())
    for call in (lambda: model.explain_items(long, ctx, items), lambda: model.explain_top_slots(long, ctx, items),
                 lambda: model.recommend_explained(long, ctx)):
        with pytest.raises(CarcaHipError, match="64"):
            call()
