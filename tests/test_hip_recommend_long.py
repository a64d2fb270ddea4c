"""CARCA.recommend / rank_items past the fused envelope (allow_composed=True): profiles of more than
64 slots through rc::CaLongScorer (the cross-attention sweep staging a user's valid slots 64 at a time) and encoder
geometries with no fused kernel through long_profile's composed encoder.
  1. C ABI, hand-made tables: the long kernels' outputs equal the 64-slot kernels' bit for bit for the same valid slots.
  2. C ABI, more than 64 valid slots: against a float64 evaluation of section 10's formula over the same tables.
  3. / 4. model level against the fp64 oracle and the model's own (composed) forward.
  5. exclusion and candidate sets at length.   6. train.evaluate_full / evaluate_full_ranks.   7. the envelope's errors."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from carca_replication_amd import CarcaHipError, _lib, ops
from carca_replication_amd.catalogue import CandidateSet
from tests.test_hip_recommend import _check, _excl_sets, _oracle_scores, _oracle_topk, _setup

pytestmark = pytest.mark.gpu

GEOMS = [(64, 4), (90, 3), (128, 1)]


# ---- hand-made tables behind the C ABI -------------------------------------------------------------------------------
class Tables:
    """Random fp32 model-side tables of decoder 0 for B users with nv[u] valid slots each: the item side, and per valid
    slot a K row, its folded values u and its id -- laid out by `layout` at any L and any slot positions."""

    def __init__(self, d, H, n_items, nv, seed, id_hi=None):
        g = torch.Generator().manual_seed(seed)
        self.d, self.H, self.n_items, self.nv, self.B = d, H, n_items, list(nv), len(nv)
        self.ld = (d + 3) // 4 * 4
        r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
        self.item_q = torch.zeros(n_items, self.ld)
        self.item_q[:, :d] = r(n_items, d) * 1.2
        self.item_w = r(n_items) * 0.5
        self.user_q = torch.zeros(self.B, self.ld)
        self.user_q[:, :d] = r(self.B, d) * 0.5
        self.user_off = r(self.B) * 0.5
        self.ffn_b = r(1) * 0.5
        self.K = [r(n, d) * 1.2 for n in nv]
        self.U = [r(n, H) for n in nv]
        self.ids = [torch.randint(1, id_hi or n_items, (n,), generator=g, dtype=torch.int32) for n in nv]
        self.g = g
        self.dev = {k: getattr(self, k).cuda() for k in ("item_q", "item_w", "user_q", "user_off", "ffn_b")}

    def layout(self, L, positions):
        """positions[u]: ascending slot positions of user u's valid slots.  Every other slot is a pad (id 0) whose K / u
        rows hold large values no kernel may read."""
        B, d, H = self.B, self.d, self.H
        p_ids = torch.zeros(B, L, dtype=torch.int32)
        k = torch.full((B * L, self.ld), 1e4)
        u = torch.full((B * L, 4), -1e4)
        for b in range(B):
            pos = torch.as_tensor(positions[b], dtype=torch.int64)
            assert pos.numel() == self.nv[b] and (pos.numel() < 2 or bool((pos[1:] > pos[:-1]).all()))
            p_ids[b, pos] = self.ids[b]
            k[b * L + pos, :d] = self.K[b]
            u[b * L + pos, :H] = self.U[b]
        return dict(L=L, p_ids=p_ids.cuda(), user_k=k.cuda(), user_u=u.cuda())

    def fill(self, D, lay, excl):
        D.B, D.L, D.n_items, D.d, D.H, D.decoder = self.B, lay["L"], self.n_items, self.d, self.H, 0
        D.p_ids, D.ld_p_ids = lay["p_ids"].data_ptr(), lay["L"]
        D.item_q, D.ld_item_q = self.dev["item_q"].data_ptr(), self.ld
        D.item_w, D.ld_item_w = self.dev["item_w"].data_ptr(), 1
        D.user_k, D.ld_user_k = lay["user_k"].data_ptr(), self.ld
        D.user_u, D.ld_user_u = lay["user_u"].data_ptr(), 4
        D.user_q, D.ld_user_q = self.dev["user_q"].data_ptr(), self.ld
        D.user_off, D.ld_user_off = self.dev["user_off"].data_ptr(), 1
        D.ffn_b = self.dev["ffn_b"].data_ptr()
        if excl is not None:
            D.exclude, D.n_exclude, D.ld_exclude = excl.data_ptr(), excl.shape[1], excl.shape[1]

    def _run(self, D, entry, second, n, cand):
        outs = (torch.empty(self.B, n, device="cuda"), torch.empty(self.B, n, dtype=torch.int64, device="cuda"))
        for name, t in zip(("scores", second), outs):
            setattr(D, name, t.data_ptr())
            setattr(D, "ld_" + name, n)
        lib = _lib.load()
        if cand is None:
            rc = getattr(lib, entry)(C.byref(D), ops._stream())
        else:
            rc = getattr(lib, entry + "_among")(C.byref(D), C.byref(_lib.Candidates(cand.data_ptr(), cand.shape[0])),
                                                ops._stream())
        _lib.check(rc, entry)
        torch.cuda.synchronize()
        return outs[0].cpu(), outs[1].cpu()

    def recommend(self, lay, k, excl, cand=None):
        D = _lib.RecommendDesc()
        self.fill(D, lay, excl)
        D.k = k
        return self._run(D, "carca_recommend", "ids_out", k, cand)

    def rank(self, lay, items, excl, cand=None):
        D = _lib.RankDesc()
        self.fill(D, lay, excl)
        D.items, D.n_list, D.ld_items = items.data_ptr(), items.shape[1], items.shape[1]
        return self._run(D, "carca_rank_items", "ranks", items.shape[1], cand)

    def ref_scores(self):
        """float64 sigmoid(logit) [B, n_items] of DESIGN section 10's cross-attention formula over these tables."""
        d, H, dh = self.d, self.H, self.d // self.H
        q = self.item_q[:, :d].double().view(self.n_items, H, dh)
        out = torch.zeros(self.B, self.n_items, dtype=torch.float64)
        for b in range(self.B):
            att = torch.zeros(self.n_items, dtype=torch.float64)
            if self.nv[b]:
                K = self.K[b].double().view(-1, H, dh)
                s = torch.einsum("nhc,lhc->nhl", q + self.user_q[b, :d].double().view(1, H, dh), K) / math.sqrt(dh)
                att = (torch.softmax(s, dim=-1) * self.U[b].double().t().unsqueeze(0)).sum(dim=(1, 2))
            out[b] = torch.sigmoid(att + self.item_w.double() + self.user_off[b].double() + self.ffn_b.double())
        return out


def _scattered(nv, L, g):
    """nv ascending positions in [0, L), on both sides of every 64-position boundary where nv allows."""
    forced = [p for b in range(64, L, 64) for p in (b - 1, b)][:nv]
    rest = [p for p in torch.randperm(L, generator=g).tolist() if p not in forced][: nv - len(forced)]
    return sorted(forced + rest)


@pytest.mark.parametrize("dH", GEOMS, ids=[f"{d}x{H}" for d, H in GEOMS])
def test_long_kernels_equal_short_kernels_bit_for_bit(dH):
    d, H = dH
    n_items, k = 600, 20
    nv = [0, 64, 1, 37, 17]
    T = Tables(d, H, n_items, nv, seed=d)
    g = T.g
    # a wide exclusion list with zeros and repeats (wider than one round of the list kernel), the same for every layout
    excl = torch.randint(0, n_items, (T.B, 280), generator=g, dtype=torch.int32)
    excl[:, ::3] = 0
    excl = excl.cuda()
    items = torch.randint(1, n_items, (T.B, 9), generator=g, dtype=torch.int32)
    items[:, 0], items[:, 1], items[:, 2], items[:, 3] = 0, n_items + 5, excl[:, 1].cpu(), items[:, 4]
    items = items.cuda()
    cand = torch.arange(2, n_items, 2, dtype=torch.int32)[torch.randperm(299, generator=g)[:290].sort().values].cuda()
    lays = {
        64: T.layout(64, [list(range(64 - n, 64)) for n in nv]),
        128: T.layout(128, [list(range(128 - n, 128)) for n in nv]),  # 64 leading pads and more
        200: T.layout(200, [_scattered(n, 200, g) for n in nv]),      # id-0 holes between the valid slots
    }
    want = None
    for L, lay in lays.items():
        got = (T.recommend(lay, k, excl), T.rank(lay, items, excl), T.recommend(lay, k, excl, cand),
               T.rank(lay, items, excl, cand), T.recommend(lay, k, None))
        if want is None:
            want = got
            assert int((want[0][1] != 0).sum()) == T.B * k  # (real lists, not padding)
            assert set(want[1][1][:, 0].tolist()) == {-1} and int(want[1][1][:, 4:].min()) >= 0
            continue
        for a, b in zip(got, want):
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), L


COUNTS = (65, 128, 129, 1024)


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("dH", GEOMS, ids=[f"{d}x{H}" for d, H in GEOMS])
def test_more_than_64_valid_slots_against_float64(dH, count):
    d, H = dH
    n_items, k, B = 300, 10, 2
    L = min(1024, count + 3)
    nv = [count, count // 2 + 1]
    T = Tables(d, H, n_items, nv, seed=1000 * d + count, id_hi=40)  # (profile ids below 40: excluding them leaves a catalogue)
    for b in range(B):  # a slot that dominates many items' softmax arrives first in the second chunk: the running
        if nv[b] > 64:  # (m, den, num) of the first chunk must be rescaled there
            T.K[b][64] *= 2.5
    lay = T.layout(L, [_scattered(n, L, T.g) for n in nv])
    excl = lay["p_ids"]  # the whole profile, L wide
    ref = T.ref_scores()
    excl_sets = [set(T.ids[b].tolist()) for b in range(B)]
    ws, wi, full = _oracle_topk(ref[:, 1:], excl_sets, k)
    gs, gi = T.recommend(lay, k, excl)
    err = float((gs.double() - ws).abs().max())
    print(f"d={d} H={H} valid slots={count}: max |score - float64| = {err:.2e}")
    _check((gs, gi), (ws, wi), full, k, atol=1e-5)
    for b in range(B):
        assert not set(gi[b].tolist()) & excl_sets[b]
    rs, rr = T.rank(lay, gi.to(torch.int32).cuda(), excl)
    assert torch.equal(rr, torch.arange(k).expand(B, k))
    assert torch.equal(rs, gs)


# ---- model level -----------------------------------------------------------------------------------------------------
def _profiles(B, L, n_items, n_ctx, lens, seed):
    rng = np.random.default_rng(seed)
    p_x = torch.zeros(B, L, dtype=torch.int64)
    for b, ell in enumerate(lens):
        if ell:
            p_x[b, L - ell:] = torch.from_numpy(rng.integers(1, n_items, size=ell))
    p_c = torch.from_numpy(rng.random((B, L, n_ctx))).double() * (p_x != 0).unsqueeze(-1)
    return p_x, p_c


# (d, H, embedding, decoder, encoding, residual_ca, L, n_items, k, n_ctx, n_blocks, l2)
MODEL_CASES = [
    (90, 3, "all", "ca", "identity", True, 100, 300, 10, 6, 2, False),
    (64, 4, "attrctx", "ca", "learnable", False, 65, 300, 10, 6, 1, False),
    (128, 1, "id", "ca", "positional", True, 200, 300, 20, 0, 1, False),
    (64, 2, "all", "dot", "identity", True, 200, 300, 10, 6, 1, False),
    (90, 3, "attrctx", "wdot", "learnable", True, 65, 300, 10, 6, 1, True),
    (100, 5, "all", "dot", "identity", True, 20, 300, 10, 6, 1, False),  # an encoder geometry with no fused kernel
]


@pytest.mark.parametrize("case", MODEL_CASES, ids=[f"{c[0]}x{c[1]}-{c[2]}-{c[3]}{'-l2' if c[11] else ''}-L{c[6]}-nb{c[10]}"
                                                   for c in MODEL_CASES])
def test_recommend_matches_oracle_past_the_fused_envelope(case):
    d, H, emb, dec, enc, res, L, n, k, n_ctx, nb, l2 = case
    B = 5
    cfg, P, attrs, batch, model = _setup(d, H, emb, dec, enc, res, L, B, n, n_ctx, nb, l2)
    lens = [0, 1, min(64, L), min(65, L), L]
    p_x, p_c = _profiles(B, L, n, n_ctx, lens, seed=11)
    ctx = batch[2]
    y = _oracle_scores(cfg, P, attrs, (p_x, p_c, ctx), n)
    ws, wi, full = _oracle_topk(y, _excl_sets(p_x), k)
    prof = (p_x.cuda(), None, p_c.float().cuda())
    assert ops.use_composed(d, [H], L)
    with pytest.raises(CarcaHipError):
        model.recommend(prof, ctx.float().cuda(), k=k)
    got = model.recommend(prof, ctx.float().cuda(), k=k, allow_composed=True)
    print(f"{case}: max |score - oracle| = {float((got[0].cpu().double() - ws).abs().max()):.2e}")
    _check(got, (ws, wi), full, k, atol=2e-5)
    # scores of the returned ids equal the model's own (composed) forward over them as one target group
    gs, gi = got
    live = gi.cpu() != 0
    assert live.any()
    o_x = gi.clamp(min=1)
    o_c = ctx.float().cuda().unsqueeze(1).expand(B, k, n_ctx).contiguous()
    af = attrs.float().cuda()
    with torch.no_grad():
        yf = model((p_x.cuda(), af[p_x.cuda()], p_c.float().cuda()), [(o_x, af[o_x], o_c)])
    yf = yf.reshape(B, k).cpu()
    assert float((yf[live] - gs.cpu()[live]).abs().max()) < 1e-5
    # and rank_items places them where recommend did
    rs, rr = model.rank_items(prof, ctx.float().cuda(), gi, allow_composed=True)
    assert torch.equal(rs.cpu()[live], gs.cpu()[live])
    assert torch.equal(rr.cpu()[live], torch.arange(k).expand(B, k)[live])


def test_exclusion_and_candidates_at_length():
    d, H, L, n, n_ctx, B, k = 64, 4, 200, 600, 6, 3, 128
    cfg, P, attrs, batch, model = _setup(d, H, "all", "ca", "identity", True, L, B, n, n_ctx, 1)
    rng = np.random.default_rng(5)
    p_x = torch.stack([torch.from_numpy(rng.permutation(np.arange(1, n))[:L]) for _ in range(B)])  # 200 distinct ids
    p_c = torch.from_numpy(rng.random((B, L, n_ctx))).double()
    prof, c = (p_x.cuda(), None, p_c.float().cuda()), batch[2].float().cuda()
    s_all, i_all = (t.cpu() for t in model.recommend(prof, c, k=k, exclude=None, allow_composed=True))
    s_pr, i_pr = (t.cpu() for t in model.recommend(prof, c, k=k, allow_composed=True))  # exclude="profile"
    S = CandidateSet(torch.arange(1, n)[torch.arange(1, n) % 3 != 0], n, device="cuda")
    s_ca, i_ca = (t.cpu() for t in model.recommend(prof, c, k=k, candidates=S, allow_composed=True))
    in_S = set(S.ids.tolist())
    for b in range(B):
        own = set(p_x[b].tolist())
        assert len(own) == L and own & set(i_all[b].tolist())  # (the profile's items do rank in the unrestricted list)
        assert not own & set(i_pr[b].tolist()) and not own & set(i_ca[b].tolist())
        # the excluding call is the unrestricted order with the profile's items taken out
        keep = [j for j in range(k) if int(i_all[b, j]) not in own]
        assert i_pr[b, :len(keep)].tolist() == i_all[b, keep].tolist()
        assert torch.equal(s_pr[b, :len(keep)], s_all[b, keep])
        # the restricted call is the excluding order with the items outside S taken out
        assert set(i_ca[b].tolist()) <= in_S
        keep = [j for j in range(k) if int(i_pr[b, j]) in in_S]
        assert i_ca[b, :len(keep)].tolist() == i_pr[b, keep].tolist()
        assert torch.equal(s_ca[b, :len(keep)], s_pr[b, keep])
    # rank_items agrees under both
    want = torch.arange(k).expand(B, k)
    for ids, scores, kw in ((i_pr, s_pr, {}), (i_ca, s_ca, dict(candidates=S))):
        rs, rr = model.rank_items(prof, c, ids.cuda(), allow_composed=True, **kw)
        assert torch.equal(rr.cpu(), want) and torch.equal(rs.cpu(), scores)
    # an excluded item keeps the position it would take: a profile item's rank counts only eligible items before it
    rs, rr = model.rank_items(prof, c, p_x[:, :5].cuda(), allow_composed=True)
    rs0, rr0 = model.rank_items(prof, c, p_x[:, :5].cuda(), exclude=None, allow_composed=True)
    assert torch.equal(rs, rs0) and bool((rr <= rr0).all()) and bool((rr >= rr0 - (L - 1)).all())


def _long_log(n_users, n_items, n_ctx, seed):
    rng = np.random.default_rng(seed)
    profiles, ctxd = {}, {}
    for u in range(n_users):
        items = [int(v) for v in rng.integers(1, n_items, size=int(rng.integers(4, 110)))]
        profiles[u] = items
        for it in items:
            ctxd[(u, it)] = rng.random(n_ctx).astype(np.float32)
    return profiles, ctxd


def test_evaluate_full_and_ranks_at_80_slots():
    from carca_replication_amd.device_data import DeviceInteractions, DeviceLoader
    from carca_replication_amd.train import evaluate_full, evaluate_full_ranks, full_rank_metrics
    from tests.test_hip_rank import _oracle_full_ranks
    from tests.test_hip_recommend import _oracle_full_metrics

    n_items, n_ctx, L, k = 200, 6, 80, 10
    cfg, P, attrs, _, model = _setup(64, 2, "all", "ca", "identity", True, L, 2, n_items, n_ctx, 1)
    profiles, ctxd = _long_log(16, n_items, n_ctx, 3)
    log = DeviceInteractions(profiles, ctxd, n_items)
    loader = DeviceLoader(log, "test", batch_size=8, profile_seq_len=L, target_seq_len=10)
    batches = [(p_x.cpu(), p_c.double().cpu(), o_x.cpu(), o_c.double().cpu()) for p_x, _, p_c, o_x, _, o_c, _ in loader]
    assert max(int((b[0] != 0).sum(1).max()) for b in batches) > 64  # (profiles the fused kernels cannot hold)
    hr_w, ndcg_w, amb = _oracle_full_metrics(cfg, P, attrs, batches, k)
    assert amb < 0.1
    hr, ndcg = evaluate_full(model, loader, "cuda", k)
    assert abs(hr - hr_w) <= amb + 1e-9 and abs(ndcg - ndcg_w) <= amb + 1e-6
    want_r, amb_n = _oracle_full_ranks(cfg, P, attrs, batches)
    assert amb_n < 3
    ks = (1, 5, 10, 150)
    want, got = full_rank_metrics(want_r, ks), evaluate_full_ranks(model, loader, "cuda", ks=ks)
    assert got["users"] == len(want_r)
    assert got[f"HR@{k}"] == hr and abs(got[f"NDCG@{k}"] - ndcg) < 1e-6
    tol = amb_n / len(want_r) + 1e-9
    for kk in ks:
        assert abs(got[f"HR@{kk}"] - want[f"HR@{kk}"]) <= tol
    assert abs(got["MRR"] - want["MRR"]) <= tol


def test_envelope():
    _, _, _, batch, model = _setup(64, 2, "all", "ca", "identity", True, 16, 2, 300, 6, 1)
    c = batch[2].float().cuda()
    ones = lambda L: (torch.ones(2, L, dtype=torch.int64).cuda(), None, torch.zeros(2, L, 6).cuda())  # noqa: E731
    items = torch.ones(2, 1, dtype=torch.int64).cuda()
    with pytest.raises(CarcaHipError, match="64"):
        model.recommend(ones(65), c, k=10)
    with pytest.raises(CarcaHipError, match="64"):
        model.rank_items(ones(65), c, items)
    with pytest.raises(CarcaHipError, match="1024"):
        model.recommend(ones(1025), c, k=10, allow_composed=True)
    with pytest.raises(CarcaHipError, match="1024"):
        model.rank_items(ones(1025), c, items, allow_composed=True)
    model.train()
    for call in (lambda: model.recommend(ones(65), c, k=10, allow_composed=True),
                 lambda: model.rank_items(ones(65), c, items, allow_composed=True)):
        with pytest.raises(CarcaHipError, match="eval"):
            call()
    model.eval()
    s, i = model.recommend(ones(65), c, k=10, allow_composed=True)  # (the same call in eval mode is served)
    assert s.shape == (2, 10) and int(i.min()) >= 2
    _, _, _, b48, m48 = _setup(48, 1, "id", "ca", "identity", True, 8, 2, 50, 0, 1)
    with pytest.raises(CarcaHipError, match=r"\(48, 1\)"):
        m48.recommend((b48[0].cuda(), None, b48[1].float().cuda()), None, k=5, allow_composed=True)
    _, _, _, b256, m256 = _setup(256, 2, "id", "dot", "identity", True, 8, 2, 50, 0, 1)
    with pytest.raises(CarcaHipError, match="128"):
        m256.recommend((b256[0].cuda(), None, b256[1].float().cuda()), None, k=5, allow_composed=True)
    # the C ABI: L beyond CARCA_MAX_PROFILE_L is unsupported, whatever the decoder
    T = Tables(64, 4, 300, [3], seed=0)
    lay = T.layout(64, [[61, 62, 63]])
    lay["L"] = 1025
    with pytest.raises(CarcaHipError, match="1024"):
        T.recommend(lay, 5, None)
