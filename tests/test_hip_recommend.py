"""CARCA.recommend (full-catalogue top-k, csrc/recommend.hip) and train.evaluate_full against the fp64 CPU oracle: the
oracle scores every item 1..n_items-1 as ONE target group carrying the user's context (oracle.carca_forward, eval mode),
then takes the top k under the selection's rule (best first, ties to the smaller id, excluded ids never)."""
import pickle

import numpy as np
import pytest
import torch

from oracle import carca_oracle as O
from tests.model_util import build_model

pytestmark = pytest.mark.gpu

G, N_ATTRS = 24, 12


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
    # (one trailing padding target, dropped: keeps the reference's bare squeeze off a 1 x 1 score matrix)
    ids = torch.cat([torch.arange(1, n_items), torch.zeros(1, dtype=torch.int64)]).expand(B, -1)
    o_c = ctx.unsqueeze(1).expand(B, n_items, ctx.shape[1])
    y = O.carca_forward(P, cfg, (p_x, attrs[p_x], p_c), [(ids, attrs[ids], o_c)], training=False)
    return y.reshape(B, n_items)[:, :-1]


def _oracle_topk(y, excl, k):
    """y [B, n-1] for ids 1..n-1; excl: list of sets.  -> (scores [B, k], ids [B, k], sorted eligible scores per user)"""
    B = y.shape[0]
    out_s, out_i, full = torch.zeros(B, k, dtype=torch.float64), torch.zeros(B, k, dtype=torch.int64), []
    for b in range(B):
        ids = torch.tensor([i for i in range(1, y.shape[1] + 1) if i not in excl[b]], dtype=torch.int64)
        if ids.numel() == 0:
            full.append(torch.zeros(0, dtype=torch.float64))
            continue
        s = y[b, ids - 1]
        order = torch.sort(s, descending=True, stable=True).indices  # (ids ascending: ties to the smaller id)
        m = min(k, ids.numel())
        out_s[b, :m], out_i[b, :m] = s[order[:m]], ids[order[:m]]
        full.append(s[order])
    return out_s, out_i, full


def _check(got, want, full, k, atol=2e-5):
    gs, gi = (t.cpu() for t in got)
    ws, wi = want
    assert gs.shape == (ws.shape[0], k) and gi.dtype == torch.int64
    assert float((gs.double() - ws).abs().max()) < atol
    for b in range(ws.shape[0]):
        s = full[b]
        m = min(k, s.numel())
        assert torch.all(gi[b, m:] == 0) and torch.all(gs[b, m:] == 0)
        for r in range(m):  # ids must agree wherever the oracle's neighbours are clearly apart
            lo = s[r - 1] - s[r] if r > 0 else torch.tensor(1.0)
            hi = s[r] - s[r + 1] if r + 1 < s.numel() else torch.tensor(1.0)
            if min(float(lo), float(hi)) > 1e-5:
                assert int(gi[b, r]) == int(wi[b, r]), (b, r)


def _excl_sets(p_x, extra=None):
    return [set(p_x[b].tolist()) - {0} | (set(extra[b].tolist()) - {0} if extra is not None else set())
            for b in range(p_x.shape[0])]


# (d, H, embedding, decoder, encoding, residual_ca, L, B, n_items, k, n_ctx, n_blocks, l2)
CASES = [
    (64, 4, "all", "ca", "identity", True, 16, 5, 300, 10, 6, 1, False),
    (64, 4, "attrctx", "ca", "learnable", False, 1, 1, 2, 10, 6, 0, False),
    (62, 2, "id", "ca", "positional", True, 17, 300, 300, 128, 0, 1, False),
    (62, 2, "mlpid", "ca", "identity", False, 64, 5, 4097, 100, 0, 2, False),
    (64, 1, "attr", "ca", "learnable", True, 50, 5, 300, 1, 6, 1, False),
    (64, 1, "all", "ca", "positional", False, 16, 5, 4097, 10, 6, 1, False),
    (90, 3, "all", "ca", "identity", True, 50, 5, 4097, 100, 6, 2, False),
    (90, 3, "attrctx", "ca", "positional", False, 64, 1, 300, 128, 6, 1, False),
    (96, 2, "id", "ca", "learnable", True, 1, 5, 300, 10, 0, 1, False),
    (96, 2, "all", "ca", "identity", False, 17, 5, 2, 1, 6, 1, False),
    (90, 1, "mlpid", "ca", "positional", True, 16, 1, 4097, 10, 0, 1, False),
    (90, 1, "attr", "ca", "identity", False, 50, 300, 300, 100, 0, 1, False),
    (128, 4, "all", "ca", "learnable", True, 64, 5, 300, 128, 6, 1, False),
    (128, 4, "id", "ca", "identity", False, 17, 5, 4097, 1, 0, 1, False),
    (120, 2, "attrctx", "ca", "identity", True, 16, 5, 300, 10, 6, 1, False),
    (120, 2, "all", "ca", "positional", False, 1, 300, 300, 10, 6, 1, False),
    (128, 1, "mlpid", "ca", "learnable", True, 50, 5, 300, 100, 0, 1, False),
    (128, 1, "attr", "ca", "positional", False, 64, 5, 2, 128, 0, 1, False),
    (64, 2, "all", "dot", "identity", True, 16, 5, 4097, 10, 6, 1, False),
    (90, 3, "attrctx", "wdot", "learnable", True, 50, 300, 300, 100, 6, 1, False),
    (96, 2, "all", "wdot", "positional", True, 17, 5, 4097, 128, 6, 1, True),
    (128, 4, "id", "wdot", "identity", True, 1, 1, 300, 10, 0, 1, True),
    (64, 1, "mlpid", "dot", "positional", True, 64, 5, 300, 1, 0, 2, False),
]


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}x{c[1]}-{c[2]}-{c[3]}{'-l2' if c[12] else ''}-{c[4][:3]}-"
                                             f"res{int(c[5])}-L{c[6]}-B{c[7]}-n{c[8]}-k{c[9]}" for c in CASES])
def test_recommend_matches_oracle(case):
    d, H, emb, dec, enc, res, L, B, n, k, n_ctx, nb, l2 = case
    cfg, P, attrs, batch, model = _setup(d, H, emb, dec, enc, res, L, B, n, n_ctx, nb, l2)
    p_x, p_c, ctx = batch
    y = _oracle_scores(cfg, P, attrs, batch, n)
    ws, wi, full = _oracle_topk(y, _excl_sets(p_x), k)
    got = model.recommend((p_x.cuda(), None, p_c.float().cuda()), ctx.float().cuda(), k=k)
    _check(got, (ws, wi), full, k)
    # scores of the returned ids equal the model's own forward over them as one target group
    gs, gi = got
    live = gi.cpu() != 0
    if live.any():
        o_x = gi.clamp(min=1)
        o_c = ctx.float().cuda().unsqueeze(1).expand(B, k, n_ctx).contiguous()
        o_a = attrs.float().cuda()[o_x]
        with torch.no_grad():
            yf = model(((p_x.cuda(), attrs.float().cuda()[p_x.cuda()], p_c.float().cuda())), [(o_x, o_a, o_c)])
        yf = yf.reshape(B, k).cpu()
        assert float((yf[live] - gs.cpu()[live]).abs().max()) < 1e-5


def test_exclusion_rules():
    cfg, P, attrs, batch, model = _setup(64, 2, "all", "ca", "identity", True, 16, 5, 300, 6, 1)
    p_x, p_c, ctx = batch
    y = _oracle_scores(cfg, P, attrs, batch, 300)
    prof = (p_x.cuda(), None, p_c.float().cuda())
    c = ctx.float().cuda()
    # no exclusion: the profile's own items are eligible (and some of them rank in the top k)
    s0, i0 = model.recommend(prof, c, k=50, exclude=None)
    ws, wi, full = _oracle_topk(y, [set() for _ in range(5)], 50)
    _check((s0, i0), (ws, wi), full, 50)
    # "profile" removes exactly those
    s1, i1 = model.recommend(prof, c, k=50)
    hit = [set(i0[b].tolist()) & (set(p_x[b].tolist()) - {0}) for b in range(5)]
    assert any(hit)
    for b in range(5):
        assert not (set(i1[b].tolist()) & (set(p_x[b].tolist()) - {0}))
    # an explicit list with duplicates and zeros
    extra = torch.tensor([[int(wi[b, 0]), int(wi[b, 0]), 0, int(wi[b, 3])] for b in range(5)], dtype=torch.int32)
    s2, i2 = model.recommend(prof, c, k=20, exclude=extra.cuda())
    ws, wi2, full = _oracle_topk(y, [set(extra[b].tolist()) - {0} for b in range(5)], 20)
    _check((s2, i2), (ws, wi2), full, 20)
    # everything excluded: all padding
    allx = torch.arange(300, dtype=torch.int64).expand(5, -1).cuda()
    s3, i3 = model.recommend(prof, c, k=10, exclude=allx)
    assert torch.all(i3 == 0) and torch.all(s3 == 0)


def test_cache_follows_weights_and_stays_out_of_pickles():
    from carca_replication_amd.optim import Adam

    cfg, P, attrs, batch, model = _setup(64, 4, "all", "ca", "learnable", True, 16, 5, 300, 6, 1)
    p_x, p_c, ctx = batch
    prof, c = (p_x.cuda(), None, p_c.float().cuda()), ctx.float().cuda()
    a = model.recommend(prof, c, k=10)
    b = model.recommend(prof, c, k=10)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])  # bit-identical
    assert "_item_table_cache" in model.embeds.__dict__ and "_reco_cache" in model.decoder.__dict__
    blob = pickle.dumps(model)
    assert b"_item_table_cache" not in blob and b"_reco_cache" not in blob and b"_ctx_matrix_cache" not in blob
    # load_state_dict: new weights
    P2 = O.perturb_params(O.init_params(cfg, 300, G, 6, N_ATTRS, 16, seed=5, dtype=torch.float64), seed=6)
    model.load_state_dict({k: v.float() for k, v in P2.items()})
    ws, wi, full = _oracle_topk(_oracle_scores(cfg, P2, attrs, batch, 300), _excl_sets(p_x), 10)
    _check(model.recommend(prof, c, k=10), (ws, wi), full, 10)
    # re-registered attribute table
    attrs2 = attrs.clone()
    attrs2[1:] = attrs2[1:].flip(0)
    model.embeds.register_attr_table(attrs2.float().cuda())
    ws, wi, full = _oracle_topk(_oracle_scores(cfg, P2, attrs2, batch, 300), _excl_sets(p_x), 10)
    _check(model.recommend(prof, c, k=10), (ws, wi), full, 10)
    # a project Adam step
    model.train()
    opt = Adam(model.parameters(), lr=1e-2)
    with torch.no_grad():
        for p in model.parameters():
            p.grad = torch.randn_like(p) * 0.1
    opt.step()
    model.eval()
    P3 = {k: v.detach().double().cpu() for k, v in model.state_dict().items()}
    ws, wi, full = _oracle_topk(_oracle_scores(cfg, P3, attrs2, batch, 300), _excl_sets(p_x), 10)
    _check(model.recommend(prof, c, k=10), (ws, wi), full, 10)


def test_envelope_errors():
    from carca_replication_amd import CarcaHipError

    _, _, _, batch, model = _setup(64, 2, "all", "ca", "identity", True, 16, 2, 300, 6, 1)
    p_x, p_c, ctx = batch
    prof, c = (p_x.cuda(), None, p_c.float().cuda()), ctx.float().cuda()
    with pytest.raises(CarcaHipError, match="128"):
        model.recommend(prof, c, k=129)
    model.train()
    with pytest.raises(CarcaHipError, match="eval"):
        model.recommend(prof, c, k=10)
    model.eval()
    long = torch.ones(2, 65, dtype=torch.int64).cuda()
    with pytest.raises(CarcaHipError, match="64"):
        model.recommend((long, None, torch.zeros(2, 65, 6).cuda()), c, k=10)
    model.embeds.register_attr_table(None)
    with pytest.raises(CarcaHipError, match="register_attr_table"):
        model.recommend(prof, c, k=10)
    _, _, _, batch, m48 = _setup(48, 1, "id", "ca", "identity", True, 8, 2, 50, 0, 1)
    with pytest.raises(CarcaHipError, match=r"\(48, 1\)"):
        m48.recommend((batch[0].cuda(), None, batch[1].float().cuda()), None, k=5)


def test_c2_sized_against_chunked_forward():
    """C2 dimensions: 12,102 items, 4096 attributes, d 90, H 3, 2 blocks, B = 128; the reference is the model's own forward
    over the whole catalogue in chunks of target groups (pinned to the oracle by the forward's own tests)."""
    torch.manual_seed(0)
    from carca_replication_amd import modules as M

    n_items, n_attrs, n_ctx, d, H, L, B, k = 12102, 4096, 6, 90, 3, 50, 128, 10
    enc = M.IdentityEncoding()
    model = M.CARCA(d, 0.0, M.AllEmbedding(n_items, d, 450, n_ctx, n_attrs, enc),
                    torch.nn.ModuleList([M.SelfAttentionBlock(d, H, 0.0, True) for _ in range(2)]),
                    M.CrossAttentionBlock(d, H, 0.0, True)).cuda().eval()
    gen = torch.Generator().manual_seed(1)
    attrs = (torch.rand(n_items, n_attrs, generator=gen) < 0.01).float()
    attrs[0] = 0
    model.embeds.register_attr_table(attrs.cuda())
    lens = torch.randint(3, L + 1, (B,), generator=gen)
    p_x = torch.randint(1, n_items, (B, L), generator=gen) * (torch.arange(L) >= (L - lens).unsqueeze(1))
    p_c = torch.rand(B, L, n_ctx, generator=gen) * (p_x != 0).unsqueeze(-1)
    ctx = torch.rand(B, n_ctx, generator=gen)
    p_x, p_c, ctx = p_x.cuda(), p_c.cuda(), ctx.cuda()
    s, i = model.recommend((p_x, None, p_c), ctx, k=k)
    ys = []
    with torch.no_grad():
        for lo in range(1, n_items, 1024):
            ids = torch.arange(lo, min(lo + 1024, n_items), device="cuda").expand(B, -1).contiguous()
            oc = ctx.unsqueeze(1).expand(B, ids.shape[1], n_ctx).contiguous()
            ys.append(model((p_x, None, p_c), [(ids, None, oc)]).reshape(B, -1))
    y = torch.cat(ys, 1).double().cpu()
    ws, wi, full = _oracle_topk(y, _excl_sets(p_x.cpu()), k)
    _check((s, i), (ws, wi), full, k, atol=1e-5)


def _log(n_users, n_items, n_ctx, seed):
    rng = np.random.default_rng(seed)
    profiles, ctxd = {}, {}
    for u in range(n_users):
        items = [int(v) for v in rng.integers(1, n_items, size=int(rng.integers(4, 20)))]
        profiles[u] = items
        for it in items:
            ctxd[(u, it)] = rng.random(n_ctx).astype(np.float32)
    return profiles, ctxd


def _oracle_full_metrics(cfg, P, attrs, batches, k):
    hr = ndcg = 0.0
    amb, users = 0, 0
    for p_x, p_c, o_x, o_c in batches:
        n = attrs.shape[0]
        y = _oracle_scores(cfg, P, attrs, (p_x, p_c, o_c[:, 0]), n)
        for b in range(p_x.shape[0]):
            pos = int(o_x[b, 0])
            excl = set(p_x[b].tolist()) - {0, pos}
            ids = torch.tensor([i for i in range(1, n) if i not in excl])
            s = y[b, ids - 1]
            sp = y[b, pos - 1]
            rank = int(((s > sp) | ((s == sp) & (ids < pos))).sum())
            amb += int(((s - sp).abs() < 1e-5).sum()) > 1
            if rank < k:
                hr += 1
                ndcg += 1.0 / np.log2(rank + 2)
            users += 1
    return hr / users, ndcg / users, amb / users


def test_evaluate_full_matches_oracle_full_ranking():
    from carca_replication_amd.device_data import DeviceInteractions, DeviceLoader
    from carca_replication_amd.train import evaluate_full

    n_items, n_ctx, L, k = 200, 6, 16, 10
    cfg, P, attrs, _, model = _setup(64, 2, "all", "ca", "identity", True, L, 2, n_items, n_ctx, 1)
    profiles, ctxd = _log(24, n_items, n_ctx, 3)
    log = DeviceInteractions(profiles, ctxd, n_items)
    loader = DeviceLoader(log, "test", batch_size=8, profile_seq_len=L, target_seq_len=10)
    batches = [(p_x.cpu(), p_c.double().cpu(), o_x.cpu(), o_c.double().cpu()) for p_x, _, p_c, o_x, _, o_c, _ in loader]
    hr_w, ndcg_w, amb = _oracle_full_metrics(cfg, P, attrs, batches, k)
    assert amb < 0.1
    host = [(p_x, attrs.float()[p_x.long()], p_c.float(), o_x, attrs.float()[o_x.long()], o_c.float(), torch.zeros_like(o_x))
            for p_x, p_c, o_x, o_c in batches]
    for ld in (loader, host):
        hr, ndcg = evaluate_full(model, ld, "cuda", k)
        assert abs(hr - hr_w) <= amb + 1e-9 and abs(ndcg - ndcg_w) <= amb + 1e-6
