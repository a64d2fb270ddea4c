"""BCE against K shared negatives, gBCE (ops.sampled_bce, CARCA.sampled_bce_loss, engine.train_step(loss="sampled_bce");
DESIGN.md section 16) on the GPU: the op against fp64 torch autograd with and without the context rows, large logits,
masking, the empty batch, run-to-run bits and memory; the model's loss and every parameter gradient against
torch.autograd over the oracle, every negative embedded with the row's own context; the training step."""
import math
import os
import random

import pytest
import torch
import torch.nn.functional as F

from carca_replication_amd import CarcaHipError, ops
from oracle import carca_oracle as O
from tests.test_hip_catalogue_xent import MODEL_CASES, N_ATTRS, _setup
from tests.test_sampled_bce_host import ref_bce

pytestmark = pytest.mark.gpu


def _operands(R, K, d, n_items, seed):
    """As test_hip_sampled_xent._operands: 20 % padding rows (pos 0, negative, past the catalogue; never row 0), a third of
    the samples accidental hits of some row's positive, invalid sample ids, duplicates; plus the context rows C."""
    g = torch.Generator().manual_seed(seed)
    P = torch.randn(R, d, generator=g, dtype=torch.float64)
    Tp = torch.randn(R, d, generator=g, dtype=torch.float64) / d ** 0.5
    S = torch.randn(K, d, generator=g, dtype=torch.float64) / d ** 0.5
    Cr = torch.randn(R, d, generator=g, dtype=torch.float64) / d ** 0.5
    pos = torch.randint(1, n_items, (R,), generator=g)
    bad = torch.rand(R, generator=g) < 0.2
    bad[0] = False  # (the R = 1 cases keep their row)
    pos[bad] = torch.tensor([0, -3, n_items, n_items + 7])[torch.randint(0, 4, (int(bad.sum()),), generator=g)]
    s = torch.randint(1, n_items, (K,), generator=g)  # with replacement: duplicates
    if K > 2:
        s[: K // 3] = pos[torch.randint(0, R, (K // 3,), generator=g)]  # accidental hits (and some invalid ids)
        s[K - 1] = 0
    bad_s = torch.rand(K, generator=g) < 0.1
    s[bad_s] = torch.tensor([0, -1, n_items, n_items + 3])[torch.randint(0, 4, (int(bad_s.sum()),), generator=g)]
    return P, Tp, S, Cr, pos, s


def _strided(x, ld):
    """x [rows, d] fp32 as the first d columns of a [rows, ld] buffer filled with a sentinel past d."""
    buf = torch.full((x.shape[0], ld), 777.0, dtype=torch.float32, device="cuda")
    buf[:, : x.shape[1]] = x
    return buf[:, : x.shape[1]]


def _check_op(R, K, d, n_items=5000, seed=0, beta=0.4375, with_c=True, scale=1.0, ld=None):
    P64, T64, S64, C64, pos, s = _operands(R, K, d, n_items, seed)
    P64 = P64 * scale
    ref = [x.cuda().requires_grad_(True) for x in ((P64, T64, S64, C64) if with_c else (P64, T64, S64))]
    want = ref_bce(ref[0], ref[1], pos, ref[2], s, n_items, beta, ref[3] if with_c else None)
    want.backward()
    mk = (lambda x: _strided(x.float().cuda(), ld)) if ld else (lambda x: x.float().cuda())
    got_in = [mk(x).requires_grad_(True) for x in ((P64, T64, S64, C64) if with_c else (P64, T64, S64))]
    got = ops.sampled_bce(got_in[0], got_in[1], pos.cuda(), got_in[2], s.cuda(), n_items, beta,
                          C=got_in[3] if with_c else None)
    got.backward()
    w = want.item()
    print(f"R={R} K={K} d={d} C={with_c}: loss {got.item():.9g} want {w:.9g}")
    assert math.isfinite(got.item())
    assert abs(got.item() - w) <= 1e-5 * max(abs(w), 0.1), (got.item(), w)
    for name, g, r in zip(("P", "Tp", "S", "C"), got_in, ref):
        assert g.grad.shape == r.grad.shape, name
        assert bool(torch.isfinite(g.grad).all()), name
        err = float((g.grad.double() - r.grad).abs().max())
        print(f"  d{name}: err {err:.3g} max|ref| {float(r.grad.abs().max()):.3g}")
        assert err <= 1e-4 * float(r.grad.abs().max()) + 1e-9, (name, err, float(r.grad.abs().max()))
    return got_in


# R in {1, 17, 65, 700}, K in {1, 63, 64, 65, 130, 2048}, d in {64, 90, 128, 192, 256}: the three NCB instantiations, one
# below / at / one above a 64 tile in both operands, a ragged last tile
OP_CASES = [(1, 1, 64), (17, 63, 90), (17, 64, 128), (65, 65, 192), (700, 130, 256), (700, 2048, 90), (1, 2048, 128),
            (65, 64, 64), (17, 130, 256), (700, 1, 128), (65, 2048, 64), (1, 65, 192), (700, 63, 192), (17, 2048, 256),
            (65, 130, 90)]


@pytest.mark.parametrize("R,K,d", OP_CASES)
def test_op_matches_fp64_reference(R, K, d):
    _check_op(R, K, d, seed=R + K + d, with_c=True)
    _check_op(R, K, d, seed=R + K + d + 1, with_c=False)


def test_op_cases_cover_every_split_layout():
    cus = ops.num_cus()
    plans = {c: ops.sampled_bce_plan(*c, cus) for c in OP_CASES}
    assert plans[(17, 2048, 256)]["splits_samples"] > 1  # several sample splits (one row block)
    assert plans[(700, 63, 192)]["splits_rows"] > 1      # several row splits: dS through partials
    p = plans[(17, 63, 90)]
    assert p["splits_samples"] == 1 and p["splits_rows"] == 1  # one workgroup, dS written by the tile itself
    assert any(q["splits_samples"] > 1 and q["splits_rows"] > 1 for q in plans.values())


def test_op_strided_operands_leave_zeros_past_d():
    """Row stride past d (the model passes its padded rows): the low-level calls on [rows, ld] buffers whose columns past
    d hold a sentinel; every gradient is 0 there."""
    R, K, d, ld, n_items, beta = 65, 130, 90, 96, 5000, 0.4375
    P64, T64, S64, C64, pos, s = _operands(R, K, d, n_items, 21)
    _check_op(R, K, d, seed=21, ld=ld)  # (the op on strided views)
    full = [_strided(x.float().cuda(), ld)._base for x in (P64, T64, S64, C64)]
    P, Tp, S, Cr = full
    pos32, s32 = pos.int().cuda(), s.int().cuda()
    loss, saved, _ = ops.sampled_bce_fwd(P, Tp, Cr, pos32, S, s32, n_items, beta, d)
    dP, dTp, dS, dC = ops.sampled_bce_bwd(P, Tp, Cr, pos32, S, s32, n_items, beta, saved, torch.ones(1, device="cuda"), d)
    want = ref_bce(P64.cuda(), T64.cuda(), pos, S64.cuda(), s, n_items, beta, C64.cuda())
    assert abs(loss.item() - want.item()) <= 1e-5 * max(abs(want.item()), 0.1)
    for name, g in (("dP", dP), ("dTp", dTp), ("dS", dS), ("dC", dC)):
        assert g.shape[1] == ld and float(g[:, d:].abs().max()) == 0.0, name
        assert float(g[:, :d].abs().max()) > 0.0, name


@pytest.mark.parametrize("with_c", [True, False])
def test_op_large_logits_stay_finite(with_c):
    """P scaled so that |z| reaches about 80 on both signs: softplus(80) = 80 and exp(80) overflows fp32."""
    R, K, d, n_items = 65, 130, 128, 5000
    P64, T64, S64, C64, pos, s = _operands(R, K, d, n_items, 31)
    z = P64 @ S64.T + ((P64 * C64).sum(1, keepdim=True) if with_c else 0.0)
    scale = 80.0 / float(z.abs().max())
    assert float((z * scale).max()) > 60 and float((z * scale).min()) < -60
    _check_op(R, K, d, seed=31, with_c=with_c, scale=scale)


def test_op_small_catalogue_masks_most_samples():
    """n_items = 3: most samples are the row's own positive or no class at all; a row whose every sample is masked pays
    beta softplus(-z+) alone."""
    _check_op(300, 70, 90, n_items=3, seed=11)
    R, K, d, beta = 40, 70, 64, 0.3
    g = torch.Generator().manual_seed(5)
    P, Tp, Cr = (torch.randn(R, d, generator=g).cuda() for _ in range(3))
    S = torch.randn(K, d, generator=g).cuda()
    pos = torch.tensor([1, 2] * (R // 2), dtype=torch.int32).cuda()
    s = torch.tensor([1, 0, 3, -1, 7] * (K // 5), dtype=torch.int32).cuda()  # id 1 and ids that are no class
    loss, saved, row_loss = ops.sampled_bce_fwd(P, Tp, Cr, pos, S, s, 3, beta, d)
    zp = (P.double() * Tp.double()).sum(1)
    alone = beta * F.softplus(-zp)
    assert torch.allclose(row_loss[0::2].double(), alone[0::2], rtol=1e-5, atol=1e-6)  # pos 1: every sample masked
    assert float(saved[2][0::2].abs().max()) == 0.0  # ... and G_r = 0
    assert bool((row_loss[1::2].double() > alone[1::2] + 1e-3).all())  # pos 2: the K / 5 copies of id 1 are negatives


def test_op_no_valid_row_gives_zero_loss_and_gradients():
    P, Tp, Cr = (torch.randn(5, 90, device="cuda", requires_grad=True) for _ in range(3))
    S = torch.randn(33, 90, device="cuda", requires_grad=True)
    loss = ops.sampled_bce(P, Tp, torch.tensor([0, 0, -1, 40, 0], device="cuda"), S,
                           torch.randint(1, 40, (33,), device="cuda"), 40, 0.5, C=Cr)
    loss.backward()
    assert loss.item() == 0.0
    for g in (P.grad, Tp.grad, S.grad, Cr.grad):
        assert float(g.abs().max()) == 0.0


def test_op_two_calls_are_bit_identical():
    P64, T64, S64, C64, pos, s = _operands(700, 2048, 90, 5000, seed=5)
    outs = []
    for _ in range(2):
        P, Tp, S, Cr = (x.float().cuda().requires_grad_(True) for x in (P64, T64, S64, C64))
        loss = ops.sampled_bce(P, Tp, pos.cuda(), S, s.cuda(), 5000, 0.4375, C=Cr)
        loss.backward()
        outs.append((loss.detach().clone(), P.grad.clone(), Tp.grad.clone(), S.grad.clone(), Cr.grad.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_op_needs_no_logit_buffer():
    """R = 6,400, K = 16,384, d = 128: one [R, K] fp32 buffer is 419 MB; the op's memory beyond its inputs and the
    gradients it returns stays under a tenth of that."""
    R, K, d, n_items = 6400, 16384, 128, 1_000_001
    g = torch.Generator(device="cuda").manual_seed(0)
    P = torch.randn(R, d, device="cuda", generator=g).requires_grad_(True)
    Tp, Cr = ((torch.randn(R, d, device="cuda", generator=g) / d ** 0.5).requires_grad_(True) for _ in range(2))
    S = (torch.randn(K, d, device="cuda", generator=g) / d ** 0.5).requires_grad_(True)
    pos = torch.randint(0, n_items, (R,), device="cuda", generator=g)
    s = torch.randint(1, n_items, (K,), device="cuda", generator=g)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss = ops.sampled_bce(P, Tp, pos, S, s, n_items, 0.5, C=Cr)
    loss.backward()
    torch.cuda.synchronize()
    outputs = (P.grad.numel() + Tp.grad.numel() + S.grad.numel() + Cr.grad.numel()) * 4
    extra = torch.cuda.max_memory_allocated() - base - outputs
    print(f"extra {extra / 2 ** 20:.1f} MiB of {R * K * 4 / 2 ** 20:.0f}")
    assert extra < 0.1 * R * K * 4, extra / 2 ** 20
    assert math.isfinite(loss.item()) and loss.item() > 0


# ---- model level ---------------------------------------------------------------------------------------------------
N_ITEMS, K_MODEL, T_MODEL = 300, 200, 0.75


def _draw(pos, n_ctx, n_items=N_ITEMS, K=K_MODEL, seed=0):
    """K sample ids with duplicates, accidental hits of the batch's positives and invalid ids; the positives' context,
    different from the profile's."""
    g = torch.Generator().manual_seed(seed + 100)
    s = torch.randint(1, n_items, (K,), generator=g)
    flat = pos.reshape(-1)
    s[:10] = flat[torch.randint(0, flat.numel(), (10,), generator=g)]
    s[10:13] = torch.tensor([0, -2, n_items + 1])
    pos_ctx = torch.rand(*pos.shape, n_ctx, generator=g, dtype=torch.float64) * (pos != 0).unsqueeze(-1)
    return s, pos_ctx


def _oracle_loss(Pg, cfg, attrs, batch, pos_ctx, s, t, masks=None):
    """The profile rows of the oracle's forward; every negative embedded WITH THE ROW'S OWN CONTEXT through O.embedding
    (ids [B L, K], the context broadcast over K), the positive with pos_ctx; then the loss in fp64."""
    p_x, p_c, pos = batch
    B, L = p_x.shape
    trace = {}
    O.carca_forward(Pg, cfg, (p_x, attrs[p_x], p_c), [(pos, attrs[pos], pos_ctx)], training=True, trace=trace, masks=masks)
    p = trace["p_final"]
    if cfg.decoder == "wdot":  # p[t] * sum_{j<=t} gamma^j, the reference's float32 slot weights (carca.py:376,385-386)
        w = torch.tril((cfg.gamma ** torch.arange(0, L)).unsqueeze(0).expand(L, L)).to(p.dtype).sum(1)
        p = p * w.view(1, L, 1)
    fix = lambda x: torch.where((x >= 1) & (x < N_ITEMS), x, torch.zeros_like(x))  # noqa: E731
    R, K = B * L, s.numel()
    ids = fix(s).view(1, K).expand(R, K)
    ctx = pos_ctx.reshape(R, 1, -1).expand(R, K, pos_ctx.shape[-1])
    E = O.embedding(Pg, cfg, ids, attrs[ids], ctx, O.get_mask(ids, torch.float64), target=True)  # [R, K, d]
    tp = fix(pos)
    Tp = O.embedding(Pg, cfg, tp, attrs[tp], pos_ctx, O.get_mask(tp, torch.float64), target=True).reshape(R, -1)
    p = p.reshape(R, -1)
    posf, sl = pos.reshape(-1), s.long()
    valid = (posf >= 1) & (posf < N_ITEMS)
    neg = ((sl >= 1) & (sl < N_ITEMS)).view(1, K) & (sl.view(1, K) != posf.view(R, 1))
    beta = ops.sampled_bce_beta(K, N_ITEMS, t)
    zp = (p * Tp).sum(1)
    zs = torch.einsum("rd,rkd->rk", p, E)
    rows = beta * F.softplus(-zp) + (F.softplus(zs) * neg).sum(1)
    return (rows * valid).sum() / valid.sum()


def _run(model, batch, pos_ctx, s, t=T_MODEL):
    p_x, p_c, pos = batch
    model.zero_grad(set_to_none=True)
    a = None if hasattr(model.embeds, "register_attr_table") else torch.zeros(*p_x.shape, N_ATTRS, device="cuda")
    loss = model.sampled_bce_loss((p_x.cuda(), a, p_c.float().cuda()), pos.cuda(), pos_ctx.float().cuda(), s.cuda(), t=t)
    loss.backward()
    return loss


def _compare(model, P, cfg, attrs, batch, masks=None, tol=1e-4, t=T_MODEL):
    s, pos_ctx = _draw(batch[2], batch[1].shape[-1], seed=cfg.d)
    loss = _run(model, batch, pos_ctx, s, t)
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    want = _oracle_loss(Pg, cfg, attrs, batch, pos_ctx, s, t, masks=masks(model) if masks else None)
    want.backward()
    print(f"loss {loss.item():.9g} want {want.item():.9g}")
    assert abs(loss.item() - want.item()) <= tol * max(abs(want.item()), 1.0), (loss.item(), want.item())
    refs = {n: Pg[n].grad if Pg[n].grad is not None else torch.zeros_like(Pg[n]) for n, _ in model.named_parameters()}
    # (floor: fp32 round-off of the model's largest gradient, for tensors whose exact gradient is 0 -- the key biases)
    floor = 1e-6 * max(float(r.abs().max()) for r in refs.values())
    for name, prm in model.named_parameters():
        ref = refs[name]
        got = prm.grad.cpu().double() if prm.grad is not None else torch.zeros_like(ref)
        err = float((got - ref).abs().max())
        print(f"  {name}: err {err:.3g} max|ref| {float(ref.abs().max()):.3g}")
        assert err <= tol * float(ref.abs().max()) + floor, (name, err, float(ref.abs().max()))


@pytest.mark.parametrize("emb,dec,enc,nb,d,H", MODEL_CASES, ids=["-".join(map(str, c)) for c in MODEL_CASES])
def test_model_loss_and_gradients_match_oracle(emb, dec, enc, nb, d, H):
    """Includes the embeddings without a context term (attr, id, mlpid): C = None."""
    cfg, P, attrs, batch, model = _setup(emb, dec, enc, nb, d, H, 12)
    _compare(model, P, cfg, attrs, batch)


def test_model_plain_bce_at_t_zero_matches_oracle():
    cfg, P, attrs, batch, model = _setup("all", "dot", "identity", 2, 90, 3, 12)
    _compare(model, P, cfg, attrs, batch, t=0.0)


def test_model_embedding_without_context_passes_no_context_rows():
    from carca_replication_amd.catalogue_xent import _context_rows

    for emb, has in (("all", True), ("attrctx", True), ("attr", False), ("id", False), ("mlpid", False)):
        _, _, _, batch, model = _setup(emb, "dot", "identity", 1, 64, 2, 12)
        c = _context_rows(model, torch.rand(5, 12, 3, device="cuda"))
        assert (c is not None) == has, emb
        if has:
            assert c.shape == (60, 64) and c.requires_grad


@pytest.mark.parametrize("L,d,H", [pytest.param(80, 64, 2, id="composed-L80"), pytest.param(12, 48, 1, id="unbuilt-d48-H1")])
def test_model_composed_routes_match_oracle(L, d, H):
    cfg, P, attrs, batch, model = _setup("all", "wdot", "learnable", 2, d, H, L, B=3)
    assert ops.use_composed(d, [H] * 2, L)
    _compare(model, P, cfg, attrs, batch)


def test_model_dropout_replays_exported_masks():
    p = 0.3
    cfg, P, attrs, batch, model = _setup("all", "dot", "identity", 2, 90, 3, 12, p=p)
    B, L = batch[0].shape
    model._keep_dropout_masks = True
    torch.manual_seed(7)

    def masks(m):
        raw, sc, d = m._last_dropout_masks, 1.0 / (1.0 - p), cfg.d
        f = lambda x: x.cpu().double() * sc  # noqa: E731
        mk = {"embed": f(raw["embed"]).view(B, L, d)}
        for i, b in enumerate(raw["blocks"]):
            mk[f"attn{i}"] = f(b["m_attn"])
            mk[f"ffn1_{i}"] = f(b["m_ffn1"])[:, :d].reshape(B, L, d)
            mk[f"ffn2_{i}"] = f(b["m_ffn2"])[:, :d].reshape(B, L, d)
        return mk

    _compare(model, P, cfg, attrs, batch, masks=masks, tol=2e-4)


def test_model_deterministic_mode_gives_identical_gradients():
    cfg, P, attrs, batch, model = _setup("all", "dot", "identity", 2, 90, 3, 12)
    s, pos_ctx = _draw(batch[2], 3)
    ops.set_deterministic(True)
    try:
        runs = []
        for _ in range(2):
            loss = _run(model, batch, pos_ctx, s)
            runs.append([loss.detach().clone()] + [p.grad.clone() for p in model.parameters()])
    finally:
        ops.set_deterministic(False)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_model_errors():
    cfg, P, attrs, batch, model = _setup("all", "dot", "identity", 1, 64, 2, 12)
    p_x, p_c, pos = batch
    prof = (p_x.cuda(), None, p_c.float().cuda())
    s, pos_ctx = _draw(pos, 3)
    s, pos_ctx, posd = s.cuda(), pos_ctx.float().cuda(), pos.cuda()
    with pytest.raises(CarcaHipError, match="shape"):
        model.sampled_bce_loss(prof, posd[:, 1:], pos_ctx, s)
    with pytest.raises(CarcaHipError, match="pos_ctx"):
        model.sampled_bce_loss(prof, posd, pos_ctx[:, :, :2], s)
    with pytest.raises(CarcaHipError, match="integer"):
        model.sampled_bce_loss(prof, posd, pos_ctx, s.float())
    for t in (-0.5, 1.5):
        with pytest.raises(ValueError, match="t must lie in"):
            model.sampled_bce_loss(prof, posd, pos_ctx, s, t=t)
    _, _, _, _, m_ca = _setup("all", "ca", "identity", 1, 64, 2, 12)
    with pytest.raises(CarcaHipError, match="CrossAttentionBlock"):
        m_ca.sampled_bce_loss(prof, posd, pos_ctx, s)
    model.embeds.register_attr_table(None)
    with pytest.raises(CarcaHipError, match="register_attr_table"):
        model.sampled_bce_loss(prof, posd, pos_ctx, s)


# ---- engine ----------------------------------------------------------------------------------------------------------
def test_train_step_equals_the_steps_by_hand_and_keeps_the_table_sparse(tmp_path, monkeypatch):
    """train_step(loss="sampled_bce") under a seed = default sampler draw, sampled_bce_loss, backward, mark_rows, step by
    hand: the same parameters, bit for bit.  With the item table a touched-row table (engine.SPARSE_TABLE_BYTES = 0) the
    rows announced are p_x, the positives and the samples, and untouched rows keep their bits."""
    from carca_replication_amd import engine
    from carca_replication_amd.optim import Adam
    from tests.test_hip_catalogue_xent_train import _loaders, _model

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(engine, "SPARSE_TABLE_BYTES", 0)
    monkeypatch.setattr(engine, "SAMPLED_BCE_DEFAULT_K", 8)  # (a few of the 60 items: the table stays sparse)
    train_loader, _, attrs, (n_items, n_ctx, n_attrs) = _loaders(tmp_path)
    batch = [t[:2].cuda() for t in engine.as_batch7(next(iter(train_loader)))]  # (two users)
    torch.manual_seed(1)
    m1 = _model(n_items, n_ctx, n_attrs)
    m2 = _model(n_items, n_ctx, n_attrs)
    m2.load_state_dict(m1.state_dict())
    for m in (m1, m2):
        m.embeds.register_attr_table(torch.as_tensor(attrs, dtype=torch.float32).cuda())
    before = m1.embeds.items_embed.weight.detach().clone()
    o1 = Adam(m1.parameters(), lr=1e-2, weight_decay=0.0)
    o2 = Adam(m2.parameters(), lr=1e-2, weight_decay=0.0)
    p_x, p_a, p_c, o_x, _, o_c = batch[:6]
    half = o_x.shape[1] // 2
    pos, pos_ctx = o_x[:, :half], o_c[:, :half]
    ops.set_deterministic(True)  # (gradients without fp32 atomics: the two models' gradients are the same bits)
    try:
        torch.manual_seed(5)
        engine.train_step(m1, o1, batch, loss="sampled_bce")
        torch.manual_seed(5)
        sampler = engine.default_sampler(m2, p_x.device, engine.SAMPLED_BCE_DEFAULT_K)
        assert sampler.n_samples == 8 and sampler._cdf is None
        samples = sampler.sample()
        o2.zero_grad(set_to_none=True)
        m2.sampled_bce_loss((p_x, p_a, p_c), pos, pos_ctx, samples, t=engine.SAMPLED_BCE_T).backward()
        E2 = m2.embeds.items_embed.weight
        o2.mark_rows(E2, torch.cat([p_x.reshape(-1), pos.reshape(-1), samples.reshape(-1)]))
        o2.step()
    finally:
        ops.set_deterministic(False)
    for (n, a), b in zip(m1.named_parameters(), m2.parameters()):
        assert torch.equal(a, b), n
    E = m1.embeds.items_embed.weight
    mask = o1.state[E]["row_touched"]
    want = torch.zeros(n_items, dtype=torch.uint8, device="cuda")
    want[torch.cat([p_x.reshape(-1), pos.reshape(-1), samples.reshape(-1)]).long()] = 1
    assert torch.equal(mask, want)
    assert int(mask.sum()) < n_items
    untouched = want == 0
    assert torch.equal(E.detach()[untouched], before[untouched])
    assert not torch.equal(E.detach()[want == 1], before[want == 1])
    with pytest.raises(CarcaHipError, match="sharded"):
        engine.train_step(m1, o1, batch, sharded=True, loss="sampled_bce")


def test_train_runs_an_epoch_and_refuses_graph_capture(tmp_path, monkeypatch):
    from carca_replication_amd.optim import Adam
    from carca_replication_amd.train import train
    from tests.test_hip_catalogue_xent_train import _loaders, _model

    monkeypatch.chdir(tmp_path)
    random.seed(0)
    torch.manual_seed(0)
    train_loader, val_loader, attrs, (n_items, n_ctx, n_attrs) = _loaders(tmp_path)
    model = _model(n_items, n_ctx, n_attrs, p=0.2)
    model.embeds.register_attr_table(torch.as_tensor(attrs, dtype=torch.float32).cuda())
    optim = Adam(model.parameters(), lr=1e-3, weight_decay=0.0, betas=(0.9, 0.98))
    train(model=model, train_loader=train_loader, val_loader=val_loader, test_loader=None, device="cuda", optim=optim,
          epochs=1, early_stop=20, datadir="run", verbose=1, loss="sampled_bce")
    logs = [f for f in os.listdir("run") if f.endswith(".csv")]
    rows = [ln.strip().split(";") for ln in open(os.path.join("run", logs[0]))]
    losses = [float(r[3]) for r in rows if r[2] == "train"]
    assert len(losses) == 1 and math.isfinite(losses[0]) and losses[0] > 0
    with pytest.raises(CarcaHipError, match="graphed"):
        train(model=model, train_loader=train_loader, val_loader=val_loader, test_loader=None, device="cuda",
              optim=optim, epochs=1, datadir="run2", verbose=0, graphed=True, loss="sampled_bce")
