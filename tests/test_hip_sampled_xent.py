"""Sampled softmax cross-entropy with the logQ correction (ops.sampled_xent, CARCA.sampled_softmax_loss; DESIGN.md
section 14) on the GPU: the op against fp64 torch, its identity with the full-catalogue softmax of section 13, run-to-run
bits and memory; the model's loss and every parameter gradient against torch.autograd over the oracle."""
import math

import pytest
import torch

from carca_replication_amd import CarcaHipError, ops
from oracle import carca_oracle as O
from tests.model_util import build_model
from tests.test_hip_catalogue_xent import G, MODEL_CASES, N_ATTRS, _setup

pytestmark = pytest.mark.gpu


def _ref_loss(P, Tp, pos, S, s_ids, log_q):
    """fp64 sampled softmax: per valid row, logsumexp over the positive and the samples that are classes and not the
    positive, every logit corrected by -log(K Q); 0 without a valid row."""
    n, K = log_q.numel(), s_ids.numel()
    pos, s = pos.long().to(P.device), s_ids.long().to(P.device)
    valid = (pos >= 1) & (pos < n)
    if not bool(valid.any()):
        return (P.sum() + Tp.sum() + S.sum()) * 0.0
    lq = log_q.double().to(P.device)
    s_ok = (s >= 1) & (s < n)
    bs = torch.where(s_ok, -(lq[torch.where(s_ok, s, 0)] + math.log(K)), torch.zeros((), dtype=P.dtype, device=P.device))
    pv = pos[valid]
    Pv = P[valid]
    zp = (Pv * Tp[valid]).sum(1) - (lq[pv] + math.log(K))
    zs = (Pv @ S.T + bs).masked_fill(~(s_ok.view(1, -1) & (s.view(1, -1) != pv.view(-1, 1))), -float("inf"))
    lse = torch.logsumexp(torch.cat([zp.view(-1, 1), zs], 1), 1)
    return (lse - zp).mean()


def _operands(R, K, d, n_items, seed):
    g = torch.Generator().manual_seed(seed)
    P = torch.randn(R, d, generator=g, dtype=torch.float64)
    Tp = torch.randn(R, d, generator=g, dtype=torch.float64) / d ** 0.5
    S = torch.randn(K, d, generator=g, dtype=torch.float64) / d ** 0.5
    pos = torch.randint(1, n_items, (R,), generator=g)
    bad = torch.rand(R, generator=g) < 0.2  # padding rows: pos 0, negative or past the catalogue
    pos[bad] = torch.tensor([0, -3, n_items, n_items + 7])[torch.randint(0, 4, (int(bad.sum()),), generator=g)]
    s = torch.randint(1, n_items, (K,), generator=g)  # with replacement: duplicates
    if K > 2:
        s[: K // 3] = pos[torch.randint(0, R, (K // 3,), generator=g)]  # accidental hits (and some invalid ids)
        s[K - 1] = 0
    bad_s = torch.rand(K, generator=g) < 0.1
    s[bad_s] = torch.tensor([0, -1, n_items, n_items + 3])[torch.randint(0, 4, (int(bad_s.sum()),), generator=g)]
    counts = torch.randint(0, 50, (n_items,), generator=g).double()
    w = (counts[1:] + 1) ** 0.7
    log_q = torch.cat([torch.tensor([-float("inf")], dtype=torch.float64), torch.log(w / w.sum())]).float()
    return P, Tp, S, pos, s, log_q


def _check_op(R, K, d, n_items=5000, seed=0):
    P64, T64, S64, pos, s, log_q = _operands(R, K, d, n_items, seed)
    Pr, Tr, Sr = (x.cuda().requires_grad_(True) for x in (P64, T64, S64))
    want = _ref_loss(Pr, Tr, pos, Sr, s, log_q)
    want.backward()
    P, Tp, S = (x.float().cuda().requires_grad_(True) for x in (P64, T64, S64))
    got = ops.sampled_xent(P, Tp, pos.cuda(), S, s.cuda(), log_q.cuda())
    got.backward()
    w = want.item()
    assert abs(got.item() - w) <= 1e-5 * max(abs(w), 0.1), (got.item(), w)
    for name, g, r in (("P", P.grad, Pr.grad), ("Tp", Tp.grad, Tr.grad), ("S", S.grad, Sr.grad)):
        assert g.shape == r.shape, name
        err = float((g.double() - r).abs().max())
        assert err <= 1e-4 * float(r.abs().max()) + 1e-9, (name, err, float(r.abs().max()))


OP_CASES = [(1, 1, 64), (17, 63, 90), (17, 64, 128), (3400, 65, 192), (6400, 1000, 256), (3400, 8192, 90),
            (1, 8192, 128), (6400, 64, 64), (17, 1000, 256), (3400, 1, 128), (6400, 8192, 64), (1, 65, 192),
            (17, 8192, 256), (3400, 1000, 64), (6400, 63, 192)]


@pytest.mark.parametrize("R,K,d", OP_CASES)
def test_op_matches_fp64_reference(R, K, d):
    _check_op(R, K, d, seed=R + K + d)


def test_op_small_catalogue_every_sample_a_hit_or_invalid():
    """n_items = 3: most samples are the row's own positive or no class at all; rows whose every sample is masked
    reduce to loss 0 with the positive alone."""
    _check_op(300, 70, 90, n_items=3, seed=11)


def test_op_no_valid_row_gives_zero_loss_and_gradients():
    P = torch.randn(5, 90, device="cuda", requires_grad=True)
    Tp = torch.randn(5, 90, device="cuda", requires_grad=True)
    S = torch.randn(33, 90, device="cuda", requires_grad=True)
    log_q = torch.full((40,), -math.log(39.0), device="cuda")
    loss = ops.sampled_xent(P, Tp, torch.tensor([0, 0, -1, 40, 0], device="cuda"), S,
                            torch.randint(1, 40, (33,), device="cuda"), log_q)
    loss.backward()
    assert loss.item() == 0.0
    for g in (P.grad, Tp.grad, S.grad):
        assert float(g.abs().max()) == 0.0


def test_op_every_sample_equals_catalogue_xent():
    """samples = arange(1, n_items), uniform Q: the sampled loss is section 13's full softmax, gradients included (dT of
    the catalogue = the scatter of dS and dTp)."""
    n_items, d, R = 12102, 90, 3400
    g = torch.Generator().manual_seed(3)
    P64 = torch.randn(R, d, generator=g, dtype=torch.float64)
    T64 = torch.randn(n_items, d, generator=g, dtype=torch.float64) / d ** 0.5
    pos = torch.randint(1, n_items, (R,), generator=g)
    pos[torch.rand(R, generator=g) < 0.2] = 0
    pos = pos.cuda()
    P1, T1 = P64.float().cuda().requires_grad_(True), T64.float().cuda().requires_grad_(True)
    full = ops.catalogue_xent(P1, T1, pos)
    full.backward()
    P2, T2 = P64.float().cuda().requires_grad_(True), T64.float().cuda().requires_grad_(True)
    s = torch.arange(1, n_items, device="cuda")
    log_q = torch.full((n_items,), -math.log(n_items - 1), device="cuda")
    log_q[0] = -float("inf")
    samp = ops.sampled_xent(P2, T2[pos.clamp(0, n_items - 1)], pos, T2[s], s, log_q)
    samp.backward()
    assert abs(samp.item() - full.item()) <= 1e-5 * abs(full.item()), (samp.item(), full.item())
    for a, b in ((P2.grad, P1.grad), (T2.grad, T1.grad)):
        err = float((a - b).abs().max())
        assert err <= 1e-4 * float(b.abs().max()), (err, float(b.abs().max()))


def test_op_two_calls_are_bit_identical():
    P64, T64, S64, pos, s, log_q = _operands(3400, 8192, 90, 5000, seed=5)
    outs = []
    for _ in range(2):
        P, Tp, S = (x.float().cuda().requires_grad_(True) for x in (P64, T64, S64))
        loss = ops.sampled_xent(P, Tp, pos.cuda(), S, s.cuda(), log_q.cuda())
        loss.backward()
        outs.append((loss.detach().clone(), P.grad.clone(), Tp.grad.clone(), S.grad.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_op_needs_no_logit_buffer():
    """R = 6,400, K = 65,536, d = 128: one [R, K] fp32 buffer is 1.68 GB; the op's memory beyond its inputs and the
    gradients it returns stays under a tenth of that."""
    R, K, d, n_items = 6400, 65536, 128, 1_000_001
    g = torch.Generator(device="cuda").manual_seed(0)
    P = torch.randn(R, d, device="cuda", generator=g).requires_grad_(True)
    Tp = (torch.randn(R, d, device="cuda", generator=g) / d ** 0.5).requires_grad_(True)
    S = (torch.randn(K, d, device="cuda", generator=g) / d ** 0.5).requires_grad_(True)
    pos = torch.randint(0, n_items, (R,), device="cuda", generator=g)
    s = torch.randint(1, n_items, (K,), device="cuda", generator=g)
    log_q = torch.full((n_items,), -math.log(n_items - 1), device="cuda")
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss = ops.sampled_xent(P, Tp, pos, S, s, log_q)
    loss.backward()
    torch.cuda.synchronize()
    outputs = (P.grad.numel() + Tp.grad.numel() + S.grad.numel()) * 4
    extra = torch.cuda.max_memory_allocated() - base - outputs
    assert extra < 0.1 * R * K * 4, extra / 2 ** 20
    assert math.isfinite(loss.item()) and loss.item() > 0


# ---- model level ---------------------------------------------------------------------------------------------------
N_ITEMS, K_MODEL = 300, 200


def _draw(n_items=N_ITEMS, K=K_MODEL, seed=0, pos=None):
    """K sample ids with duplicates, accidental hits of the batch's positives and invalid ids; a non-uniform log Q."""
    g = torch.Generator().manual_seed(seed + 100)
    s = torch.randint(1, n_items, (K,), generator=g)
    if pos is not None:
        flat = pos.reshape(-1)
        s[:10] = flat[torch.randint(0, flat.numel(), (10,), generator=g)]
    s[10:13] = torch.tensor([0, -2, n_items + 1])
    w = torch.rand(n_items - 1, generator=g, dtype=torch.float64) + 0.1
    log_q = torch.cat([torch.tensor([-float("inf")], dtype=torch.float64), torch.log(w / w.sum())]).float()
    return s, log_q


def _oracle_loss(Pg, cfg, attrs, batch, n_items, s, log_q, masks=None):
    p_x, p_c, pos = batch
    B, L = p_x.shape
    trace = {}
    O.carca_forward(Pg, cfg, (p_x, attrs[p_x], p_c), [(pos, attrs[pos], p_c)], training=True, trace=trace, masks=masks)
    p = trace["p_final"]
    if cfg.decoder == "wdot":  # p[t] * sum_{j<=t} gamma^j, the reference's float32 slot weights (carca.py:376,385-386)
        w = torch.tril((cfg.gamma ** torch.arange(0, L)).unsqueeze(0).expand(L, L)).to(p.dtype).sum(1)
        p = p * w.view(1, L, 1)
    fix = lambda t: torch.where((t >= 1) & (t < n_items), t, torch.zeros_like(t))  # noqa: E731
    ids = fix(s).view(1, -1)
    S = O.embedding(Pg, cfg, ids, attrs[ids], torch.zeros(1, ids.shape[1], p_c.shape[-1], dtype=torch.float64),
                    O.get_mask(ids, torch.float64), target=True)[0]
    tp = fix(pos)
    Tp = O.embedding(Pg, cfg, tp, attrs[tp], torch.zeros(B, L, p_c.shape[-1], dtype=torch.float64),
                     O.get_mask(tp, torch.float64), target=True)
    return _ref_loss(p.reshape(B * L, -1), Tp.reshape(B * L, -1), pos.reshape(-1), S, s, log_q)


def _run(model, batch, s, log_q):
    p_x, p_c, pos = batch
    model.zero_grad(set_to_none=True)
    a = None if hasattr(model.embeds, "register_attr_table") else torch.zeros(*p_x.shape, N_ATTRS, device="cuda")
    loss = model.sampled_softmax_loss((p_x.cuda(), a, p_c.float().cuda()), pos.cuda(), s.cuda(), log_q.cuda())
    loss.backward()
    return loss


def _compare(model, P, cfg, attrs, batch, masks=None, tol=1e-4):
    s, log_q = _draw(seed=cfg.d, pos=batch[2])
    loss = _run(model, batch, s, log_q)
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    want = _oracle_loss(Pg, cfg, attrs, batch, N_ITEMS, s, log_q, masks=masks(model) if masks else None)
    want.backward()
    assert abs(loss.item() - want.item()) <= tol * max(abs(want.item()), 1.0), (loss.item(), want.item())
    refs = {n: Pg[n].grad if Pg[n].grad is not None else torch.zeros_like(Pg[n]) for n, _ in model.named_parameters()}
    # (floor: fp32 round-off of the model's largest gradient, for tensors whose exact gradient is 0 -- the key biases)
    floor = 1e-6 * max(float(r.abs().max()) for r in refs.values())
    for name, prm in model.named_parameters():
        ref = refs[name]
        got = prm.grad.cpu().double() if prm.grad is not None else torch.zeros_like(ref)
        err = float((got - ref).abs().max())
        assert err <= tol * float(ref.abs().max()) + floor, (name, err, float(ref.abs().max()))


@pytest.mark.parametrize("emb,dec,enc,nb,d,H", MODEL_CASES, ids=["-".join(map(str, c)) for c in MODEL_CASES])
def test_model_loss_and_gradients_match_oracle(emb, dec, enc, nb, d, H):
    cfg, P, attrs, batch, model = _setup(emb, dec, enc, nb, d, H, 12)
    _compare(model, P, cfg, attrs, batch)


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
        f = lambda t: t.cpu().double() * sc  # noqa: E731
        mk = {"embed": f(raw["embed"]).view(B, L, d)}
        for i, b in enumerate(raw["blocks"]):
            mk[f"attn{i}"] = f(b["m_attn"])
            mk[f"ffn1_{i}"] = f(b["m_ffn1"])[:, :d].reshape(B, L, d)
            mk[f"ffn2_{i}"] = f(b["m_ffn2"])[:, :d].reshape(B, L, d)
        return mk

    _compare(model, P, cfg, attrs, batch, masks=masks, tol=2e-4)


@pytest.mark.parametrize("emb,dec", [("all", "dot"), ("attr", "wdot"), ("mlpid", "dot")])
def test_model_every_sample_equals_catalogue_softmax_loss(emb, dec):
    """samples = arange(1, n_items) with uniform Q: the loss and every parameter gradient of catalogue_softmax_loss."""
    cfg, P, attrs, batch, model = _setup(emb, dec, "learnable", 2, 64, 2, 12)
    p_x, p_c, pos = batch
    a = None if hasattr(model.embeds, "register_attr_table") else torch.zeros(*p_x.shape, N_ATTRS, device="cuda")
    prof = (p_x.cuda(), a, p_c.float().cuda())
    model.zero_grad(set_to_none=True)
    full = model.catalogue_softmax_loss(prof, pos.cuda())
    full.backward()
    want = {n: q.grad.clone() for n, q in model.named_parameters()}
    s = torch.arange(1, N_ITEMS, device="cuda")
    log_q = torch.full((N_ITEMS,), -math.log(N_ITEMS - 1), device="cuda")
    log_q[0] = -float("inf")
    model.zero_grad(set_to_none=True)
    samp = model.sampled_softmax_loss(prof, pos.cuda(), s, log_q)
    samp.backward()
    assert abs(samp.item() - full.item()) <= 1e-5 * abs(full.item()), (samp.item(), full.item())
    floor = 1e-6 * max(float(g.abs().max()) for g in want.values())
    for n, q in model.named_parameters():
        err = float((q.grad - want[n]).abs().max())
        assert err <= 1e-4 * float(want[n].abs().max()) + floor, (n, err, float(want[n].abs().max()))


def test_model_deterministic_mode_gives_identical_gradients():
    cfg, P, attrs, batch, model = _setup("all", "dot", "identity", 2, 90, 3, 12)
    s, log_q = _draw(pos=batch[2])
    ops.set_deterministic(True)
    try:
        runs = []
        for _ in range(2):
            loss = _run(model, batch, s, log_q)
            runs.append([loss.detach().clone()] + [p.grad.clone() for p in model.parameters()])
    finally:
        ops.set_deterministic(False)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_model_errors():
    cfg, P, attrs, batch, model = _setup("all", "dot", "identity", 1, 64, 2, 12)
    p_x, p_c, pos = batch
    prof = (p_x.cuda(), None, p_c.float().cuda())
    s, log_q = _draw()
    s, log_q = s.cuda(), log_q.cuda()
    with pytest.raises(CarcaHipError, match="shape"):
        model.sampled_softmax_loss(prof, pos[:, 1:].cuda(), s, log_q)
    with pytest.raises(CarcaHipError, match="log_q"):
        model.sampled_softmax_loss(prof, pos.cuda(), s, log_q[1:])
    with pytest.raises(CarcaHipError, match="integer"):
        model.sampled_softmax_loss(prof, pos.cuda(), s.float(), log_q)
    _, _, _, _, m_ca = _setup("all", "ca", "identity", 1, 64, 2, 12)
    with pytest.raises(CarcaHipError, match="CrossAttentionBlock"):
        m_ca.sampled_softmax_loss(prof, pos.cuda(), s, log_q)
    cfgn = dict(d=64, H=2, n_blocks=1, encoding="identity", embedding="all", decoder="wdot", l2_norm=True)
    m_n = build_model(cfgn, N_ITEMS, G, 3, N_ATTRS, 12).cuda().train()
    m_n.embeds.register_attr_table(attrs.float().cuda())
    with pytest.raises(CarcaHipError, match="normalize=True"):
        m_n.sampled_softmax_loss(prof, pos.cuda(), s, log_q)
    model.embeds.register_attr_table(None)
    with pytest.raises(CarcaHipError, match="register_attr_table"):
        model.sampled_softmax_loss(prof, pos.cuda(), s, log_q)
