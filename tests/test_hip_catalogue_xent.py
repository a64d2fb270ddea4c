"""Full-catalogue softmax cross-entropy (ops.catalogue_xent, CARCA.catalogue_softmax_loss) on the
GPU against fp64 torch: the op against F.cross_entropy, the model's loss and every parameter gradient against
torch.autograd over the oracle."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from carca_replication_amd import CarcaHipError, ops
from oracle import carca_oracle as O
from tests.model_util import build_model

pytestmark = pytest.mark.gpu


def _ref_loss(P, T, pos):
    """fp64 F.cross_entropy over classes 1 .. n_items-1 of the valid rows; 0 without one."""
    n = T.shape[0]
    pos = pos.long()
    valid = (pos >= 1) & (pos < n)
    if not bool(valid.any()):
        return (P.sum() + T.sum()) * 0.0
    logits = P[valid] @ T[1:].T
    return F.cross_entropy(logits, pos[valid] - 1)


def _operands(R, n_items, d, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    P = torch.randn(R, d, generator=g, dtype=torch.float64) * scale
    T = torch.randn(n_items, d, generator=g, dtype=torch.float64) * scale / d ** 0.5
    pos = torch.randint(1, max(n_items, 2), (R,), generator=g)
    bad = torch.rand(R, generator=g) < 0.2  # padding rows: pos 0, negative or past the catalogue
    pos[bad] = torch.tensor([0, -3, n_items, n_items + 7])[torch.randint(0, 4, (int(bad.sum()),), generator=g)]
    return P, T, pos


def _check_op(R, n_items, d, seed=0):
    P64, T64, pos = _operands(R, n_items, d, seed)
    Pr, Tr = P64.clone().requires_grad_(True), T64.clone().requires_grad_(True)
    want = _ref_loss(Pr, Tr, pos)
    want.backward()
    P = P64.float().cuda().requires_grad_(True)
    T = T64.float().cuda().requires_grad_(True)
    got = ops.catalogue_xent(P, T, pos.cuda())
    got.backward()
    w = want.item()
    # (relative, with a floor for the one-class catalogue, whose loss is 0 up to the fp32 rounding of lse - z_pos)
    assert abs(got.item() - w) <= 1e-5 * max(abs(w), 0.1), (got.item(), w)
    for g, r in ((P.grad, Pr.grad), (T.grad, Tr.grad)):
        assert g.shape == r.shape
        err = float((g.double().cpu() - r).abs().max())
        assert err <= 1e-4 * float(r.abs().max()) + 1e-9, (err, float(r.abs().max()))
    return P, T, pos


@pytest.mark.parametrize("R,n_items,d", [(1, 2, 64), (17, 3, 90), (300, 257, 128), (17, 4097, 192), (3400, 12102, 90),
                                         (300, 12102, 64), (1, 257, 90), (3400, 2, 128), (300, 4097, 90)])
def test_op_matches_fp64_cross_entropy(R, n_items, d):
    _check_op(R, n_items, d, seed=R + n_items + d)


def test_op_no_valid_row_gives_zero_loss_and_gradients():
    P = torch.randn(5, 90, device="cuda", requires_grad=True)
    T = torch.randn(40, 90, device="cuda", requires_grad=True)
    loss = ops.catalogue_xent(P, T, torch.tensor([0, 0, -1, 40, 0], device="cuda"))
    loss.backward()
    assert loss.item() == 0.0
    assert float(P.grad.abs().max()) == 0.0 and float(T.grad.abs().max()) == 0.0


def test_op_two_calls_are_bit_identical():
    P64, T64, pos = _operands(3400, 12102, 90, seed=5)
    outs = []
    for _ in range(2):
        P = P64.float().cuda().requires_grad_(True)
        T = T64.float().cuda().requires_grad_(True)
        loss = ops.catalogue_xent(P, T, pos.cuda())
        loss.backward()
        outs.append((loss.detach().clone(), P.grad.clone(), T.grad.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_op_c4_catalogue_needs_no_logit_buffer():
    """n_items = 1,000,001, d = 128, R = 4096: the logits alone would be 16 GB; the op's memory beyond its inputs and
    outputs stays under 512 MB, and the loss is right (checked against a chunked fp64 reference)."""
    n_items, d, R = 1_000_001, 128, 4096
    g = torch.Generator(device="cuda").manual_seed(0)
    T = (torch.randn(n_items, d, device="cuda", generator=g) / d ** 0.5).requires_grad_(True)
    P = torch.randn(R, d, device="cuda", generator=g).requires_grad_(True)
    pos = torch.randint(0, n_items, (R,), device="cuda", generator=g)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss = ops.catalogue_xent(P, T, pos)
    loss.backward()
    torch.cuda.synchronize()
    outputs = T.grad.numel() * 4 + P.grad.numel() * 4
    extra = torch.cuda.max_memory_allocated() - base - outputs
    assert extra < 512 * 2 ** 20, extra / 2 ** 20
    # fp64 reference of the loss over 64 rows, item range in chunks
    rows = torch.arange(0, R, 64, device="cuda")
    Pd, Td = P.detach()[rows].double(), T.detach().double()
    lse = torch.full((rows.numel(),), -float("inf"), dtype=torch.float64, device="cuda")
    for i0 in range(1, n_items, 1 << 17):
        lse = torch.logaddexp(lse, torch.logsumexp(Pd @ Td[i0: i0 + (1 << 17)].T, dim=1))
    p = pos[rows]
    valid = p >= 1
    want = (lse - (Pd * Td[p]).sum(1))[valid]
    _, lse_got = ops.catalogue_xent_fwd(P.detach(), T.detach(), ops._ids32(pos), d)
    got = lse_got[rows][valid].double() - (Pd * Td[p]).sum(1)[valid]
    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())


# ---- model level ---------------------------------------------------------------------------------------------------
G, N_ATTRS = 24, 12


def _setup(emb, dec, enc, nb, d, H, L, B=5, n_items=300, n_ctx=3, p=0.0, seed=0):
    cfg = O.CarcaConfig(d=d, H=H, n_blocks=nb, encoding=enc, embedding=emb, decoder=dec)
    P = O.perturb_params(O.init_params(cfg, n_items, G, n_ctx, N_ATTRS, L, seed=seed, dtype=torch.float64), seed=seed + 1)
    rng = np.random.default_rng(seed + 7)
    attrs = torch.from_numpy(rng.random((n_items, N_ATTRS))).double()
    attrs[0] = 0
    p_x = torch.zeros(B, L, dtype=torch.int64)
    pos = torch.zeros(B, L, dtype=torch.int64)
    for b in range(B):
        ell = 0 if b == 1 else int(rng.integers(1, L + 1))
        if ell:
            p_x[b, L - ell:] = torch.from_numpy(rng.integers(1, n_items, size=ell))
            pos[b, L - ell:] = torch.from_numpy(rng.integers(1, n_items, size=ell))
    p_c = torch.from_numpy(rng.random((B, L, n_ctx))).double() * (p_x != 0).unsqueeze(-1)
    model = build_model(dict(d=d, H=H, n_blocks=nb, encoding=enc, embedding=emb, decoder=dec), n_items, G, n_ctx,
                        N_ATTRS, L, p=p)
    model.load_state_dict({k: v.float() for k, v in P.items()}, strict=True)
    model = model.cuda().train()
    if hasattr(model.embeds, "register_attr_table"):
        model.embeds.register_attr_table(attrs.float().cuda())
    return cfg, P, attrs, (p_x, p_c, pos), model


def _oracle_loss(Pg, cfg, attrs, batch, n_items, masks=None):
    p_x, p_c, pos = batch
    B, L = p_x.shape
    trace = {}
    O.carca_forward(Pg, cfg, (p_x, attrs[p_x], p_c), [(pos, attrs[pos], p_c)], training=True, trace=trace, masks=masks)
    p = trace["p_final"]
    if cfg.decoder == "wdot":  # p[t] * sum_{j<=t} gamma^j, the reference's float32 slot weights (carca.py:376,385-386)
        w = torch.tril((cfg.gamma ** torch.arange(0, L)).unsqueeze(0).expand(L, L)).to(p.dtype).sum(1)
        p = p * w.view(1, L, 1)
    ids = torch.arange(n_items).view(1, -1)
    zero = torch.zeros(1, n_items, p_c.shape[-1], dtype=torch.float64)
    T = O.embedding(Pg, cfg, ids, attrs[ids], zero, O.get_mask(ids, torch.float64), target=True)[0]
    return _ref_loss(p.reshape(B * L, -1), T, pos.reshape(-1))


def _run(model, batch):
    p_x, p_c, pos = batch
    model.zero_grad(set_to_none=True)
    a = None if hasattr(model.embeds, "register_attr_table") else torch.zeros(*p_x.shape, N_ATTRS, device="cuda")
    loss = model.catalogue_softmax_loss((p_x.cuda(), a, p_c.float().cuda()), pos.cuda())
    loss.backward()
    return loss


def _compare(model, P, cfg, attrs, batch, n_items, masks=None, tol=1e-4):
    loss = _run(model, batch)
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    want = _oracle_loss(Pg, cfg, attrs, batch, n_items, masks=masks(model) if masks else None)
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


MODEL_CASES = [
    ("all", "dot", "identity", 2, 90, 3), ("all", "wdot", "learnable", 1, 64, 2),
    ("attrctx", "dot", "positional", 1, 64, 4), ("attrctx", "wdot", "identity", 2, 90, 3),
    ("attr", "dot", "learnable", 0, 90, 3), ("attr", "wdot", "positional", 2, 64, 2),
    ("id", "dot", "identity", 1, 64, 1), ("id", "wdot", "learnable", 2, 90, 3),
    ("mlpid", "dot", "positional", 2, 90, 3), ("mlpid", "wdot", "identity", 0, 64, 2),
]


@pytest.mark.parametrize("emb,dec,enc,nb,d,H", MODEL_CASES, ids=["-".join(map(str, c)) for c in MODEL_CASES])
def test_model_loss_and_gradients_match_oracle(emb, dec, enc, nb, d, H):
    L = 12
    cfg, P, attrs, batch, model = _setup(emb, dec, enc, nb, d, H, L)
    _compare(model, P, cfg, attrs, batch, 300)


@pytest.mark.parametrize("L,d,H", [pytest.param(80, 64, 2, id="composed-L80"), pytest.param(12, 48, 1, id="unbuilt-d48-H1")])
def test_model_composed_routes_match_oracle(L, d, H):
    cfg, P, attrs, batch, model = _setup("all", "wdot", "learnable", 2, d, H, L, B=3)
    assert ops.use_composed(d, [H] * 2, L)
    _compare(model, P, cfg, attrs, batch, 300)


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

    _compare(model, P, cfg, attrs, batch, 300, masks=masks, tol=2e-4)


def test_model_deterministic_mode_gives_identical_gradients():
    cfg, P, attrs, batch, model = _setup("all", "dot", "identity", 2, 90, 3, 12)
    ops.set_deterministic(True)
    try:
        runs = []
        for _ in range(2):
            loss = _run(model, batch)
            runs.append([loss.detach().clone()] + [p.grad.clone() for p in model.parameters()])
    finally:
        ops.set_deterministic(False)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_model_errors():
    cfg, P, attrs, batch, model = _setup("all", "dot", "identity", 1, 64, 2, 12)
    p_x, p_c, pos = batch
    prof = (p_x.cuda(), None, p_c.float().cuda())
    with pytest.raises(CarcaHipError, match="shape"):
        model.catalogue_softmax_loss(prof, pos[:, 1:].cuda())
    _, _, _, _, m_ca = _setup("all", "ca", "identity", 1, 64, 2, 12)
    with pytest.raises(CarcaHipError, match="CrossAttentionBlock"):
        m_ca.catalogue_softmax_loss(prof, pos.cuda())
    cfgn = dict(d=64, H=2, n_blocks=1, encoding="identity", embedding="all", decoder="wdot", l2_norm=True)
    m_n = build_model(cfgn, 300, G, 3, N_ATTRS, 12).cuda().train()
    m_n.embeds.register_attr_table(attrs.float().cuda())
    with pytest.raises(CarcaHipError, match="normalize=True"):
        m_n.catalogue_softmax_loss(prof, pos.cuda())
    model.embeds.register_attr_table(None)
    with pytest.raises(CarcaHipError, match="register_attr_table"):
        model.catalogue_softmax_loss(prof, pos.cuda())
