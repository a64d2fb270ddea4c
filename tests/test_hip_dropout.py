"""Training-mode dropout (p > 0).  torch's Philox stream cannot be reproduced inside a kernel, so parity is
checked the way SURVEY.md section 7.5 asks: (1) the kernels export their keep-masks, the CPU oracle replays the
reference arithmetic with exactly those masks, outputs and every parameter gradient must agree; (2) keep-rates
are statistically right; (3) the same seed gives the same masks, a different seed different ones."""
import pytest
import torch

from oracle import carca_oracle as O
from tests.model_util import dev, model_from_params

pytestmark = pytest.mark.gpu


def _setup(p, d=90, H=3, nb=2, B=6, L=50, n_items=300, n_attrs=40, n_ctx=4, g=120):
    cfg = O.CarcaConfig(d=d, H=H, n_blocks=nb)
    P = O.perturb_params(O.init_params(cfg, n_items, g, n_ctx, n_attrs, L, seed=0), seed=1)
    profile, pos, _ = O.synth_eval_batch(B, L, L, n_items, n_attrs, n_ctx, seed=3, min_len=2)
    neg = (pos[0].flip(1).contiguous(), pos[1].flip(1).contiguous(), pos[2])
    px = profile[0]
    pos = (pos[0] * (px != 0), pos[1], pos[2])
    neg = (neg[0] * (px != 0), neg[1], neg[2])
    y_true = torch.cat([(px != 0).int(), torch.zeros_like(px)], dim=1)
    o_x = torch.cat([pos[0], neg[0]], dim=1)
    model = model_from_params(P, cfg)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = p
    return cfg, P, profile, pos, neg, y_true, o_x, model


def _oracle_masks(model, cfg, p, B, L, Ns):
    raw = model._last_dropout_masks
    d, sc = cfg.d, 1.0 / (1.0 - p)
    f = lambda t: t.cpu().float() * sc  # noqa: E731
    mk = {"embed": f(raw["embed"]).view(B, L, d)}
    for i, b in enumerate(raw["blocks"]):
        mk[f"attn{i}"] = f(b["m_attn"])
        mk[f"ffn1_{i}"] = f(b["m_ffn1"])[:, :d].reshape(B, L, d)
        mk[f"ffn2_{i}"] = f(b["m_ffn2"])[:, :d].reshape(B, L, d)
    for gi, m in enumerate(raw["cross"]):
        mk[f"cross{gi}"] = f(m)
    return mk


@pytest.mark.parametrize("p,d,H", [pytest.param(0.3, 90, 3, id="0.3"), pytest.param(0.5, 90, 3, id="0.5"),
                                   pytest.param(0.3, 128, 1, id="0.3-d128-H1"), pytest.param(0.5, 64, 4, id="0.5-d64-H4")])
def test_dropout_forward_backward_match_oracle_with_same_masks(p, d, H):
    from carca_replication_amd import modules as M

    cfg, P, profile, pos, neg, y_true, o_x, model = _setup(p, d=d, H=H)
    B, L = profile[0].shape
    model.train()
    model._keep_dropout_masks = True
    torch.manual_seed(7)
    y = model(profile=dev(profile), targets=[dev(pos), dev(neg)])
    loss = M.BinaryCrossEntropy()(y, y_true.cuda(), M.get_mask(o_x.cuda()))
    loss.backward()
    mk = _oracle_masks(model, cfg, p, B, L, [L, L])
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    yo = O.carca_forward(Pg, cfg, profile, [pos, neg], training=True, masks=mk)
    lo = O.bce_loss(yo, y_true, O.get_mask(o_x))
    lo.backward()
    assert float((y.detach().cpu() - yo.detach()).abs().max()) < 5e-5
    assert abs(float(loss) - float(lo)) < 1e-5
    for name, prm in model.named_parameters():
        ref = Pg[name].grad if Pg[name].grad is not None else torch.zeros_like(Pg[name])
        err = float((prm.grad.cpu() - ref).abs().max())
        assert err <= 2e-4 * float(ref.abs().max()) + 1e-7, (name, err, float(ref.abs().max()))


def test_dropout_keep_rates_and_seeding():
    p = 0.5
    cfg, P, profile, pos, neg, y_true, o_x, model = _setup(p, B=16)
    model.train()
    model._keep_dropout_masks = True

    def run(seed):
        torch.manual_seed(seed)
        with torch.enable_grad():
            model(profile=dev(profile), targets=[dev(pos), dev(neg)])
        raw = model._last_dropout_masks
        return [raw["embed"].clone()] + [b["m_ffn1"][:, :cfg.d].clone() for b in raw["blocks"]] + \
               [b["m_ffn2"][:, :cfg.d].clone() for b in raw["blocks"]] + [b["m_attn"].clone() for b in raw["blocks"]]

    a, b, c = run(11), run(11), run(12)
    for x, y_ in zip(a, b):
        assert torch.equal(x, y_)
    assert any(not torch.equal(x, z) for x, z in zip(a, c))
    for m in a[:5]:  # elementwise sites: every entry is a fair coin at p = 0.5
        n = m.numel()
        rate = float(m.float().mean())
        assert abs(rate - (1 - p)) < 5 * (p * (1 - p) / n) ** 0.5 + 1e-3, rate
    # sites must not share a stream
    assert not torch.equal(a[1], a[3])


def test_eval_mode_ignores_dropout():
    cfg, P, profile, pos, neg, y_true, o_x, model = _setup(0.5)
    model.eval()
    with torch.no_grad():
        y1 = model(profile=dev(profile), targets=[dev(pos)])
        y2 = model(profile=dev(profile), targets=[dev(pos)])
    want = O.carca_forward(P, cfg, profile, [pos], training=False)
    assert torch.equal(y1, y2)
    assert float((y1.cpu() - want).abs().max()) < 2e-5


@pytest.mark.parametrize("causal", [None, 0, -1])
def test_standalone_mha_train_mode_dropout_replays_in_the_oracle(causal):
    """MultiHeadAttention.forward on its own in TRAIN mode with p > 0 (carca.py:258: self.dropout on the weights; VERDICT r4
    item 7b): carca_mha_core_drop draws the masks, the module keeps the keep-mask, and the oracle replays the reference
    arithmetic with exactly that mask -- output, the returned PRE-dropout weights (carca.py:262-263) and every gradient."""
    from carca_replication_amd import modules as M

    torch.manual_seed(0)
    B, Tq, Tk, d, H, p = 5, 23, 37, 90, 3, 0.4
    mha = M.MultiHeadAttention(d, H, p).cuda().train()
    q = torch.randn(B, Tq, d, device="cuda", requires_grad=True)
    kv = torch.randn(B, Tk, d, device="cuda", requires_grad=True)
    q_mask = (torch.rand(B, Tq, device="cuda") > 0.2).float()
    k_mask = (torch.rand(B, Tk, device="cuda") > 0.2).float()
    k_mask[0] = 0  # a user with no key at all: every weight exactly 0
    torch.manual_seed(3)
    w, out = mha(q, kv, kv, q_mask=q_mask, k_mask=k_mask, causal=causal, return_w=True)
    keep = mha.last_keep_mask
    assert keep is not None and keep.shape == (B, H, Tq, Tk) and keep.dtype == torch.uint8
    rate = float(keep.float().mean())
    assert abs(rate - (1 - p)) < 0.02
    go, gw = torch.randn_like(out), torch.randn_like(w)
    (out * go).sum().add((w * gw).sum()).backward()

    P = {"a." + k: v.detach().cpu().clone().requires_grad_(True) for k, v in mha.state_dict().items()}
    qc, kc = q.detach().cpu().requires_grad_(True), kv.detach().cpu().requires_grad_(True)
    w_o, out_o = O.mha(P, "a.", H, qc, kc, kc, q_mask.cpu(), k_mask.cpu(), causal, drop_mask=keep.cpu().float() / (1 - p))
    w_o_hm = torch.cat(list(w_o.transpose(0, 1)), dim=0)  # [B, H, Tq, Tk] -> head-major [H * B, Tq, Tk] (carca.py:242-244)
    assert float((out.detach().cpu() - out_o.detach()).abs().max()) < 2e-5
    assert float((w.detach().cpu() - w_o_hm.detach()).abs().max()) < 2e-6
    ((out_o * go.cpu()).sum() + (w_o_hm * gw.cpu()).sum()).backward()
    pairs = [("q", q.grad, qc.grad), ("kv", kv.grad, kc.grad)] + \
            [(k, dict(mha.named_parameters())[k].grad, P["a." + k].grad) for k in dict(mha.named_parameters())]
    # (WK.bias: true gradient 0 -- the softmax is invariant to a shift of a query's scores -- so what both sides hold is the
    # round-off of sums whose terms are the size of the OTHER gradients: an absolute floor relative to those)
    floor = 1e-5 * max(float(r.abs().max()) for _, _, r in pairs if r is not None)
    for name, got, ref in pairs:
        ref = ref if ref is not None else torch.zeros_like(got.cpu())
        assert float((got.cpu() - ref).abs().max()) <= 2e-4 * float(ref.abs().max()) + floor, name
    # same seed, same mask; another seed, another mask; eval mode: no mask, the dropout-free result
    torch.manual_seed(3)
    mha(q, kv, kv, q_mask=q_mask, k_mask=k_mask, causal=causal)
    assert torch.equal(mha.last_keep_mask, keep)
    torch.manual_seed(4)
    with torch.no_grad():
        mha(q, kv, kv, q_mask=q_mask, k_mask=k_mask, causal=causal)
    assert not torch.equal(mha.last_keep_mask, keep)
    mha.eval()
    with torch.no_grad():
        out_e = mha(q, kv, kv, q_mask=q_mask, k_mask=k_mask, causal=causal)
    assert mha.last_keep_mask is None
    _, out_eo = O.mha({k: v.detach() for k, v in P.items()}, "a.", H, qc.detach(), kc.detach(), kc.detach(), q_mask.cpu(),
                      k_mask.cpu(), causal)
    assert float((out_e.cpu() - out_eo).abs().max()) < 2e-5
