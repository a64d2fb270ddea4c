"""The algebra csrc/recommend.hip relies on, pinned in fp64 over the CPU oracle: in eval mode every
embedding is affine in the context, e(i, c) = T[i] + M c (i != 0), and each decoder's score of (user, item) factorises
into per-item tables (T, QT, wT), per-user rows (K, folded values u, beta, M c) and a per-pair masked softmax or dot.
The factorised logit must equal the oracle's score with the whole catalogue as one target group."""
import itertools

import pytest
import torch

from oracle import carca_oracle as O

N_ITEMS, G, N_ATTRS, L, B = 40, 10, 7, 9, 4


def _factorised(P, cfg, attrs, p_x, p_c, ctx, n_ctx):
    d, H = cfg.d, cfg.H
    ids = torch.arange(N_ITEMS).view(1, -1)
    zero = torch.zeros(1, N_ITEMS, n_ctx, dtype=torch.float64)
    T = O.embedding(P, cfg, ids, attrs[ids], zero, O.get_mask(ids, torch.float64), target=True)[0]  # e(i, 0)
    assert torch.all(T[0] == 0)
    M = torch.zeros(d, n_ctx, dtype=torch.float64)
    if n_ctx and cfg.embedding == "all":
        M = P["embeds.joint_embed.weight"][:, d:] @ P["embeds.feats_embed.weight"][:, N_ATTRS:]
    elif n_ctx and cfg.embedding == "attrctx":
        M = P["embeds.joint_embed.weight"] @ P["embeds.feats_embed.weight"][:, N_ATTRS:]
    mc = ctx @ M.T                                                                                  # [B, d]
    trace = {}
    O.carca_forward(P, cfg, (p_x, attrs[p_x], p_c), [(ids[:, 1:2].expand(B, 1), attrs[ids[:, 1:2]].expand(B, 1, N_ATTRS),
                                                        ctx.unsqueeze(1))], training=False, trace=trace)
    p = trace["p_final"]                                                                            # [B, L, d]
    if cfg.decoder == "ca":
        pre = "decoder.attn."
        Wq, bq, Wk, bk = (P[pre + n] for n in ("WQ.weight", "WQ.bias", "WK.weight", "WK.bias"))
        Wv, bv = P[pre + "WV.weight"], P[pre + "WV.bias"]
        w, b = P["decoder.ffn.weight"][0], P["decoder.ffn.bias"][0]
        dh = d // H
        QT = T @ Wq.T + bq                                 # per item
        dq = mc @ Wq.T                                     # per user
        K = p @ Wk.T + bk
        V = p @ Wv.T + bv
        u = (V.view(B, L, H, dh) * w.view(1, 1, H, dh)).sum(-1)                      # folded values [B, L, H]
        Kh = K.view(B, L, H, dh)
        beta = torch.einsum("bhc,blhc->bhl", dq.view(B, H, dh), Kh)                 # [B, H, L]
        s = (torch.einsum("ihc,blhc->bihl", QT.view(N_ITEMS, H, dh), Kh) + beta.unsqueeze(1)) / dh ** 0.5
        valid = (p_x != 0).view(B, 1, 1, L)
        s = s.masked_fill(~valid, float("-inf"))
        a = torch.softmax(s, -1).nan_to_num(0.0)                                     # fully masked profile: 0
        logit = torch.einsum("bihl,blh->bi", a, u) + b
        if cfg.residual_ca:
            logit = logit + (T @ w).view(1, -1) + (mc @ w).view(-1, 1)
        return torch.sigmoid(logit)
    last = p[:, -1]
    if cfg.decoder == "wdot":
        last = last * (cfg.gamma ** torch.arange(0, L)).to(torch.float64).sum()  # the float32 slot weights of carca.py:376
        if cfg.l2_norm:
            last = last / last.norm(dim=-1, keepdim=True).clamp(min=1e-12)
    dot = last @ T.T + (last * mc).sum(-1, keepdim=True)                            # p . (T[i] + M c)
    if cfg.decoder == "wdot" and cfg.l2_norm:
        n2 = (T * T).sum(-1).view(1, -1) + 2 * mc @ T.T + (mc * mc).sum(-1, keepdim=True)  # ||T[i] + M c||^2
        return (dot / n2.clamp(min=0).sqrt().clamp(min=1e-12) + 1) / 2
    return torch.sigmoid(dot)


DECODERS = [("ca", False, True), ("ca", False, False), ("dot", False, True), ("wdot", False, True), ("wdot", True, True)]


@pytest.mark.parametrize("emb,dec,n_ctx", [(e, dc, n) for e, dc, n in itertools.product(
    ["all", "attrctx", "attr", "id", "mlpid"], DECODERS, [0, 6])])
def test_factorised_logit_equals_oracle(emb, dec, n_ctx):
    kind, l2, res = dec
    H = 2
    cfg = O.CarcaConfig(d=8, H=H, n_blocks=1, residual_ca=res, encoding="learnable", embedding=emb, decoder=kind,
                        l2_norm=l2)
    P = O.perturb_params(O.init_params(cfg, N_ITEMS, G, n_ctx, N_ATTRS, L, seed=3, dtype=torch.float64), seed=4,
                         scale=0.3)
    gen = torch.Generator().manual_seed(5)
    attrs = torch.rand(N_ITEMS, N_ATTRS, generator=gen, dtype=torch.float64)
    attrs[0] = 0
    p_x = torch.randint(1, N_ITEMS, (B, L), generator=gen)
    p_x[0] = 0                  # a fully padded profile
    p_x[1, :-1] = 0             # a one-item profile
    p_x[2, :3] = 0              # left padding
    p_c = torch.rand(B, L, n_ctx, generator=gen, dtype=torch.float64) * (p_x != 0).unsqueeze(-1)
    ctx = torch.rand(B, n_ctx, generator=gen, dtype=torch.float64)
    ids = torch.arange(1, N_ITEMS).expand(B, -1)
    want = O.carca_forward(P, cfg, (p_x, attrs[p_x], p_c), [(ids, attrs[ids], ctx.unsqueeze(1).expand(B, N_ITEMS - 1,
                                                                                                        n_ctx))],
                           training=False).reshape(B, N_ITEMS - 1)
    got = _factorised(P, cfg, attrs, p_x, p_c, ctx, n_ctx)[:, 1:]
    assert float((got - want).abs().max()) < 1e-10
