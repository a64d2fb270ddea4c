"""Reference for CARCA.explain_items / explain_top_slots, pure torch on the CPU.

In eval mode the cross-attention decoder's logit is additive over the profile slots (carca.py:253-263, 338-347):
    logit(u, i) = base(u, i) + sum_t contrib(u, i, t),    contrib(u, i, t) = sum_h w_h(u, i, t) U[u, t, h],
with w the reference's return_w weights, U[u, t, h] = w_ffn,h . V[u, t, h] the decoder FFN folded into the value rows and
base = the FFN bias (+ w_ffn . e(i, context) with the residual).  oracle_explain takes all of it from
oracle.carca_forward's trace in float64; top_slots is the selection explain_top_slots makes over a dense contrib."""
import torch

from oracle import carca_oracle as O


def oracle_explain(cfg, P, attrs, batch, items):
    """items [B, N] int64 (any ids) -> float64 (y [B, N], base [B, N], contrib [B, N, L], weights [B, H, N, L], live [B, N]);
    an id that is no item has y = base = 0 and zero rows."""
    p_x, p_c, ctx = batch
    B, N = items.shape
    n = attrs.shape[0]
    live = (items >= 1) & (items < n)
    ids = torch.where(live, items, torch.zeros_like(items))
    o_c = ctx.unsqueeze(1).expand(B, N, ctx.shape[1])
    tr = {}
    y = O.carca_forward(P, cfg, (p_x, attrs[p_x], p_c), [(ids, attrs[ids], o_c)], training=False, trace=tr).reshape(B, N)
    return (y * live,) + decompose(cfg, P, tr["dec_w0"], tr["p_final"], tr["o_embed0"], live) + (live,)


def decompose(cfg, P, w, p_final, o_embed, live):
    """(base [B, N], contrib [B, N, L], weights [B, H, N, L]) from the trace's dec_w0, p_final and o_embed0."""
    B, L, d = p_final.shape
    H = cfg.H
    V = p_final @ P["decoder.attn.WV.weight"].T + P["decoder.attn.WV.bias"]
    fw = P["decoder.ffn.weight"].reshape(-1)
    U = (V * fw).view(B, L, H, d // H).sum(-1)  # [B, L, H]
    w = w * live.unsqueeze(1).unsqueeze(-1)
    contrib = torch.einsum("bhnl,blh->bnl", w, U)
    base = P["decoder.ffn.bias"].reshape(()) + ((o_embed @ fw) if cfg.residual_ca else torch.zeros(live.shape, dtype=w.dtype))
    return base * live, contrib, w


def top_slots(contrib, p_x, m, live=None):
    """The m valid slots (p_x[u, t] != 0) with the largest contrib per (u, j), descending, ties to the LATER slot; stable.
    contrib [B, N, L], p_x [B, L]; live [B, N] bool: entries that are items (None: all).  -> (slots [B, N, m] int64,
    slot_items [B, N, m] int64, values [B, N, m] of contrib's dtype), padded with (-1, 0, 0)."""
    B, N, L = contrib.shape
    slots = torch.full((B, N, m), -1, dtype=torch.int64)
    items = torch.zeros(B, N, m, dtype=torch.int64)
    vals = torch.zeros(B, N, m, dtype=contrib.dtype)
    for b in range(B):
        v = torch.nonzero(p_x[b] != 0).reshape(-1).flip(0)  # later slots first: a stable sort keeps them ahead in a tie
        if v.numel() == 0:
            continue
        c = contrib[b][:, v]
        order = torch.sort(c, dim=1, descending=True, stable=True).indices[:, :m]
        k = order.shape[1]
        slots[b, :, :k] = v[order]
        items[b, :, :k] = p_x[b][v[order]]
        vals[b, :, :k] = torch.gather(c, 1, order)
    if live is not None:
        dead = ~live
        slots[dead], items[dead], vals[dead] = -1, 0, 0
    return slots, items, vals
