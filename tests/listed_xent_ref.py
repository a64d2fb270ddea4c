"""The reference of the softmax cross-entropy over per-list negatives (ops.listed_xent) in plain torch,
at the operands' precision (the tests pass float64 and differentiate it with autograd): gather, masked logsumexp, mean."""
import torch


def list_index(lists, n_items):
    """(ids [U], index [G, N]) of lists [G, N] by a plain Python loop: the distinct ids in [1, n_items) ascending, and the
    position of each entry in them, -1 for an entry that is no class."""
    rows = [[int(x) for x in row] for row in lists.tolist()]
    ids = sorted({x for row in rows for x in row if 1 <= x < n_items})
    at = {x: u for u, x in enumerate(ids)}
    index = [[at.get(x, -1) if 1 <= x < n_items else -1 for x in row] for row in rows]
    return torch.tensor(ids, dtype=torch.int64), torch.tensor(index, dtype=torch.int64).reshape(lists.shape)


def ref_loss(P, Tp, pos, S, lists, index, rows_per_list, n_items, bias=None, pos_bias=None):
    """mean over valid r of logsumexp({z(r, +)} U {z(r, j) : j in N_r}) - z(r, +), with z(r, +) = P[r] . Tp[r] + pos_bias[r],
    z(r, j) = P[r] . S[index[g, j]] + bias[g, j], g = r // rows_per_list and N_r = {j : index[g, j] >= 0, lists[g, j] in
    [1, n_items), lists[g, j] != pos[r]}; row r is valid iff pos[r] lies in [1, n_items); 0 without a valid row."""
    dev = P.device
    pos, lists, index = pos.long().to(dev).reshape(-1), lists.long().to(dev), index.long().to(dev)
    G, N = lists.shape
    assert P.shape[0] == G * rows_per_list and pos.numel() == P.shape[0]
    valid = (pos >= 1) & (pos < n_items)
    zero = (P.sum() + Tp.sum() + S.sum()) * 0.0
    if not bool(valid.any()):
        return zero
    zp = (P * Tp).sum(1)
    if pos_bias is not None:
        zp = zp + pos_bias.to(dev, P.dtype).reshape(-1)
    total = zero
    for g in range(G):
        rows = torch.arange(g * rows_per_list, (g + 1) * rows_per_list, device=dev)[valid[g * rows_per_list:(g + 1) * rows_per_list]]
        if rows.numel() == 0:
            continue
        live = (index[g] >= 0) & (lists[g] >= 1) & (lists[g] < n_items)
        z = P.new_zeros(rows.numel(), N)
        if S.shape[0] > 0:
            z = P[rows] @ S[index[g].clamp(min=0)].T
        if bias is not None:
            z = z + bias[g].to(dev, P.dtype).view(1, N)
        mask = live.view(1, N) & (lists[g].view(1, N) != pos[rows].view(-1, 1))
        z = z.masked_fill(~mask, -float("inf"))
        lse = torch.logsumexp(torch.cat([zp[rows].view(-1, 1), z], 1), 1)
        total = total + (lse - zp[rows]).sum()
    return total / valid.sum()
