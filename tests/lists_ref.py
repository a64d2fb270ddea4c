"""A pure-torch reference of the selection CARCA.recommend_from makes over each user's own list, given the scores of the
list's entries: per user the distinct valid ids minus the excluded ones, ordered by (score descending, id ascending),
the first k, padded with id 0 and score 0.  It checks selection, not scoring."""
import torch


def lists_topk(scores, items, n_items, k, excluded=None):
    """scores [B, N] float, items [B, N] int (CPU tensors; a repeated id carries one score, the first is taken);
    excluded: None or one set of ids per user.  -> (scores [B, k] of scores' dtype, ids [B, k] int64)."""
    B, N = items.shape
    out_s = torch.zeros(B, k, dtype=scores.dtype)
    out_i = torch.zeros(B, k, dtype=torch.int64)
    for u in range(B):
        seen = {}
        for j in range(N):
            i = int(items[u, j])
            if 1 <= i < n_items and i not in seen and not (excluded is not None and i in excluded[u]):
                seen[i] = j
        order = sorted(seen, key=lambda i: (-float(scores[u, seen[i]]), i))[:k]
        for r, i in enumerate(order):
            out_s[u, r], out_i[u, r] = scores[u, seen[i]], i
    return out_s, out_i


def positive_rank(ids, pos):
    """The position of pos [B] in ids [B, k] (the positive's rank in the list), -1 where it is not there."""
    hit = ids == pos.reshape(-1, 1).to(ids.dtype)
    at = hit.to(torch.int64).argmax(dim=1)
    return torch.where(hit.any(dim=1), at, torch.full_like(at, -1))
