"""The reference of the similar_items tests: the formula of the call stated in fp64 over the SAME fp32
table rows, its fp32 evaluation for the score tolerance, and the comparison rules.  CPU only.

  dot:    score(q, i) = sum_c X[q, c] X[i, c]
  cosine: score(q, i) = ((X[q] . X[i]) * r_q) * r_i,  r_i = 1 / max(sqrt(sum_c X[i, c]^2), 1e-12)
Eligible: ids 1 .. n_items - 1, minus the query when exclude_self, intersected with `allowed` when given.  Order: score
descending, ties to the smaller id.  Fewer than k eligible items, or a query id outside [1, n_items): (id 0, score 0)."""
import torch

EPS32 = float(torch.finfo(torch.float32).eps)


def ref_scores(X, n_cols, metric, dtype):
    """[n_items, n_items] scores of every (query, item) pair, the statement above evaluated in `dtype`."""
    Y = X[:, :n_cols].to(dtype)
    s = Y @ Y.t()
    if metric == "cosine":
        r = 1.0 / torch.sqrt((Y * Y).sum(1)).clamp_min(1e-12)
        s = (s * r[:, None]) * r[None, :]
    elif metric != "dot":
        raise ValueError(metric)
    return s


def ref_topk(S64, items, k, exclude_self=True, allowed=None):
    """S64 [n_items, n_items] from ref_scores; items: a list of query ids.  -> (scores [Q, k] fp64, ids [Q, k] int64, the
    sorted eligible scores per query, the eligible ids in that order per query)."""
    n = S64.shape[0]
    Q = len(items)
    out_s, out_i = torch.zeros(Q, k, dtype=torch.float64), torch.zeros(Q, k, dtype=torch.int64)
    full, order = [], []
    base = torch.zeros(n, dtype=torch.bool)
    if allowed is None:
        base[1:] = True
    else:
        a = torch.as_tensor(sorted(set(int(i) for i in allowed if 1 <= int(i) < n)), dtype=torch.int64)
        base[a] = True
    for j, q in enumerate(int(i) for i in items):
        if not 1 <= q < n:
            full.append(torch.zeros(0, dtype=torch.float64)), order.append(torch.zeros(0, dtype=torch.int64))
            continue
        el = base.clone()
        if exclude_self:
            el[q] = False
        ids = torch.nonzero(el).reshape(-1)  # ascending: a stable sort leaves ties to the smaller id
        s, at = torch.sort(S64[q, ids], descending=True, stable=True)
        m = min(k, ids.numel())
        out_s[j, :m], out_i[j, :m] = s[:m], ids[at][:m]
        full.append(s), order.append(ids[at])
    return out_s, out_i, full, order


def score_tolerance(S32, S64):
    """The project's rule (tests/test_hip_row_kernels.py): 8 x the fp32 reference's own error + 4 eps32 max|ref64|."""
    return 8.0 * float((S32.double() - S64).abs().max()) + 4.0 * EPS32 * float(S64.abs().max())


def clear_positions(full, k, scale, ties=False):
    """Per query, a bool [min(k, eligible)] mask of the positions whose ids are compared: both neighbours in the reference
    order more than 1e-5 max(1, max|ref64|) away.  ties: neighbours with exactly the reference's score (duplicate rows)
    do not count -- the nearest DIFFERENT score decides."""
    thr = 1e-5 * max(1.0, scale)
    out = []
    for s in full:
        m = min(k, s.numel())
        if ties and s.numel():
            vals, inv = torch.unique_consecutive(s, return_inverse=True)
            gap_v = torch.full((vals.numel(),), float("inf"), dtype=torch.float64)
            if vals.numel() > 1:
                dv = vals[:-1] - vals[1:]
                gap_v[:-1] = torch.minimum(gap_v[:-1], dv)
                gap_v[1:] = torch.minimum(gap_v[1:], dv)
            out.append((gap_v[inv] > thr)[:m])
            continue
        gap = torch.full((s.numel(),), float("inf"), dtype=torch.float64)
        if s.numel() > 1:
            d = s[:-1] - s[1:]
            gap[:-1] = torch.minimum(gap[:-1], d)
            gap[1:] = torch.minimum(gap[1:], d)
        out.append((gap > thr)[:m])
    return out


def compared_share(clear):
    total = sum(int(c.numel()) for c in clear)
    return sum(int(c.sum()) for c in clear) / max(total, 1)


def check(got, want, full, k, tol, scale, ties=False, min_share=0.9):
    """got = (scores [Q, k], ids [Q, k]) from the device; want = ref_topk's first two outputs.  Scores within tol at every
    position, padding exact, ids equal at every clear position; at least min_share of the positions are compared."""
    gs, gi = got[0].detach().cpu(), got[1].detach().cpu()
    ws, wi = want
    assert gs.dtype == torch.float32 and gi.dtype == torch.int64 and gs.shape == ws.shape and gi.shape == wi.shape
    clear = clear_positions(full, k, scale, ties)
    share = compared_share(clear)
    print(f"compared share of positions: {share:.4f}; tol {tol:.3e}")
    for j, s in enumerate(full):
        m = min(k, s.numel())
        err = float((gs[j, :m].double() - ws[j, :m]).abs().max()) if m else 0.0
        assert err <= tol, (j, err, tol)
        assert not bool(gs[j, m:].any()) and not bool(gi[j, m:].any()), j  # padding: (0, 0.0)
        c = clear[j]
        assert torch.equal(gi[j, :m][c], wi[j, :m][c]), j
        assert bool(((gi[j, :m] >= 1)).all()), j
    assert share >= min_share, share
    return share
