"""The reference of the diversity re-rank tests: greedy maximal marginal relevance stated in float64
over the SAME fp32 table rows and pool scores, vectorised over the users of a batch.  CPU only.

  valid entry:  1 <= id < n_items
  sim(a, b)  =  X[a] . X[b] ("dot")  or  ((X[a] . X[b]) r_a) r_b,  r = 1 / max(||X[.]||, 1e-12)  ("cosine")
  rel_j      =  (s_j - s_min) / (s_max - s_min) over the user's valid entries, 0 where s_max == s_min; or s_j
  step t     :  obj_j = lam rel_j - (1 - lam) M_j,  M_j = 0 at t = 0, else max over the selected s of sim(id_j, id_s);
                the largest obj wins, ties to the smaller pool position
  ild        =  mean over pairs of the selected entries of 1 - sim (0 with fewer than two)"""
import torch

NEG = float("-inf")


def margin(n_cols):
    """The objective margin of an fp32 run: the Cauchy-Schwarz bound (n_cols + 8) 2^-24 on an fp32 cosine of n_cols terms,
    counted twice for the max over the prefix and twice for rel."""
    return 4.0 * (n_cols + 8) * 2.0 ** -24


def pool_sims(X, ids, n_cols, metric, dtype=torch.float64):
    """(G [B, P, P]: sim between the pool entries of each user in `dtype`, valid [B, P])."""
    n = X.shape[0]
    ids = ids.to(torch.int64)
    valid = (ids >= 1) & (ids < n)
    rows = X[:, :n_cols].to(dtype)[torch.where(valid, ids, torch.zeros_like(ids))]
    G = rows @ rows.transpose(1, 2)
    if metric == "cosine":
        r = 1.0 / torch.sqrt((rows * rows).sum(-1)).clamp_min(1e-12)
        G = (G * r[:, :, None]) * r[:, None, :]
    elif metric != "dot":
        raise ValueError(metric)
    return G, valid


def relevance(scores, valid, normalize):
    s = scores.to(torch.float64)
    if not normalize:
        return s
    lo = torch.where(valid, s, torch.full_like(s, float("inf"))).min(1, keepdim=True).values
    hi = torch.where(valid, s, torch.full_like(s, NEG)).max(1, keepdim=True).values
    rng = hi - lo
    return torch.where(rng > 0, (s - lo) / torch.where(rng > 0, rng, torch.ones_like(rng)), torch.zeros_like(s))


def greedy(G, scores, valid, k, lam, normalize=True, forced=None):
    """The greedy path in float64.  forced: None, or positions [B, k] (-1 = none) to walk instead of the arg max.
    -> dict(pos [B, k] int64, -1 where no valid entry was left; deficit [B, k]: the step's maximal objective minus the
    objective of the entry taken (0 on the reference's own path); gap [B, k]: the step's best minus second-best objective
    (inf with one live entry); ild [B])."""
    B, P = scores.shape
    rel = relevance(scores, valid, normalize)
    live = valid.clone()
    M = torch.zeros(B, P, dtype=torch.float64)
    pos = torch.full((B, k), -1, dtype=torch.int64)
    deficit = torch.zeros(B, k, dtype=torch.float64)
    gap = torch.full((B, k), float("inf"), dtype=torch.float64)
    div_sum = torch.zeros(B, dtype=torch.float64)
    count = torch.zeros(B, dtype=torch.int64)
    rows = torch.arange(B)
    for t in range(k):
        obj = torch.where(live, lam * rel - (1.0 - lam) * M, torch.full_like(rel, NEG))
        any_live = live.any(1)
        top2 = torch.topk(obj, min(2, P), dim=1).values
        pick = torch.argmax(obj, 1)  # (the first of equal maxima: the smaller pool position)
        if forced is not None:
            f = forced[:, t]
            assert bool(((f >= 0) == any_live).all()), "the walked path stops where valid entries remain, or goes on without"
            pick = torch.where(f >= 0, f, pick)
            assert bool(live[rows, pick][any_live].all()), "the walked path takes an invalid or already taken entry"
        deficit[:, t] = torch.where(any_live, top2[:, 0] - obj[rows, pick], torch.zeros(B, dtype=torch.float64))
        if P > 1:
            gap[:, t] = torch.where(top2[:, 1] > NEG, top2[:, 0] - top2[:, 1], gap[:, t])
        pos[:, t] = torch.where(any_live, pick, pos[:, t])
        sim = G[rows, :, pick]  # sim(id_j, id_pick) for every j
        # the pick's similarities to the entries taken before it: M holds their max, its share of the ILD sum their sum
        taken_before = valid & ~live
        div_sum += torch.where(any_live, ((1.0 - sim) * taken_before).sum(1), torch.zeros(B, dtype=torch.float64))
        count += any_live.to(torch.int64)
        M = torch.where(any_live[:, None], sim if t == 0 else torch.maximum(M, sim), M)
        live[rows[any_live], pick[any_live]] = False
    pairs = (count * (count - 1) // 2).to(torch.float64)
    ild = torch.where(pairs > 0, div_sum / pairs.clamp_min(1.0), torch.zeros(B, dtype=torch.float64))
    return dict(pos=pos, deficit=deficit, gap=gap, ild=ild)


def gather_outputs(scores, ids, pos):
    """What the call returns for a path: (scores [B, k] -- the pool's values, ids [B, k] int64), (0, 0) where pos is -1."""
    p = pos.clamp_min(0)
    s = torch.where(pos >= 0, scores.gather(1, p), torch.zeros((), dtype=scores.dtype))
    i = torch.where(pos >= 0, ids.to(torch.int64).gather(1, p), torch.zeros((), dtype=torch.int64))
    return s, i


def greedy_int(X, ids, scores, n_cols, k):
    """The exact path for an integer table and integer scores with metric "dot", normalize=False, lam = 1/2, in int64:
    2 obj_j = s_j - M_j, ties to the smaller position.  -> pos [B, k] (-1 = none)."""
    G, valid = pool_sims(X.to(torch.int64), ids, n_cols, "dot", torch.int64)
    B, P = ids.shape
    s = scores.to(torch.int64)
    assert bool((s.to(scores.dtype) == scores).all())
    live, M = valid.clone(), torch.zeros(B, P, dtype=torch.int64)
    pos = torch.full((B, k), -1, dtype=torch.int64)
    rows = torch.arange(B)
    low = torch.iinfo(torch.int64).min
    for t in range(k):
        obj = torch.where(live, s - M, torch.full_like(s, low))
        best = obj.max(1, keepdim=True).values
        pick = ((obj == best) & live).to(torch.int64).argmax(1)  # the first live maximum
        any_live = live.any(1)
        pos[:, t] = torch.where(any_live, pick, pos[:, t])
        sim = G[rows, :, pick]
        M = torch.where(any_live[:, None], sim if t == 0 else torch.maximum(M, sim), M)
        live[rows[any_live], pick[any_live]] = False
    return pos


def positions_of(ids_out, pool_ids):
    """The pool position of each returned id for pools of DISTINCT valid ids: [B, k], -1 for the padding id 0."""
    eq = (ids_out.to(torch.int64)[:, :, None] == pool_ids.to(torch.int64)[:, None, :]) & (ids_out != 0)[:, :, None]
    assert bool((eq.sum(-1) <= 1).all())
    return torch.where(eq.any(-1), eq.to(torch.int64).argmax(-1), torch.full_like(ids_out, -1))
