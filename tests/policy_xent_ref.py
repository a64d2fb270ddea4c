"""Float64 torch reference for ops.policy_xent, CARCA.log_prob_rows and catalogue.policy_objective (DESIGN.md section
29), shared by tests/test_policy_objective_host.py and tests/test_hip_policy_xent.py: the masked log-softmax, the entropy
and the objectives, written densely so that torch.autograd gives every gradient.  Runs on whatever device its inputs are
on; nothing here calls the package's kernels."""
import numpy as np
import torch

from tests import policy_ref as PR


def eligible(n_items: int, R: int, excl=None, device="cpu") -> torch.Tensor:
    """[R, n_items] bool: class i of row r is eligible iff 1 <= i < n_items and i is not in excl[r] (0, duplicates and
    ids outside the catalogue in a list exclude nothing)."""
    el = torch.ones(R, n_items, dtype=torch.bool, device=device)
    el[:, 0] = False
    if excl is not None and excl.shape[1]:
        e = excl.to(device=device, dtype=torch.int64)
        ok = (e >= 1) & (e < n_items)
        rows = torch.arange(R, device=device).view(R, 1).expand_as(e)
        el[rows[ok], e[ok]] = False
    return el


def valid_rows(items: torch.Tensor, el: torch.Tensor) -> torch.Tensor:
    n_items = el.shape[1]
    it = items.to(device=el.device, dtype=torch.int64)
    inside = (it >= 1) & (it < n_items)
    return inside & el[torch.arange(el.shape[0], device=el.device), it.clamp(0, n_items - 1)]


def policy_rows(P: torch.Tensor, T: torch.Tensor, items: torch.Tensor, tau: float, excl=None):
    """P [R, d], T [n_items, d] float64 -> (log_prob [R], valid [R] bool, entropy [R], the eligibility [R, n_items],
    grad1 [R] = E_p|log p + H|, the 1-norm of the entropy's gradient in z, detached); log_prob and entropy are 0 on rows
    that are not valid and differentiable in P and T."""
    R, n_items = P.shape[0], T.shape[0]
    el = eligible(n_items, R, excl, P.device)
    valid = valid_rows(items, el)
    z = (P @ T.T) / tau
    z = torch.where(el, z, torch.full((), float("-inf"), dtype=z.dtype, device=z.device))
    # (a row without an eligible class is not valid; give it one finite logit so that no nan reaches the graph)
    z = torch.where(el.any(1, keepdim=True), z, torch.zeros((), dtype=z.dtype, device=z.device))
    lp = torch.log_softmax(z, dim=1)
    p = torch.exp(lp)
    ent = -(p * torch.where(el, lp, torch.zeros((), dtype=z.dtype, device=z.device))).sum(1)
    it = items.to(device=P.device, dtype=torch.int64).clamp(0, n_items - 1)
    own = lp[torch.arange(R, device=P.device), it]
    zero = torch.zeros((), dtype=z.dtype, device=z.device)
    grad1 = (p * torch.where(el, lp + ent.unsqueeze(1), zero).abs()).sum(1).detach()
    return torch.where(valid, own, zero), valid, torch.where(valid, ent, zero), el, grad1


def objective(log_probs, valid, logged, rewards, kind, clip=None, entropy=None, entropy_coef=0.0):
    """catalogue.policy_objective restated over the valid rows alone, float64."""
    ok = valid.bool()
    lp = log_probs.double()[ok]
    r = rewards.double()[ok]
    n = lp.numel()
    if n == 0:
        return (log_probs.double() * 0.0).sum() + (0.0 if entropy is None else (entropy.double() * 0.0).sum())
    if kind == "weighted_nll":
        w0 = torch.ones_like(lp) if logged is None else torch.exp(lp.detach() - logged.double()[ok])
        loss = -(r * w0 * lp).mean()
    else:
        w = torch.exp(lp - logged.double()[ok])
        if kind == "ips":
            loss = -(r * w).mean()
        elif kind == "clipped_ips":
            loss = -(r * torch.clamp(w, max=float(clip))).mean()
        elif kind == "snips":
            loss = -(r * w).sum() / w.sum()
        else:
            raise ValueError(kind)
    if entropy_coef:
        loss = loss - entropy_coef * entropy.double()[ok].mean()
    return loss


def objective_numpy(log_probs, valid, logged, rewards, kind, clip=None, entropy=None, entropy_coef=0.0) -> float:
    """The closed forms in numpy float64."""
    ok = np.asarray(valid, dtype=bool)
    lp = np.asarray(log_probs, dtype=np.float64)[ok]
    r = np.asarray(rewards, dtype=np.float64)[ok]
    if lp.size == 0:
        return 0.0
    lg = None if logged is None else np.asarray(logged, dtype=np.float64)[ok]
    if kind == "weighted_nll":
        out = -np.mean(r * (1.0 if lg is None else np.exp(lp - lg)) * lp)
    else:
        w = np.exp(lp - lg)
        out = {"ips": lambda: -np.mean(r * w), "clipped_ips": lambda: -np.mean(r * np.minimum(w, clip)),
               "snips": lambda: -(r * w).sum() / w.sum()}[kind]()
    if entropy_coef:
        out -= entropy_coef * np.mean(np.asarray(entropy, dtype=np.float64)[ok])
    return float(out)


def logit_format_tol(P: torch.Tensor, T: torch.Tensor, tau: float) -> torch.Tensor:
    """[R]: what fp32 may move a row's logits / tau by: (d + 64) 2^-24 max_i sum_k |P[r, k] T[i, k]| / tau -- d rounded
    products and sums of the exact-fp32 MFMA chain plus 64 ulps for the scaling by 1 / tau and the subtractions."""
    d = P.shape[1]
    return (d + 64) * 2.0 ** -24 * (P.abs() @ T.abs().T).max(1).values / tau


def log_prob_tol(P, T, tau, el) -> torch.Tensor:
    """[R]: logit_format_tol + policy_ref.entropy_format_tol(n_eligible), the reduction's share."""
    n_el = el.sum(1).cpu().numpy()
    fmt = torch.tensor([PR.entropy_format_tol(int(n)) for n in n_el], dtype=torch.float64, device=P.device)
    return logit_format_tol(P, T, tau) + fmt


def entropy_tol(P, T, tau, el, grad1) -> torch.Tensor:
    """[R]: the entropy moves with the logits through its gradient dH/dz_i = -p_i (log p_i + H), whose 1-norm is grad1 =
    E_p|log p + H| (policy_rows' last output): logit_format_tol grad1 + entropy_format_tol(n_eligible), the form
    tests/test_hip_policy.py::test_entropy uses."""
    n_el = el.sum(1).cpu().numpy()
    fmt = torch.tensor([PR.entropy_format_tol(int(n)) for n in n_el], dtype=torch.float64, device=P.device)
    return logit_format_tol(P, T, tau) * grad1 + fmt


# ---- the model level: the float64 oracle's rows and item table -------------------------------------------------------
def oracle_rows(Pg, cfg, attrs, p_x, p_c, n_items, masks=None):
    """(rows [B L, d], T [n_items, d]) float64, differentiable in the parameter dict Pg: the final profile rows with the
    decoder's slot weights and the item table under a zero context, as tests/test_hip_catalogue_xent.py::_oracle_loss
    forms them."""
    from oracle import carca_oracle as O

    B, L = p_x.shape
    trace = {}
    O.carca_forward(Pg, cfg, (p_x, attrs[p_x], p_c), [(p_x, attrs[p_x], p_c)], training=True, trace=trace, masks=masks)
    p = trace["p_final"]
    if cfg.decoder == "wdot":
        w = torch.tril((cfg.gamma ** torch.arange(0, L)).unsqueeze(0).expand(L, L)).to(p.dtype).sum(1)
        p = p * w.view(1, L, 1)
    ids = torch.arange(n_items).view(1, -1)
    zero = torch.zeros(1, n_items, p_c.shape[-1], dtype=torch.float64)
    T = O.embedding(Pg, cfg, ids, attrs[ids], zero, O.get_mask(ids, torch.float64), target=True)[0]
    return p.reshape(B * L, -1), T


def profile_lists(p_x: torch.Tensor) -> torch.Tensor:
    """exclude="profile" by its definition, with loops: [B, L, L], row (b, t) the non-zero ids of p_x[b, :t + 1] ascending,
    zeros in front."""
    B, L = p_x.shape
    out = torch.zeros(B, L, L, dtype=torch.int64)
    for b in range(B):
        for t in range(L):
            ids = sorted(int(v) for v in p_x[b, :t + 1].tolist() if v != 0)
            if ids:
                out[b, t, L - len(ids):] = torch.tensor(ids)
    return out


def model_rows(Pg, cfg, attrs, p_x, p_c, n_items, items, tau, exclude=None, masks=None):
    """CARCA.log_prob_rows over the oracle: -> (log_probs [B, L], valid [B, L], entropy [B, L]) float64.  exclude: None,
    "profile" or an int [B, L, E] tensor.  A row whose own slot is padding is not valid."""
    B, L = p_x.shape
    rows, T = oracle_rows(Pg, cfg, attrs, p_x, p_c, n_items, masks)
    excl = profile_lists(p_x) if isinstance(exclude, str) else exclude
    it = torch.where(p_x != 0, items, torch.zeros_like(items)).reshape(-1)
    lp, valid, ent, _, _ = policy_rows(rows, T, it, tau, None if excl is None else excl.reshape(B * L, -1))
    return lp.view(B, L), valid.view(B, L), ent.view(B, L)


def exact_log_batch():
    """The learning check's inputs (policy_ref.e2e_inputs()'s user and reward): an exact log -- every eligible item once,
    with its true logging probability p_a as propensity -- for a dot-decoder policy over the same user.  -> dict(cfg, P,
    attrs, n, p_x [I, L], p_c [I, L, n_ctx], ctx [I, n_ctx], ids [I, 1], logged [I, 1], reward [I], tau)."""
    from tests import sampling_ref as R

    e = PR.e2e_inputs()
    n, L = R.DIST["n"], R.DIST["L"]
    cfg, P, attrs, (p_x, p_c, ctx) = R.oracle_setup("dot64x2", L, 1, n, seed=3)
    assert torch.equal(p_x, e["batch"][0])  # the same user
    I = len(e["ids"])
    rep = lambda t: t.expand(I, *t.shape[1:]).contiguous()  # noqa: E731
    return dict(cfg=cfg, P=P, attrs=attrs, n=n, p_x=rep(p_x), p_c=rep(p_c), ctx=rep(ctx),
                ids=torch.from_numpy(e["ids"]).view(I, 1), logged=torch.from_numpy(np.log(e["p_a"])).view(I, 1),
                reward=torch.from_numpy(e["reward"]), tau=32.0)


LEARNING_STEPS, LEARNING_RATE = 20, 0.05


def reference_step(Pg, b):
    """One evaluation of the learning check's objective over the float64 oracle: -> (the IPS loss, the policy's exact
    value sum p_theta r over the user's eligible items), both differentiable in Pg."""
    from carca_replication_amd import catalogue

    L = b["p_x"].shape[1]
    items, lg, rew = catalogue.off_policy_rows(tuple(b["p_x"].shape), b["ids"], b["logged"], b["reward"])
    lp, valid, _ = model_rows(Pg, b["cfg"], b["attrs"], b["p_x"], b["p_c"], b["n"], items, b["tau"], "profile")
    loss = objective(lp, valid, lg, rew, "ips")
    value = (torch.exp(lp[:, L - 1]) * b["reward"]).sum()
    return loss, value
