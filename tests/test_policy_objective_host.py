"""The host layer of training on a bandit log, without a GPU: catalogue.policy_objective's four
kinds against numpy float64 closed forms and their gradients against torch.autograd over a float64 restatement
(tests/policy_xent_ref.py), the clip's zero gradient, the empty valid set, the raise on a logged -inf, the placement of a
logged batch on log_prob_rows' rows, the exclusion lists of exclude="profile", and the learning check's premise from the
reference alone."""
import numpy as np
import pytest
import torch

from carca_replication_amd import CarcaHipError, catalogue, catalogue_xent, engine, ops
from tests import policy_xent_ref as X

KINDS = [("ips", None), ("clipped_ips", 1.3), ("snips", None), ("weighted_nll", None)]


def _rows(seed=0, B=6, L=7, frac_valid=0.6):
    g = torch.Generator().manual_seed(seed)
    lp = -torch.rand(B, L, generator=g, dtype=torch.float64) * 4.0
    logged = -torch.rand(B, L, generator=g, dtype=torch.float64) * 4.0
    ent = torch.rand(B, L, generator=g, dtype=torch.float64) * 3.0
    r = torch.randn(B, L, generator=g, dtype=torch.float64)
    valid = torch.rand(B, L, generator=g) < frac_valid
    # what rows that are not valid hold is read nowhere: make it poisonous
    logged = torch.where(valid, logged, torch.full_like(logged, float("-inf")))
    r = torch.where(valid, r, torch.full_like(r, float("nan")))
    return lp.float(), valid, logged, r, ent.float()


@pytest.mark.parametrize("kind,clip", KINDS)
@pytest.mark.parametrize("coef", [0.0, 0.01])
def test_kinds_match_closed_forms_and_autograd(kind, clip, coef):
    lp, valid, logged, r, ent = _rows(seed=len(kind))
    a, e = lp.clone().requires_grad_(True), ent.clone().requires_grad_(True)
    got = catalogue.policy_objective(a, valid, logged, r, kind, clip=clip, entropy=e, entropy_coef=coef)
    assert got.dim() == 0 and got.dtype == torch.float64
    want = X.objective_numpy(lp.numpy(), valid.numpy(), logged.numpy(), r.numpy(), kind, clip, ent.numpy(), coef)
    assert abs(got.item() - want) <= 1e-12 * max(1.0, abs(want)), (got.item(), want)
    got.backward()
    a64, e64 = lp.double().requires_grad_(True), ent.double().requires_grad_(True)
    X.objective(a64, valid, logged, r, kind, clip, e64, coef).backward()
    assert torch.allclose(a.grad.double(), a64.grad, rtol=1e-6, atol=1e-9)
    assert float(a.grad[~valid].abs().max()) == 0.0
    if coef:
        assert torch.allclose(e.grad.double(), e64.grad, rtol=1e-6, atol=1e-9)
        assert float(e.grad[~valid].abs().max()) == 0.0
    else:
        assert e.grad is None or float(e.grad.abs().max()) == 0.0


def test_weighted_nll_without_a_log_is_the_reward_weighted_likelihood():
    lp, valid, _, r, _ = _rows(seed=3)
    a = lp.clone().requires_grad_(True)
    got = catalogue.policy_objective(a, valid, None, r, "weighted_nll")
    want = X.objective_numpy(lp.numpy(), valid.numpy(), None, r.numpy(), "weighted_nll")
    assert abs(got.item() - want) <= 1e-12 * max(1.0, abs(want))
    got.backward()
    n = int(valid.sum())
    assert torch.allclose(a.grad.double()[valid], -r[valid] / n, rtol=1e-6)
    with pytest.raises(CarcaHipError, match="needs logged_log_probs"):
        catalogue.policy_objective(lp, valid, None, r, "ips")


def test_rows_at_the_cap_get_no_gradient():
    lp, valid, logged, r, _ = _rows(seed=5)
    w = torch.exp(lp.double() - logged)
    clip = float(w[valid].median())
    a = lp.clone().requires_grad_(True)
    catalogue.policy_objective(a, valid, logged, r, "clipped_ips", clip=clip).backward()
    capped = valid & (w >= clip)
    free = valid & (w < clip)
    assert bool(capped.any()) and bool(free.any())
    assert float(a.grad[capped].abs().max()) == 0.0
    assert bool((a.grad[free] != 0).all())


@pytest.mark.parametrize("kind,clip", KINDS)
def test_empty_valid_set_gives_zero_with_zero_gradients(kind, clip):
    lp, _, logged, r, ent = _rows(seed=7)
    valid = torch.zeros_like(lp, dtype=torch.bool)
    a, e = lp.clone().requires_grad_(True), ent.clone().requires_grad_(True)
    got = catalogue.policy_objective(a, valid, torch.full_like(logged, float("-inf")), r * float("nan"), kind, clip=clip,
                                     entropy=e, entropy_coef=0.5)
    got.backward()
    assert got.item() == 0.0
    assert float(a.grad.abs().max()) == 0.0 and float(e.grad.abs().max()) == 0.0


def test_a_logged_minus_inf_on_a_valid_row_raises_only_when_asked():
    lp, valid, logged, r, _ = _rows(seed=9)
    b, t = (int(v) for v in valid.nonzero()[0])
    logged[b, t] = float("-inf")
    with pytest.raises(CarcaHipError, match="cannot have drawn"):
        catalogue.policy_objective(lp, valid, logged, r, "ips")
    # the sync-free form hands the flag over instead (engine.off_policy_step ORs it into the caller's tensor)
    _, bad = catalogue._policy_objective(lp, valid, logged, r, "ips")
    assert bad.dtype == torch.bool and bool(bad)
    logged[b, t] = -1.0
    assert not bool(catalogue._policy_objective(lp, valid, logged, r, "snips")[1])


def test_argument_errors():
    lp, valid, logged, r, ent = _rows(seed=11)
    with pytest.raises(CarcaHipError, match="kind"):
        catalogue.policy_objective(lp, valid, logged, r, "dr")
    with pytest.raises(CarcaHipError, match="clip"):
        catalogue.policy_objective(lp, valid, logged, r, "clipped_ips")
    with pytest.raises(CarcaHipError, match="clip"):
        catalogue.policy_objective(lp, valid, logged, r, "ips", clip=2.0)
    with pytest.raises(CarcaHipError, match="shape"):
        catalogue.policy_objective(lp, valid[:, 1:], logged, r, "ips")
    with pytest.raises(CarcaHipError, match="entropy"):
        catalogue.policy_objective(lp, valid, logged, r, "ips", entropy_coef=0.1)


def test_off_policy_rows_put_the_first_logged_column_after_the_last_slot():
    B, L, k = 4, 6, 3
    ids = torch.arange(1, B * k + 1).view(B, k) * 5
    logged = -torch.arange(1, B * k + 1, dtype=torch.float32).view(B, k)
    for rewards in (torch.arange(B, dtype=torch.float32) + 1, (torch.arange(B * k, dtype=torch.float32) + 1).view(B, k)):
        items, lg, rew = catalogue.off_policy_rows((B, L), ids, logged, rewards)
        assert items.shape == lg.shape == rew.shape == (B, L)
        assert torch.equal(items[:, L - 1], ids[:, 0]) and not bool(items[:, :L - 1].any())
        assert torch.equal(lg[:, L - 1], logged[:, 0].double()) and not bool(lg[:, :L - 1].any())
        want = rewards if rewards.dim() == 1 else rewards[:, 0]
        assert torch.equal(rew[:, L - 1], want.double()) and not bool(rew[:, :L - 1].any())
    with pytest.raises(CarcaHipError, match="ids"):
        catalogue.off_policy_rows((B, L), ids[:, :0], logged[:, :0], torch.zeros(B))


def test_off_policy_step_places_the_action_and_refuses_other_variants():
    """engine.off_policy_step against a stand-in model that records what log_prob_rows is asked."""
    B, L = 3, 5
    seen = {}

    class Stand(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(B, L))

        def log_prob_rows(self, profile, items, temperature, exclude, with_entropy, last_slot_only):
            assert last_slot_only is True
            seen.update(items=items.clone(), temperature=temperature, exclude=exclude, with_entropy=with_entropy)
            valid = items != 0
            return self.w - 1.0, valid, (self.w * 0 + 2.0) if with_entropy else None

    m = Stand()
    opt = torch.optim.SGD(m.parameters(), lr=0.5)
    p_x = torch.randint(1, 9, (B, L))
    ids = torch.tensor([[4, 9], [7, 1], [2, 2]])
    logged = torch.full((B, 2), -1.0)
    batch = ((p_x, None, torch.zeros(B, L, 2)), torch.zeros(B, 2), ids, logged, torch.tensor([1.0, 0.0, 2.0]))
    flag = torch.zeros((), dtype=torch.bool)
    loss = engine.off_policy_step(m, opt, batch, temperature=0.5, kind="ips", undrawn=flag)
    assert torch.equal(seen["items"][:, L - 1], ids[:, 0]) and not bool(seen["items"][:, :L - 1].any())
    assert seen["temperature"] == 0.5 and seen["exclude"] == "profile" and seen["with_entropy"] is False
    assert abs(loss.item() + 1.0) < 1e-12 and not bool(flag)  # w = exp(-1 + 1) = 1: -(1 + 0 + 2) / 3
    assert torch.allclose(m.w.detach()[:, L - 1], torch.tensor([1.0, 0.0, 2.0]) / 3 * 0.5)  # one SGD step was taken
    engine.off_policy_step(m, opt, batch, kind="snips", entropy_coef=0.1)
    assert seen["with_entropy"] is True
    batch_bad = batch[:3] + (torch.full((B, 2), float("-inf")),) + batch[4:]
    engine.off_policy_step(m, opt, batch_bad, undrawn=flag)
    assert bool(flag)
    for kw in (dict(graphed=True), dict(sharded=True)):
        with pytest.raises(CarcaHipError, match="not built"):
            engine.off_policy_step(m, opt, batch, **kw)


def test_profile_exclusion_lists_hold_the_prefix_ids_sorted():
    g = torch.Generator().manual_seed(2)
    B, L, n_items = 5, 9, 40
    p_x = torch.randint(1, n_items, (B, L), generator=g)
    p_x[1] = 0
    p_x[2, :6] = 0
    p_x[3, 4] = p_x[3, 7]  # an id twice
    raw = catalogue_xent.profile_exclusion(p_x)
    assert raw.shape == (B, L, L)
    lists = ops.policy_exclusion(raw.reshape(B * L, L), B * L, n_items).view(B, L, L)
    assert lists.dtype == torch.int32
    want = X.profile_lists(p_x)
    assert torch.equal(lists.long(), want)
    for b in range(B):
        for t in range(L):
            assert [v for v in lists[b, t].tolist() if v] == sorted(v for v in p_x[b, :t + 1].tolist() if v)


def test_policy_exclusion_sorts_and_keeps_odd_ids_harmless():
    n_items = 100
    excl = torch.tensor([[70, 0, -5, 3, 3, 2 ** 40, 100], [0, 0, 0, 0, 0, 0, 0]])
    s = ops.policy_exclusion(excl, 2, n_items)
    assert s.dtype == torch.int32 and bool((s[:, 1:] >= s[:, :-1]).all())
    inside = [v for v in s[0].tolist() if 1 <= v < n_items]
    assert inside == [3, 3, 70]  # (2^40 did not wrap into the catalogue)
    valid = ops.policy_valid_rows(torch.tensor([3, 5], dtype=torch.int32), s, n_items)
    assert valid.tolist() == [False, True]
    assert ops.policy_exclusion(None, 2, n_items) is None and ops.policy_exclusion(excl[:, :0], 2, n_items) is None
    with pytest.raises(CarcaHipError, match="excl"):
        ops.policy_exclusion(excl.float(), 2, n_items)


def test_transposed_lists_name_the_valid_rows_that_exclude_each_item():
    g = torch.Generator().manual_seed(4)
    R, E, n_items = 37, 6, 23
    excl = torch.randint(-2, n_items + 3, (R, E), generator=g)
    items = torch.randint(0, n_items + 1, (R,), generator=g).int()
    s = ops.policy_exclusion(excl, R, n_items)
    valid = ops.policy_valid_rows(items, s, n_items)
    el = X.eligible(n_items, R, excl)
    assert torch.equal(valid, X.valid_rows(items, el))
    t_off, t_rows = ops.policy_transposed_lists(s, valid, n_items)
    assert t_off.shape == (n_items + 1,) and t_off.dtype == torch.int32 and t_rows.dtype == torch.int32
    rank = (torch.cumsum(valid.long(), 0) - 1).tolist()
    for i in range(1, n_items):
        got = t_rows[t_off[i]: t_off[i + 1]].tolist()
        want = sorted(rank[r] for r in range(R) if valid[r] for v in excl[r].tolist() if v == i)
        assert got == want, i


def test_temperature_check():
    for bad in (0.0, -1.0, float("inf"), float("nan"), 1e-46, "1", True, None):
        with pytest.raises(CarcaHipError, match="temperature"):
            ops.policy_temperature("log_prob_rows", bad)
    assert ops.policy_temperature("log_prob_rows", 0.25) == 0.25


def test_reference_alone_the_exact_logs_ips_step_raises_the_policys_value():
    """The learning check's premise (tests/test_hip_policy_xent.py::test_learning_on_an_exact_log), from the float64
    reference alone: LEARNING_STEPS steps of plain SGD at LEARNING_RATE on the IPS objective of the exact log raise the
    policy's exact value sum p_theta r.  (With every eligible item logged once rather than in proportion to p_a, the IPS
    mean is sum_a p_theta(a) r(a) / (I p_a(a)): linear in p_theta with weight only on the rewarded items.)"""
    b = X.exact_log_batch()
    Pg = {k: v.clone().requires_grad_(True) for k, v in b["P"].items()}
    values, losses = [], []
    for _ in range(X.LEARNING_STEPS + 1):
        loss, value = X.reference_step(Pg, b)
        values.append(value.item())
        losses.append(loss.item())
        grads = torch.autograd.grad(loss, list(Pg.values()), allow_unused=True)
        with torch.no_grad():
            for p, g in zip(Pg.values(), grads):
                if g is not None:
                    p -= X.LEARNING_RATE * g
    # the objective in closed form at the start: -sum p_theta r / (I p_a)
    L = b["p_x"].shape[1]
    with torch.no_grad():
        items, lg, rew = catalogue.off_policy_rows(tuple(b["p_x"].shape), b["ids"], b["logged"], b["reward"])
        lp, _, _ = X.model_rows(b["P"], b["cfg"], b["attrs"], b["p_x"], b["p_c"], b["n"], items, b["tau"], "profile")
        closed = -float((torch.exp(lp[:, L - 1]) * b["reward"] / torch.exp(b["logged"][:, 0])).mean())
    assert abs(losses[0] - closed) <= 1e-12
    print(f"value {values[0]:.4f} -> {values[-1]:.4f}, objective {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert values[-1] > values[0] + 0.1 and losses[-1] < losses[0]
    assert np.all(np.diff(losses) < 0)
