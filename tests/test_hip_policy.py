"""CARCA.log_prob_items / KNN.log_prob_items and the off-policy estimators over them (csrc/policy_items.h,
policy_items.hip).

What a result is compared with:
  * recommend_sampled, bit for bit: for the ids that call returned, log_prob_items' log_probs are its log_probs
    (torch.equal), under every exclusion, candidate set, temperature and forced row split;
  * itself under every change that must not move a bit: the list permuted, an id listed twice, the user alone, a
    permuted batch, a forced split of the reduce pass (ops.TUNE_RETRIEVE_PARTS);
  * the contract: exactly -inf for every ineligible entry, never NaN, lse = -inf and entropy = 0 with no eligible item;
  * float64: the log-softmax and logsumexp of the float64 oracle's logits at tolerances from sampling_ref.e_bound (the
    form tests/test_hip_sampled.py::test_log_probs uses), the entropy against the call's own log_probs (the reduction's
    arithmetic alone) and against the oracle (through the entropy's gradient);
  * the exact value of a target policy, from a log of 4096 draws: IPS and SNIPS within 4.9 standard deviations, the
    unweighted mean outside (tests/test_policy_host.py shows the band's power from the oracle alone).
Shapes are tests/test_hip_sampled.py's: n_items 33, 257 and 1000 -- one partial 1024-column chunk each -- and 4099 and
9001: 5 and 9 chunks, unequal parts, last chunks of 3 and 809 columns, rows starting at every residue mod 4.  B = 5 with
an empty and a one-slot profile; L = 9."""
import functools

import numpy as np
import pytest
import torch

from carca_replication_amd import CarcaHipError, _lib, catalogue, ops, train
from carca_replication_amd.modules import KNN
from tests import policy_ref as PR
from tests import sampling_ref as R

pytestmark = pytest.mark.gpu

PARTS = (1, 2, 3, 64)
TAUS = (1.0, 0.7)
K = 40
NEG_INF = float("-inf")
ALL_SIZES = R.SIZES + R.BIG_SIZES
CASES = [(g, n) for g in R.GEOS for n in ALL_SIZES]
IDS = [f"{g}-n{n}" for g, n in CASES]
SMALL = [(g, n) for g in R.GEOS for n in R.SIZES]
SMALL_IDS = [f"{g}-n{n}" for g, n in SMALL]


@functools.lru_cache(maxsize=None)
def _case(geo, n, L=R.L, B=R.B, seed=0):
    """-> dict: the model, the device batch, the float64 oracle logits [B, n] -- computed once, shared, never changed."""
    cfg, P, attrs, batch = R.oracle_setup(geo, L, B, n, seed)
    p_x, p_c, ctx = batch
    return dict(geo=geo, n=n, p_x=p_x, model=R.device_model(geo, P, attrs, n, L),
                prof=(p_x.cuda(), None, p_c.float().cuda()), ctx=ctx.float().cuda(),
                oracle=R.oracle_logits(geo, cfg, P, attrs, batch, n).numpy())


class _forced_parts:
    def __init__(self, S):
        self.S = S

    def __enter__(self):
        _lib.check(_lib.load().carca_set_tuning(ops.TUNE_RETRIEVE_PARTS, self.S), "set_tuning")

    def __exit__(self, *exc):
        _lib.load().carca_set_tuning(ops.TUNE_RETRIEVE_PARTS, 0)


def _exclusion_tensor(n, B=R.B):
    """tests/test_hip_sampled.py::test_contract's: everything but 5 .. 41 ids per user (n = 33: 3 .. 5), with zeros and an
    id outside the catalogue -> (the [B, n + 2] int32 tensor, the ids it leaves per user)."""
    keep = [set(list(range(1 + b, n, 7 + b))[:5 + 9 * b]) for b in range(B)]
    extra = torch.zeros(B, n + 2, dtype=torch.int32)
    for b in range(B):
        gone = sorted(set(range(1, n)) - keep[b])
        extra[b, :len(gone)] = torch.tensor(gone, dtype=torch.int32)
        extra[b, -1] = n + 3
    return extra, keep


def _all_ids(n, B=R.B):
    return torch.arange(1, n).expand(B, -1).contiguous().cuda()


def _same3(a, b):
    return len(a) == len(b) == 3 and all(torch.equal(x, y) for x, y in zip(a, b))


def _no_nan(out):
    return not any(bool(torch.isnan(t).any()) for t in out)


# ---- 1. the bits of recommend_sampled ----------------------------------------------------------------------------------
@pytest.mark.parametrize("geo,n", CASES, ids=IDS)
def test_bits_of_recommend_sampled(geo, n):
    c = _case(geo, n)
    model, prof, ctx = c["model"], c["prof"], c["ctx"]
    extra, keep = _exclusion_tensor(n)
    assert any(len(e) < K for e in keep)
    S = catalogue.CandidateSet(torch.arange(2, n, 3).cuda(), n)
    runs = []
    for tau in TAUS:
        for excl in ("profile", None, extra.cuda()):
            for cand in (None, S):
                _, ids, logged = model.recommend_sampled(prof, ctx, k=K, temperature=tau, seed=41, exclude=excl,
                                                         candidates=cand)
                got = model.log_prob_items(prof, ctx, ids, temperature=tau, exclude=excl, candidates=cand)
                assert got[0].shape == (R.B, K) and got[1].shape == got[2].shape == (R.B,)
                assert all(t.dtype == torch.float32 for t in got) and _no_nan(got)
                assert torch.equal(got[0], logged), (tau, type(excl), cand is not None)
                assert torch.equal(got[0] == NEG_INF, ids == 0)  # padding: -inf on both sides, and nowhere else
                runs.append((tau, excl, cand, ids, logged, got))
    assert any(bool((r[3] == 0).any()) for r in runs) and (n <= K or any(bool((r[3] != 0).all()) for r in runs))
    for parts in PARTS:
        with _forced_parts(parts):
            for tau, excl, cand, ids, logged, got in runs:
                again = model.log_prob_items(prof, ctx, ids, temperature=tau, exclude=excl, candidates=cand)
                assert torch.equal(again[0], logged) and _same3(again, got), parts  # (lse and entropy too)
    assert ops.get_tuning(ops.TUNE_RETRIEVE_PARTS) == 0


# ---- 2. ineligible and odd lists ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo,n", CASES, ids=IDS)
def test_ineligible_and_odd_lists(geo, n):
    c = _case(geo, n)
    model, prof, ctx, p_x = c["model"], c["prof"], c["ctx"], c["p_x"]
    members = set(range(2, n, 3))
    S = catalogue.CandidateSet(torch.arange(2, n, 3).cuda(), n)
    # the exclusion tensor: the profile, and two members of S per user
    struck = [[2 + 3 * b, 2 + 3 * ((b + 4) % 9)] for b in range(R.B)]
    excl = torch.cat([p_x, torch.tensor(struck)], 1)
    eligible = [members - set(p_x[b].tolist()) - set(struck[b]) for b in range(R.B)]
    assert all(len(e) >= 2 for e in eligible)
    mask = torch.zeros(R.B, n, dtype=torch.bool)
    for b in range(R.B):
        mask[b, sorted(eligible[b])] = True
    call = lambda items: model.log_prob_items(prof, ctx, items, temperature=0.7, exclude=excl.cuda(), candidates=S)  # noqa: E731
    full = call(torch.arange(n).expand(R.B, -1).contiguous().cuda())  # every id of the catalogue, 0 included
    full_cpu = full[0].cpu()
    assert _no_nan(full) and torch.equal(torch.isfinite(full_cpu), mask)
    assert bool((full_cpu[~mask] == NEG_INF).all()) and bool((full_cpu <= 0).all())
    # one list per user: id 0, a profile id, an id from the exclusion tensor, an id outside candidates, -1, n, n + 3,
    # 2^40, and one eligible id twice
    rows = []
    for b in range(R.B):
        prof_id = int(p_x[b, -1]) if int(p_x[b, -1]) else int(p_x[0, -1])  # (user 1's profile is empty: user 0's id, eligible or not)
        good = sorted(eligible[b])[1]
        rows.append([0, prof_id, struck[b][0], 3, -1, n, n + 3, 2 ** 40, good, good])
    special = torch.tensor(rows, dtype=torch.int64)
    assert 3 not in members
    got = call(special.cuda())
    lp = got[0].cpu()
    assert _no_nan(got) and torch.equal(got[1], full[1]) and torch.equal(got[2], full[2])
    for b in range(R.B):
        dead = [0, 2, 3, 4, 5, 6, 7] + ([1] if int(p_x[b, -1]) else [])
        assert bool((lp[b, dead] == NEG_INF).all()), b
        assert bool(torch.isfinite(lp[b, 8])) and lp[b, 8].view(torch.int32) == lp[b, 9].view(torch.int32), b
        assert lp[b, 8] == full_cpu[b, rows[b][8]], b
    # int32 lists are the same lists
    assert _same3(call(special.clamp(-5, n + 5).to(torch.int32).cuda()), call(special.clamp(-5, n + 5).cuda()))
    # any length: an entry is a lookup -- the id's value in `full`, or -inf outside the catalogue
    g = torch.Generator().manual_seed(n)
    for N in (1, 255, 256, 257):
        items = torch.randint(-2, n + 3, (R.B, N), generator=g)
        items[:, :min(N, 10)] = special[:, :min(N, 10)]
        out = call(items.cuda())
        assert out[0].shape == (R.B, N) and torch.equal(out[1], full[1]) and torch.equal(out[2], full[2])
        inside = (items > 0) & (items < n)
        want = torch.where(inside, full_cpu.gather(1, items.clamp(0, n - 1)), torch.full((R.B, N), NEG_INF))
        assert torch.equal(out[0].cpu(), want), N
        perm = torch.randperm(N, generator=g)
        again = call(items[:, perm].contiguous().cuda())
        assert torch.equal(again[0], out[0][:, perm.cuda()]), N
        assert torch.equal(again[1], out[1]) and torch.equal(again[2], out[2]), N
    # N = 0: an empty [B, 0], lse and entropy as ever
    out = call(torch.zeros(R.B, 0, dtype=torch.int64).cuda())
    assert out[0].shape == (R.B, 0) and out[0].dtype == torch.float32
    assert torch.equal(out[1], full[1]) and torch.equal(out[2], full[2])
    assert bool(torch.isfinite(out[1]).all()) and bool((out[2] >= 0).all())


# ---- 3. batch independence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo,n", CASES, ids=IDS)
def test_batch_independence(geo, n):
    c = _case(geo, n)
    model, prof, ctx = c["model"], c["prof"], c["ctx"]
    g = torch.Generator().manual_seed(n + 1)
    items = torch.randint(0, n, (R.B, 300), generator=g).cuda()
    out = model.log_prob_items(prof, ctx, items, temperature=0.8)
    assert _no_nan(out) and bool(torch.isfinite(out[0]).any())
    for b in range(R.B):
        one = model.log_prob_items(tuple(None if t is None else t[b:b + 1] for t in prof), ctx[b:b + 1], items[b:b + 1],
                                   temperature=0.8)
        assert _same3(one, tuple(t[b:b + 1] for t in out)), b
    perm = torch.tensor([3, 0, 4, 2, 1]).cuda()
    got = model.log_prob_items(tuple(None if t is None else t[perm] for t in prof), ctx[perm], items[perm], temperature=0.8)
    assert _same3(got, tuple(t[perm] for t in out))


# ---- 4. against float64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo,n", SMALL, ids=SMALL_IDS)
def test_against_float64(geo, n):
    """Figures of the first run on an MI355X are in DESIGN.md section 28."""
    c = _case(geo, n)
    e = R.e_bound(geo, c["oracle"][:, 1:])
    for tau in [1.0] + R.order_taus(c["oracle"]):
        lp, lse, _ = (t.cpu().double().numpy() for t in c["model"].log_prob_items(c["prof"], c["ctx"], _all_ids(n),
                                                                                temperature=tau))
        worst = worst_lse = 0.0
        for b in range(R.B):
            el = R.eligible_ids(c["p_x"][b], n)
            want, want_lse, _, _ = PR.policy_stats(c["oracle"][b, el] / tau)
            live = np.zeros(n, dtype=bool)
            live[el] = True
            assert np.isfinite(lp[b][live[1:]]).all() and np.isneginf(lp[b][~live[1:]]).all(), b
            worst = max(worst, float(np.abs(lp[b][el - 1] - want).max()))
            worst_lse = max(worst_lse, abs(lse[b] - want_lse))
            total = float(np.exp(lp[b][el - 1]).sum())  # every eligible item is listed: the probabilities sum to 1
            assert abs(total - 1.0) < 1e-4, (tau, b, total)
        print(f"{geo} n={n} tau={tau:.4g}: max |log_prob - float64| = {worst:.3e} (tolerance {4 * e / tau + 1e-5:.3e}), "
              f"max |lse - float64| = {worst_lse:.3e} (tolerance {2 * e / tau + 1e-5:.3e})")
        assert worst <= 4 * e / tau + 1e-5
        assert worst_lse <= 2 * e / tau + 1e-5


# ---- 5. entropy ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo,n", CASES, ids=IDS)
def test_entropy(geo, n):
    """Against -sum exp(lp) lp in float64 over the call's own log_probs (the reduction's arithmetic alone; tolerance
    policy_ref.entropy_format_tol, from the formats), and against the float64 entropy of the oracle's logits within
    (2 e / tau) E_p|log p + H| -- e = sampling_ref.e_bound, the expectation the 1-norm of the entropy's gradient in z --
    plus that term.  Hot limit: at temperature 1e6 the entropy is log n_eligible.  Figures of the first run on an MI355X
    are in DESIGN.md section 28."""
    c = _case(geo, n)
    e = R.e_bound(geo, c["oracle"][:, 1:])
    worst_own = worst_oracle = worst_hot = 0.0
    for tau in TAUS + (1e6,):
        lp, _, H = (t.cpu().double().numpy() for t in c["model"].log_prob_items(c["prof"], c["ctx"], _all_ids(n),
                                                                              temperature=tau))
        for b in range(R.B):
            el = R.eligible_ids(c["p_x"][b], n)
            fmt = PR.entropy_format_tol(len(el))
            own = abs(H[b] - PR.entropy_of_log_probs(lp[b][el - 1]))
            _, _, want, grad1 = PR.policy_stats(c["oracle"][b, el] / tau)
            vs_oracle, tol = abs(H[b] - want), 2 * e / tau * grad1 + fmt
            if tau == 1e6:
                worst_hot = max(worst_hot, abs(H[b] - np.log(len(el))) / fmt)
                assert abs(H[b] - np.log(len(el))) <= fmt, (b, H[b], np.log(len(el)))
            worst_own, worst_oracle = max(worst_own, own / fmt), max(worst_oracle, vs_oracle / tol)
            assert own <= fmt, (tau, b, own, fmt)
            assert vs_oracle <= tol, (tau, b, vs_oracle, tol)
            assert 0 <= H[b] <= np.log(len(el)) + fmt
    print(f"{geo} n={n}: worst |entropy - own float64| = {worst_own:.3f} of its tolerance, |entropy - oracle| = "
          f"{worst_oracle:.3f} of its tolerance, hot limit {worst_hot:.3f} of its tolerance")


# ---- 6. no eligible item -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ALL_SIZES)
def test_no_eligible_item(n):
    c = _case("dot64x2", n)
    model, prof, ctx = c["model"], c["prof"], c["ctx"]
    items = torch.arange(-1, n + 1).expand(R.B, -1).contiguous().cuda()
    excl = torch.zeros(R.B, n, dtype=torch.int64)
    excl[2] = torch.arange(n)  # every id, for user 2
    out = model.log_prob_items(prof, ctx, items, temperature=0.9, exclude=excl.cuda())
    assert _no_nan(out)
    assert float(out[1][2]) == NEG_INF and float(out[2][2]) == 0.0 and bool((out[0][2] == NEG_INF).all())
    others = [0, 1, 3, 4]
    assert bool(torch.isfinite(out[1][others]).all()) and bool((out[2][others] >= 0).all())
    assert bool(torch.isfinite(out[0][others][:, 2:n + 1]).all())  # (exclude lists only id 0 for them)
    empty = catalogue.CandidateSet(torch.zeros(0, dtype=torch.int64).cuda(), n)
    out = model.log_prob_items(prof, ctx, items, candidates=empty)
    assert _no_nan(out) and bool((out[0] == NEG_INF).all()) and bool((out[1] == NEG_INF).all()) and bool((out[2] == 0).all())
    knn = KNN().cuda()
    knn.register_attr_table(torch.ones(n, 4).cuda())
    out = knn.log_prob_items((c["p_x"].cuda(), None, None), None, items, exclude=excl.cuda(), candidates=empty)
    assert _no_nan(out) and bool((out[0] == NEG_INF).all()) and bool((out[1] == NEG_INF).all()) and bool((out[2] == 0).all())


# ---- 7. KNN ----------------------------------------------------------------------------------------------------------------
def _knn_table(kind, n_items, F):  # tests/test_hip_sampled.py's, restated
    g = torch.Generator().manual_seed(31)
    if kind == "multihot":  # integers: the i8 path
        A = (torch.rand(n_items, F, generator=g) < 0.3).float()
    else:  # multiples of 1/8: every fp32 sum is exact in any order
        A = torch.randint(-8, 9, (n_items, F), generator=g).float() / 8
    A[0] = 0
    return A


@pytest.mark.parametrize("n", ALL_SIZES)
@pytest.mark.parametrize("kind", ["multihot", "float"])
def test_knn(kind, n):
    F, B, L = 37, 5, 3
    A = _knn_table(kind, n, F)
    model = KNN().cuda()
    model.register_attr_table(A.cuda())
    assert (model.int8_table() is not None) == (kind == "multihot")
    g = torch.Generator().manual_seed(32)
    p_x = torch.randint(0, n, (B, L), generator=g)
    p_x[:, -1] = torch.randint(1, n, (B,), generator=g)
    prof = (p_x.cuda(), None, None)
    tau = 0.25 if n <= 1000 else 0.05
    S = catalogue.CandidateSet(torch.arange(1, n, 2)[:4000].cuda(), n)
    logits = (A[p_x[:, -1]].double() @ A.double().T).numpy()
    for cand in (None, S):
        _, ids, logged = model.recommend_sampled(prof, None, k=K, temperature=tau, seed=21, candidates=cand)
        got = model.log_prob_items(prof, None, ids, temperature=tau, candidates=cand)
        assert _no_nan(got) and torch.equal(got[0], logged) and torch.equal(got[0] == NEG_INF, ids == 0)
        for parts in PARTS:
            with _forced_parts(parts):
                assert _same3(model.log_prob_items(prof, None, ids, temperature=tau, candidates=cand), got), parts
        # an id outside the set, a profile id, id 0 and ids outside the catalogue are -inf; lse and entropy against the exact
        # float64 dot products (e = 0: what fp32 keeps of lse at this magnitude, an ulp of the largest |z|)
        odd = torch.tensor([[0, int(p_x[b, -1]), 2, -1, n, 2 ** 40] for b in range(B)]).cuda()
        lp = model.log_prob_items(prof, None, odd, temperature=tau, candidates=cand)[0].cpu()
        dead = [0, 1, 3, 4, 5] + ([2] if cand is not None else [])
        assert bool((lp[:, dead] == NEG_INF).all())
        for b in range(B):
            el = R.eligible_ids(p_x[b], n)
            if cand is not None:
                el = np.intersect1d(el, cand.ids.cpu().numpy())
            _, want_lse, want_H, grad1 = PR.policy_stats(logits[b, el] / tau)
            zmax = np.abs(logits[b, el] / tau).max()
            assert abs(float(got[1][b]) - want_lse) <= 1e-5 + 2.0 ** -22 * zmax, b
            # (z = logit / tau rounds by up to 2^-24 |z| per item: that through the entropy's gradient, plus the formats' term)
            assert abs(float(got[2][b]) - want_H) <= 2.0 ** -24 * zmax * grad1 + PR.entropy_format_tol(len(el)), b
    model.train()  # train and eval mode alike
    assert _same3(model.log_prob_items(prof, None, ids, temperature=tau, candidates=S), got)


# ---- 8. the composed route -------------------------------------------------------------------------------------------------
def test_composed_route():
    c = _case("ca64x4-all", 257, L=65, B=3)
    model, prof, ctx = c["model"], c["prof"], c["ctx"]
    _, ids, logged = model.recommend_sampled(prof, ctx, k=K, temperature=0.5, seed=1, allow_composed=True)
    with pytest.raises(CarcaHipError, match="^log_prob_items: "):
        model.log_prob_items(prof, ctx, ids, temperature=0.5)
    got = model.log_prob_items(prof, ctx, ids, temperature=0.5, allow_composed=True)
    assert _no_nan(got) and torch.equal(got[0], logged) and bool(torch.isfinite(got[0]).all())


# ---- 9. errors -------------------------------------------------------------------------------------------------------------
def test_errors_name_the_call_and_come_before_any_launch(monkeypatch):
    c = _case("ca64x4-all", 33)
    model, prof, ctx = c["model"], c["prof"], c["ctx"]
    items = _all_ids(33)

    def launched(*a, **kw):
        raise AssertionError("the model side ran before the arguments were checked")

    real = catalogue.carca_model_side
    monkeypatch.setattr(catalogue, "carca_model_side", launched)
    for t in (0, 0.0, -1.0, float("nan"), 1e-40, True):
        with pytest.raises(CarcaHipError, match="^log_prob_items: temperature must be a finite float > 0"):
            model.log_prob_items(prof, ctx, items, temperature=t)
    for bad in (items.float(), items[:3], items[0]):  # float items; the wrong leading dimension; one dimension
        with pytest.raises(CarcaHipError, match=r"^log_prob_items: items must be an int \[B, N\] tensor"):
            model.log_prob_items(prof, ctx, bad)
    model.train()
    try:
        with pytest.raises(CarcaHipError, match="^log_prob_items: the model is in training mode"):
            model.log_prob_items(prof, ctx, items)
    finally:
        model.eval()
    monkeypatch.setattr(catalogue, "carca_model_side", real)

    class Other(torch.nn.Module):  # a decoder the catalogue calls do not cover
        score_groups = None

    decoder = model.decoder
    model.decoder = Other()
    try:
        with pytest.raises(CarcaHipError, match="^log_prob_items: decoder Other is not covered"):
            model.log_prob_items(prof, ctx, items)
    finally:
        model.decoder = decoder
    groups = catalogue.ItemGroups(torch.arange(33).cuda() % 3)  # the grouped forms are not part of the call
    with pytest.raises(CarcaHipError, match="^log_prob_items: candidates must be None, a CandidateSet or"):
        model.log_prob_items(prof, ctx, items, candidates=groups)
    assert _no_nan(model.log_prob_items(prof, ctx, items))  # and the model still serves


# ---- 10. end to end --------------------------------------------------------------------------------------------------------
def test_off_policy_estimate_recovers_the_target_policys_value():
    """A log of 4096 first draws under temperature tau_A, rewards r(i) = 1 where the item's oracle logit is above the
    eligible median.  (a) The logging policy as its own target: bits, ratios exactly 0, IPS = SNIPS = the mean reward.
    (b) The target at tau_A / 2: IPS and SNIPS within 4.9 sd + 1e-3 of the exact V_B = sum p_B r (float64, from the oracle;
    4.9 standard deviations is the two-sided 1e-6 level), the unweighted mean outside that band."""
    e = PR.e2e_inputs()
    rows, n = PR.ROWS, R.DIST["n"]
    model = R.device_model(e["geo"], e["P"], e["attrs"], n, R.DIST["L"])
    p_x, p_c, ctx = e["batch"]
    prof = (p_x.expand(rows, -1).contiguous().cuda(), None, p_c.float().expand(rows, -1, -1).contiguous().cuda())
    ctx = ctx.float().expand(rows, -1).contiguous().cuda()
    _, ids, logged = model.recommend_sampled(prof, ctx, k=1, temperature=e["tau_a"], seed=R.DIST["seed"],
                                             user_keys=torch.arange(rows).cuda())
    by_id = torch.zeros(n, dtype=torch.float64)
    by_id[torch.from_numpy(e["ids"])] = torch.from_numpy(e["reward"])
    rewards = by_id.cuda()[ids[:, 0]]
    naive = float(rewards.mean())
    assert bool((ids != 0).all()) and len(torch.unique(ids)) > 10
    # (a) the logging policy
    target = model.log_prob_items(prof, ctx, ids, temperature=e["tau_a"])[0]
    assert torch.equal(target, logged)
    ratio = catalogue.policy_log_ratio(target, logged)
    assert bool((ratio == 0).all())
    est = catalogue.off_policy_estimate(ratio, rewards)
    assert float(est["ips"]) == float(est["snips"]) == naive and float(est["ess"]) == rows and float(est["n"]) == rows
    # (b) the colder target
    target = model.log_prob_items(prof, ctx, ids, temperature=e["tau_b"])[0]
    ratio = catalogue.policy_log_ratio(target, logged)
    est = catalogue.off_policy_estimate(ratio, rewards)
    ips, snips = float(est["ips"]), float(est["snips"])
    print(f"V_A = {e['v_a']:.4f}, V_B = {e['v_b']:.4f}, band {e['band']:.4f}: IPS {ips:.4f}, SNIPS {snips:.4f}, "
          f"unweighted mean {naive:.4f}, ESS {float(est['ess']):.0f}, largest weight {float(est['max_weight']):.3f}")
    assert abs(ips - e["v_b"]) <= e["band"]
    assert abs(snips - e["v_b"]) <= e["band"]
    assert abs(naive - e["v_b"]) > e["band"]  # (the band cannot hide an estimator that ignores its weights)
    assert float(est["max_weight"]) == pytest.approx(e["w"].max(), abs=1e-3)
    # the whole path over the same log in four batches
    q = rows // 4
    logs = [((prof[0][s:s + q], None, prof[2][s:s + q]), ctx[s:s + q], ids[s:s + q], logged[s:s + q], rewards[s:s + q])
            for s in range(0, rows, q)]
    got = train.off_policy_value(model, logs, "cuda", temperature=e["tau_b"])
    for k in ("ips", "snips", "ess", "max_weight"):
        assert got[k] == pytest.approx(float(est[k]), rel=1e-12), k
    assert got["n"] == rows and got["clip"] is None
    two = [(p, c_, i, l, r.reshape(-1, 1)) for p, c_, i, l, r in logs]  # rewards [B, k]: column 0 for "first"
    assert train.off_policy_value(model, two, "cuda", temperature=e["tau_b"])["ips"] == got["ips"]


def test_reduce_pass_alone_against_the_perturb_pass():
    """carca_policy_reduce and carca_sampled_perturb over one buffer (tests/test_hip_sampled.py's: 3 rows of 4099 columns, a
    tenth of them and one whole chunk excluded): the reduce pass's (max, sum) are the perturb pass's bits, the buffer is only
    read, and the entropy partial is sum exp(z - max) (max - z) over the chunk."""
    import ctypes as C

    B, n, tau = 3, 4099, 0.7
    g = torch.Generator().manual_seed(8)
    raw = (torch.randn(B, n, generator=g) * 4).float()
    gone = torch.rand(B, n, generator=g) < 0.1
    gone[:, 0] = True
    gone[1, 1024:2048] = True
    raw.view(torch.int32)[gone] = -1
    logits = raw.cuda()
    pert, part2, part3 = torch.zeros_like(logits), torch.zeros(B, 5, 2).cuda(), torch.zeros(B, 5, 3).cuda()
    X = _lib.Sampling(temperature=tau, seed=1)
    lib = _lib.load()
    _lib.check(lib.carca_sampled_perturb(logits.data_ptr(), pert.data_ptr(), part2.data_ptr(), B, n, C.byref(X),
                                         ops._stream()), "sampled_perturb")
    outs = []
    for parts in (0, 1, 2, 64):
        part3.zero_()
        with _forced_parts(parts):
            _lib.check(lib.carca_policy_reduce(logits.data_ptr(), part3.data_ptr(), B, n, tau, ops._stream()), "policy_reduce")
        outs.append(part3.cpu())
    assert all(torch.equal(o.view(torch.int32), outs[0].view(torch.int32)) for o in outs)
    assert torch.equal(logits.cpu().view(torch.int32), raw.view(torch.int32))
    assert torch.equal(outs[0][:, :, :2].contiguous().view(torch.int32), part2.cpu().view(torch.int32))
    z = (raw.numpy() / np.float32(tau)).astype(np.float32).astype(np.float64)
    live = ~gone.numpy()
    for b in range(B):
        for c in range(5):
            cols = np.arange(c * 1024, min(n, (c + 1) * 1024))
            zc = z[b, cols][live[b, cols]]
            if zc.size == 0:
                assert float(outs[0][b, c, 1]) == 0 and float(outs[0][b, c, 2]) == 0
                continue
            want = (np.exp(zc - zc.max()) * (zc.max() - zc)).sum()
            # (the exp2 argument, up to 32, rounds by 2^-20: 2^-20 log 2 = 6.6e-7 relative per term; the conversions 2^-24
            # each; the truncation of 1024 terms to units of 2^-32, 2.4e-7 absolute)
            assert abs(float(outs[0][b, c, 2]) - want) <= 1e-6 * want + 3e-7, (b, c)
