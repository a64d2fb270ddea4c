"""The four kernels of csrc/loss_metrics.hip -- bce_kernel (register arm n <= 16384, loop arm above), rank_kernel,
rank_ordered_kernel (deterministic mode) and eval_metrics_kernel (fast arm N <= 128 and B <= 192, general arm) -- called
one by one through ops.bce_fwd / ops.rank_metrics / ops.eval_metrics and through their callers (BinaryCrossEntropy,
engine.eval_batch, train.compute_HR / compute_NDCG / evaluate), against plain torch statements on the CPU.

References and bounds (none derived from the code under test):
  * ranks, HR, ties: counts over the fp32 scores themselves with the order of DESIGN.md section 1a (`>` and `==` on
    numbers; NaN above every number and equal to NaN).  Comparisons are exact, so these are compared exactly.  CPU tests
    show that the count form equals the reference's sort formula (train.py:15-32) on tie-free inputs and on rows with
    NaN candidates and a finite positive.
  * NDCG: the float64 sum of 1 / log2(rank + 2) over the reference ranks.  Each fp32 term is within 4 ulp (one log2f, one
    divide); m non-negative terms added in any order err by at most (m - 1) eps32 / 2 of their sum; so
    |got - ref64| <= (4 + B / 2) eps32 ref64 with B the users behind the sum.  One rank off by one inside the top k moves
    the sum by at least 1/log2(k+1) - 1/log2(k+2) (1.0e-2 at k = 10): orders of magnitude above the bound at every B here.
  * BCE loss: ref64 = the statement (per * mask).sum() / count in float64 on the same fp32 inputs, ref32 = the same
    statement in torch float32; err <= 8 |ref32 - ref64| + 4 eps32 |ref64| (the rule of tests/test_hip_row_kernels.py).
    Loop arm only, and only when that rule is exceeded: (ceil(n / 1024) + 14) eps32 / 2 * sum|term mask| / count, the depth
    of the chain of non-negative adds in a 1024-thread block.
  * BCE gradient: element by element, |got_i - ref64_i| <= 8 |ref32_i - ref64_i| + 4 eps32 |ref64_i| with ref64 / ref32
    from torch.autograd of the statement; masked entries exactly 0.  The 1 / count factor makes this a check of the mask
    count too (one element off in 40000 is 2.5e-5 relative).
  * one live element: the loss is that element's term within 4 eps32 (p = 0.25 / 0.75: p + eps rounds to p and |log| is
    1.39, so the argument's rounding is 0.03 eps32 of the term and logf's own error is what is measured).

Largest figures of one MI355X run (loss: err / max(noise, eps32 |ref64| / 2); gradient: the largest element's
err / max(noise_i, eps32 |ref64_i| / 2); NDCG: err / bound):
    bce_kernel, register arm    loss 2.00   gradient 2.83   one live element 0.07 of its 4 eps32
    bce_kernel, loop arm        loss 2.25   gradient 2.94   one live element 0.07   (the depth bound was never needed)
    BinaryCrossEntropy module   loss 1.00 / 0.73   gradient 2.34 / 3.38 (register / loop arm; upstream gradient 2.5)
    eval_metrics_kernel         loss 1.64 (fast arm) 1.69 (general arm)   NDCG 0.093 / 0.081 of the bound
    rank_kernel                 NDCG 0.18 .. 0.19 of the bound (atomics: varies by run)   rank_ordered_kernel 0.176
    engine.eval_batch           loss 1.00 / 1.96 / 0.84   NDCG 0.010 / 0.033 / < 0.001 (one launch / int64 ids / > 16384)
    train.compute_NDCG 0.06 .. 0.16 (rank_kernel's atomics)   train.evaluate NDCG 0.005, loss 0.063 of their bounds
Ranks, HR, ties, masked gradients and the untouched sentinels were exact everywhere.
Findings:
  * NaN scores (found by reading the kernels, before any run): every count was `v > y0` / `v == y0`, both false for NaN,
    so a NaN candidate never outranked the positive and a NaN positive had rank 0 with no ties -- a partly diverged
    model evaluated better than under the reference's torch.sort, which puts NaN first.  All four rank paths now count
    with NaN above every number and equal to NaN (rank_count / rank_count_wave in csrc/loss_metrics.hip); the NaN tests
    here fail on the old counts in all four paths.
  * ops.rank_metrics(pos=...) with a pos of fewer than B entries let the kernel read past its end; ops.py now refuses
    a pos whose element count is not B (and a pos that is not on the device) before any launch.
  * The first MI355X run of this file found nothing else: all seven arms were inside their bounds at every size above.
"""
import functools
import math

import pytest
import torch

from oracle import carca_oracle as O

gpu = pytest.mark.gpu
EPS32 = float(torch.finfo(torch.float32).eps)
BCE_EPS = float(torch.tensor(1e-8, dtype=torch.float32))  # the eps the kernels see (a C float)
SENTINEL = -12345.5
NAN, INF = float("nan"), float("inf")
REGISTER_MAX = 16384  # bce_kernel: elements held in registers; eval_metrics: the largest batch


# --------------------------------------------------------------------------------------------------
# references (plain torch on the CPU)
# --------------------------------------------------------------------------------------------------
def ref_counts(y, pos=None):
    """(rank [B], ties [B]) int64: the other columns that rank above / equal the positive; NaN above every number, equal
    to NaN."""
    B, N = y.shape
    pc = torch.zeros(B, dtype=torch.int64) if pos is None else pos.reshape(-1).to(torch.int64)
    y0 = y.gather(1, pc.view(-1, 1))
    other = torch.arange(N).view(1, -1) != pc.view(-1, 1)
    vn, yn = torch.isnan(y), torch.isnan(y0)
    gt = (y > y0) | (vn & ~yn)
    eq = (y == y0) | (vn & yn)
    return (gt & other).sum(1), (eq & other).sum(1)


def ref_metrics(y, k, pos=None):
    """(rank [B], HR sum, NDCG sum in float64, ties sum)"""
    rank, ties = ref_counts(y, pos)
    hit = rank < k
    ndcg = float((hit.double() / torch.log2(rank.double() + 2.0)).sum())
    return rank, int(hit.sum()), ndcg, int(ties.sum())


def sort_hr(y_pred, y_true, k):
    """train.py:15-21"""
    _, idxs = torch.sort(y_pred, descending=True)
    y_true_sort = torch.gather(y_true, dim=1, index=idxs)
    top_k = y_true_sort[:, :k]
    return torch.sum(top_k).item()


def sort_ndcg(y_pred, y_true, k, dtype=torch.float32):
    """train.py:24-32 (the reference's log2 of an int64 tensor gives float32; float64 for a reference value)"""
    _, idxs = torch.sort(y_pred, descending=True)
    y_true_sort = torch.gather(y_true, dim=1, index=idxs)
    top_k = y_true_sort[:, :k]
    ranks = torch.nonzero(top_k)[:, 1]
    scores = 1.0 / torch.log2((ranks + 2).to(dtype))
    return torch.sum(scores).item()


def ndcg_bound(ref64, users):
    return (4.0 + users / 2.0) * EPS32 * ref64


def bce_statement(y, y_true, mask, denom=None):
    """carca.py:441-444; dtype follows the inputs"""
    per = -(y_true * torch.log(y + BCE_EPS) + (1.0 - y_true) * torch.log(1.0 - y + BCE_EPS))
    return (per * mask).sum() / (mask.sum() if denom is None else denom)


def bce_refs(y, y_true, mask, denom=None, want_grad=False):
    """{loss64, loss32, abs64 = sum|term mask| / count, and with want_grad g64, g32} of fp32 y, 0/1 y_true and mask"""
    out = {}
    for name, dt in (("64", torch.float64), ("32", torch.float32)):
        yy = y.to(dt).clone().requires_grad_(want_grad)
        loss = bce_statement(yy, y_true.to(dt), mask.to(dt), denom)
        out["loss" + name] = loss.detach()
        if want_grad:
            (g,) = torch.autograd.grad(loss, yy)
            out["g" + name] = g
    y64, t64, m64 = y.double(), y_true.double(), mask.double()
    per = -(t64 * torch.log(y64 + BCE_EPS) + (1.0 - t64) * torch.log(1.0 - y64 + BCE_EPS))
    out["abs64"] = float((per * m64).abs().sum() / (m64.sum() if denom is None else denom))
    return out


_RATIOS = {}


def _note(key, value):
    _RATIOS[key] = max(_RATIOS.get(key, 0.0), value)


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    for key in sorted(_RATIOS):
        print(f"\nmax ratio  {key:<40} {_RATIOS[key]:.3f}", end="")
    print()


def check_loss(arm, got, refs, n, what=""):
    """The loss rule; `arm` names the kernel arm for the report."""
    got = float(got)
    ref64, ref32 = float(refs["loss64"]), float(refs["loss32"])
    assert math.isfinite(got), f"{arm} {what}: loss {got}"
    err, noise, floor = abs(got - ref64), abs(ref32 - ref64), 4 * EPS32 * abs(ref64)
    ratio = err / max(noise, floor / 8) if max(noise, floor) > 0 else (0.0 if err == 0 else math.inf)
    print(f"{arm} {what}: loss err {err:.3e} noise {noise:.3e} ratio {ratio:.2f} err/bound {err / max(8 * noise + floor, 1e-300):.3f}")
    if err > 8 * noise + floor and n > REGISTER_MAX:
        # the loop arm's one fallback: the depth of its chain of non-negative adds, nothing measured
        depth = (math.ceil(n / 1024) + 14) * EPS32 / 2 * refs["abs64"]
        print(f"{arm} {what}: over the rule, summation-depth bound {depth:.3e}, err/depth {err / depth:.3f}")
        _note(arm + " loss err/depth-bound", err / depth)
        assert err <= depth, f"{arm} {what}: err {err:.3e} > rule {8 * noise + floor:.3e} and > depth bound {depth:.3e}"
        return
    _note(arm + " loss err/noise", ratio)
    assert err <= 8 * noise + floor, f"{arm} {what}: loss err {err:.3e} > 8 * {noise:.3e} + {floor:.3e}"


def check_grad(arm, dy, refs, mask, what="", scale=1.0):
    """The element-wise gradient rule; scale: an upstream gradient both references are multiplied by."""
    assert dy.dtype == torch.float32
    got = dy.detach().reshape(-1).double().cpu()
    g64, g32 = refs["g64"].reshape(-1) * scale, (refs["g32"].reshape(-1) * scale).double()
    assert bool(torch.isfinite(got).all()), f"{arm} {what}: non-finite gradient"
    dead = mask.reshape(-1) == 0
    assert bool((got[dead] == 0).all()), f"{arm} {what}: a masked entry has a gradient"
    err, noise, floor = (got - g64).abs(), (g32 - g64).abs(), 4 * EPS32 * g64.abs()
    live = ~dead
    if bool(live.any()):
        ratio = float((err[live] / torch.maximum(noise[live], floor[live] / 8).clamp_min(1e-300)).max())
        _note(arm + " grad err/noise", ratio)
        print(f"{arm} {what}: grad max element ratio {ratio:.2f}")
    bad = err > 8 * noise + floor
    assert not bool(bad.any()), (f"{arm} {what}: {int(bad.sum())} elements over the rule, first at {int(bad.nonzero()[0])}: "
                                 f"got {float(got[bad][0]):.9e} ref64 {float(g64[bad][0]):.9e}")


def check_rank_sums(arm, got, y, k, pos=None, base=(0.0, 0.0, 0.0), what=""):
    """got: the three sums on the CPU after ONE call on y that started from `base` (exactly representable values)."""
    _, hr, ndcg, ties = ref_metrics(y, k, pos)
    B = y.shape[0]
    assert float(got[0]) == base[0] + hr, f"{arm} {what}: HR {float(got[0])} != {base[0]} + {hr}"
    assert float(got[2]) == base[2] + ties, f"{arm} {what}: ties {float(got[2])} != {base[2]} + {ties}"
    # a pre-filled sum is one more non-negative term of the chain
    users = B + (1 if base[1] != 0 else 0)
    want = base[1] + ndcg
    bound = ndcg_bound(want, users)
    err = abs(float(got[1]) - want)
    if bound > 0:
        _note(arm + " NDCG err/bound", err / bound)
    assert err <= bound, f"{arm} {what}: NDCG {float(got[1])!r} vs {want!r}: err {err:.3e} > bound {bound:.3e}"


def _ops():
    from carca_replication_amd import ops
    from carca_replication_amd._lib import CarcaHipError
    return ops, CarcaHipError


def tie_free(B, N, g):
    """[B, N] scores in (0, 1): every row a random permutation of N distinct values, so no ties by construction"""
    vals = (torch.arange(N, dtype=torch.float32) + 1.0) / (N + 1.0)
    return torch.stack([vals[torch.randperm(N, generator=g)] for _ in range(B)])


def one_hot_true(B, N, cols):
    y_true = torch.zeros(B, N)
    y_true[torch.arange(B), cols] = 1.0
    return y_true


def nan_rows(N, k):
    """Five rows of N >= 2 k + 56 scores with the positive in column 0 and NaNs on both sides of column 64:
    k - 1 NaN candidates and the best number (rank k - 1, a hit), k NaN candidates (rank k, a miss), one NaN at the last
    column (rank 1), a NaN positive among three NaN candidates (rank 0, 3 ties), an all-NaN row (rank 0, N - 1 ties)."""
    y = torch.linspace(0.1, 0.6, N).repeat(5, 1)
    y[:, 0] = 0.9
    cols = [1 + (j * 7) % 16 + (54 if j % 2 else 0) for j in range(k)]  # distinct columns in 1..16 and 55..70
    assert len(set(cols)) == k
    y[0, cols[:k - 1]] = NAN
    y[1, cols] = NAN
    y[2, N - 1] = NAN
    y[3, 0] = NAN
    y[3, [1, 64, N - 1]] = NAN
    y[4, :] = NAN
    want_rank = torch.tensor([k - 1, k, 1, 0, 0])
    want_ties = torch.tensor([0, 0, 0, 3, N - 1])
    return y, want_rank, want_ties


# --------------------------------------------------------------------------------------------------
# CPU: the count form against the reference's sort formula
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", [(1, 1), (3, 2), (17, 65), (33, 101), (8, 1001)])
def test_count_form_equals_the_sort_formula_on_tie_free_scores(B, N):
    g = torch.Generator().manual_seed(100 * B + N)
    y = tie_free(B, N, g)
    cols = torch.randint(0, N, (B,), generator=g)
    y_true = one_hot_true(B, N, cols)
    rank, ties = ref_counts(y, cols)
    assert int(ties.sum()) == 0
    order = torch.argsort(y, dim=1, descending=True)
    assert torch.equal(rank, (order == cols.view(-1, 1)).int().argmax(1))
    for k in sorted({1, 10, max(N - 1, 1), N, N + 5}):
        _, hr, ndcg, _ = ref_metrics(y, k, cols)
        assert hr == sort_hr(y, y_true, k)
        assert abs(ndcg - sort_ndcg(y, y_true, k, torch.float64)) <= 1e-12 * max(ndcg, 1.0)
        assert abs(ndcg - sort_ndcg(y, y_true, k)) <= ndcg_bound(ndcg, B)  # (the reference's own fp32 sum)


def test_count_form_equals_the_sort_formula_with_nan_candidates():
    """torch.sort(descending=True) puts NaN first: a finite positive ranks below every NaN candidate."""
    k = 10
    for N in (101, 193):
        y, want_rank, want_ties = nan_rows(N, k)
        rank, ties = ref_counts(y)
        assert torch.equal(rank, want_rank) and torch.equal(ties, want_ties)
        fin = y[:3]  # the rows with a finite positive
        y_true = one_hot_true(3, N, torch.zeros(3, dtype=torch.int64))
        for kk in (1, 2, k - 1, k, k + 1, N):
            _, hr, ndcg, _ = ref_metrics(fin, kk)
            assert hr == sort_hr(fin, y_true, kk), kk
            assert abs(ndcg - sort_ndcg(fin, y_true, kk, torch.float64)) <= 1e-12
        # a positive elsewhere, NaN candidates on both sides of it
        g = torch.Generator().manual_seed(N)
        z = tie_free(6, N, g)
        cols = torch.tensor([0, 5, 63, 64, N - 2, N - 1])
        for u in range(6):
            idx = torch.randperm(N, generator=g)[:u + 8]
            z[u, idx[idx != cols[u]]] = NAN
        zt = one_hot_true(6, N, cols)
        for kk in (1, 8, 12, N):
            _, hr, ndcg, _ = ref_metrics(z, kk, cols)
            assert hr == sort_hr(z, zt, kk), kk
            assert abs(ndcg - sort_ndcg(z, zt, kk, torch.float64)) <= 1e-12


def test_bce_statement_equals_the_oracle():
    g = torch.Generator().manual_seed(2)
    y = torch.rand(300, generator=g, dtype=torch.float64)
    t = (torch.rand(300, generator=g) < 0.5).double()
    m = (torch.rand(300, generator=g) < 0.7).double()
    assert abs(float(bce_statement(y, t, m)) - float(O.bce_loss(y, t, m, BCE_EPS))) <= 1e-14
    assert math.isnan(float(bce_statement(y, t, torch.zeros_like(m))))


# --------------------------------------------------------------------------------------------------
# bce_fwd
# --------------------------------------------------------------------------------------------------
SPECIALS = [(0.0, 0), (0.0, 1), (1.0, 0), (1.0, 1), (1.0 - 2.0 ** -24, 0), (1.0 - 2.0 ** -24, 1), (1e-30, 0), (1e-30, 1),
            (float(torch.sigmoid(torch.tensor(40.0))), 0), (float(torch.sigmoid(torch.tensor(40.0))), 1),
            (float(torch.sigmoid(torch.tensor(-40.0))), 0), (float(torch.sigmoid(torch.tensor(-40.0))), 1)]


@functools.lru_cache(maxsize=None)
def bce_inputs(n):
    """(y fp32, y_true 0/1 int32, ids int32) of n elements, about 70 % live, mostly p in (0.01, 0.99), the saturated
    values of SPECIALS at random live places where n has room for them"""
    g = torch.Generator().manual_seed(n)
    y = torch.rand(n, generator=g) * 0.98 + 0.01
    y_true = (torch.rand(n, generator=g) < 0.5).int()
    ids = (torch.rand(n, generator=g) < 0.7).int() * torch.randint(1, 90, (n,), generator=g).int()
    if n >= 63:
        at = torch.randperm(n, generator=g)[:len(SPECIALS)]
        for i, (p, t) in zip(at.tolist(), SPECIALS):
            y[i], y_true[i], ids[i] = p, t, 3
    if int((ids != 0).sum()) == 0:
        ids[0] = 5
    return y, y_true, ids


def bce_arm(n):
    return "bce register arm" if n <= REGISTER_MAX else "bce loop arm"


BCE_SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 16383, 16384, 16385, 20000, 40000]


@gpu
@pytest.mark.parametrize("n", BCE_SIZES, ids=[f"n{n}-{'register' if n <= REGISTER_MAX else 'loop'}_arm" for n in BCE_SIZES])
def test_bce_fwd_loss_and_gradient_against_float64(n):
    ops, _ = _ops()
    y, y_true, ids = bce_inputs(n)
    mask = (ids != 0).float()
    count = float(mask.sum())
    yd, td, idd = y.cuda(), y_true.cuda(), ids.cuda()
    for denom in (None, 3.0 * count, 17.0):
        refs = bce_refs(y, y_true.float(), mask, denom, want_grad=True)
        dt = None if denom is None else torch.tensor([denom], dtype=torch.float32, device="cuda")
        loss, dy = ops.bce_fwd(yd, td, idd, 1e-8, want_grad=True, denom=dt)
        loss0, none = ops.bce_fwd(yd, td, idd, 1e-8, want_grad=False, denom=dt)
        assert none is None and dy.shape == y.shape
        what = f"n={n} denom={denom}"
        check_loss(bce_arm(n), loss, refs, n, what)
        assert float(loss0) == float(loss), f"{what}: the loss depends on want_grad"
        check_grad(bce_arm(n), dy, refs, mask, what)


ONE_HOT = [(n, i) for n in (2048, REGISTER_MAX, 20000) for i in (0, 1, 1023, 1024, 2047, 16383, n - 1) if i < n]


@gpu
@pytest.mark.parametrize("n", [2048, REGISTER_MAX, 20000],
                         ids=["n2048-register_arm", "n16384-register_arm", "n20000-loop_arm"])
def test_bce_fwd_one_live_element(n):
    """A dropped, doubled or misindexed element that a mean over thousands would hide."""
    ops, _ = _ops()
    y, y_true, _ = bce_inputs(n)
    yd, td = y.cuda(), y_true.cuda()
    for i in sorted({i for (m, i) in ONE_HOT if m == n}):
        p, t = (0.25, 1) if i % 2 == 0 else (0.75, 0)
        yy, tt = yd.clone(), td.clone()
        yy[i], tt[i] = p, t
        ids = torch.zeros(n, dtype=torch.int32, device="cuda")
        ids[i] = 9
        loss, dy = ops.bce_fwd(yy, tt, ids, 1e-8, want_grad=True)
        term = -math.log(0.25 + BCE_EPS)  # both choices: the live logarithm's argument is 0.25 + eps
        err = abs(float(loss) - term)
        _note(bce_arm(n) + " one live element, loss err/(4 eps32 term)", err / (4 * EPS32 * term))
        assert err <= 4 * EPS32 * term, f"n={n} i={i}: loss {float(loss)!r} vs {term!r}"
        dy = dy.cpu()
        assert dy.nonzero().reshape(-1).tolist() == [i], f"n={n} i={i}: dy is nonzero at {dy.nonzero().reshape(-1).tolist()[:8]}"
        want = (-1.0 if t else 1.0) / (0.25 + BCE_EPS)
        assert abs(float(dy[i]) - want) <= 4 * EPS32 * abs(want), f"n={n} i={i}: dy {float(dy[i])!r} vs {want!r}"


@gpu
@pytest.mark.parametrize("n", [700, 20000], ids=["n700-register_arm", "n20000-loop_arm"])
def test_bce_fwd_all_masked_is_nan(n):
    ops, _ = _ops()
    y, y_true, _ = bce_inputs(n)
    assert math.isnan(float(bce_statement(y.double(), y_true.double(), torch.zeros(n, dtype=torch.float64))))
    loss, _ = ops.bce_fwd(y.cuda(), y_true.cuda(), torch.zeros(n, dtype=torch.int32, device="cuda"), 1e-8, want_grad=True)
    assert math.isnan(float(loss))


@gpu
@pytest.mark.parametrize("B,N", [(7, 100), (170, 101)], ids=["B7xN100-register_arm", "B170xN101-loop_arm"])
def test_binary_cross_entropy_module(B, N):
    """BinaryCrossEntropy with requires_grad (autograd._BceFn) and without; float mask, bool mask, int32 ids through
    bce_with_grad(ids=); an upstream gradient of 2.5 (one more rounding, inside the 4 eps32 of the rule)."""
    from carca_replication_amd import autograd
    from carca_replication_amd import modules as M

    n = B * N
    y, y_true, ids = (t.view(B, N) for t in bce_inputs(n))
    mask = (ids != 0).float()
    refs = bce_refs(y, y_true.float(), mask, None, want_grad=True)
    arm = bce_arm(n) + " (module)"
    yd, td, idd = y.cuda(), y_true.float().cuda(), ids.cuda()
    loss_fn = M.BinaryCrossEntropy()
    for name, m in (("float mask", M.get_mask(idd)), ("bool mask", idd != 0)):
        with torch.no_grad():
            plain = loss_fn(yd, td, m)
        check_loss(arm, plain, refs, n, name)
        yr = yd.clone().requires_grad_(True)
        loss = loss_fn(yr, td, m)
        assert loss.requires_grad and float(loss.detach()) == float(plain)
        (loss * 2.5).backward()
        assert yr.grad.shape == (B, N)
        check_grad(arm, yr.grad, refs, mask, name, scale=2.5)
    yr = yd.clone().requires_grad_(True)
    loss = autograd.bce_with_grad(yr, td, None, 1e-8, ids=idd)
    check_loss(arm, loss.detach(), refs, n, "ids")
    (loss * 2.5).backward()
    check_grad(arm, yr.grad, refs, mask, "ids", scale=2.5)


# --------------------------------------------------------------------------------------------------
# rank_metrics: rank_kernel (default) and rank_ordered_kernel (deterministic mode)
# --------------------------------------------------------------------------------------------------
@pytest.fixture(params=[False, True], ids=["rank_kernel", "rank_ordered_kernel"])
def mode(request):
    ops, _ = _ops()
    ops.set_deterministic(request.param)
    yield "rank_ordered_kernel" if request.param else "rank_kernel"
    ops.set_deterministic(False)


def run_rank(ops, y, k, pos=None, base=None):
    """(sums [3] on the CPU, rank [B] int64 on the CPU) of one call"""
    sums = None if base is None else torch.tensor(base, dtype=torch.float32, device="cuda")
    p = None if pos is None else pos.cuda()
    sums, rank = ops.rank_metrics(y if y.is_cuda else y.cuda(), k, sums=sums, want_rank=True, pos=p)
    assert rank.dtype == torch.int32 and rank.shape == (y.shape[0],)
    return sums.cpu(), rank.cpu().long()


RANK_B = [1, 3, 4, 5, 16, 17, 33, 300]
RANK_N = [1, 2, 64, 65, 66, 128, 129, 193, 1001]


@gpu
def test_rank_metrics_shapes(mode):
    ops, _ = _ops()
    g = torch.Generator().manual_seed(11)
    for B in RANK_B:
        for N in RANK_N:
            y = torch.rand(B, N, generator=g)
            yd = y.cuda()
            want_rank, _ = ref_counts(y)
            for k in sorted({k for k in (1, 10, N - 1, N, N + 5) if k >= 1}):
                sums, rank = run_rank(ops, yd, k)
                assert torch.equal(rank, want_rank), f"{mode} B={B} N={N}: ranks differ"
                check_rank_sums(mode, sums, y, k, what=f"B={B} N={N} k={k}")


@gpu
@pytest.mark.parametrize("N", [66, 130, 193])
def test_rank_metrics_column_sweep(mode, N):
    """User u has exactly one candidate above its positive, at column u + 1: no column can be dropped unnoticed."""
    ops, _ = _ops()
    B = N - 1
    g = torch.Generator().manual_seed(N)
    y = torch.rand(B, N, generator=g) * 0.4
    y[:, 0] = 0.5
    y[torch.arange(B), torch.arange(B) + 1] = 0.9
    yd = y.cuda()
    sums, rank = run_rank(ops, yd, 1)
    assert torch.equal(rank, torch.ones(B, dtype=torch.int64))
    assert sums.tolist() == [0.0, 0.0, 0.0]
    sums, rank = run_rank(ops, yd, 2)
    assert float(sums[0]) == B and float(sums[2]) == 0
    check_rank_sums(mode, sums, y, 2, what=f"sweep N={N}")


@gpu
@pytest.mark.parametrize("N,k", [(12, 10), (101, 10), (193, 70)])
def test_rank_metrics_constructed_ranks(mode, N, k):
    ops, _ = _ops()
    g = torch.Generator().manual_seed(N + k)
    want = [0, k - 1, k, N - 1]
    y = torch.rand(4, N, generator=g) * 0.4
    y[:, 0] = 0.5
    for u, r in enumerate(want):
        y[u, 1 + torch.randperm(N - 1, generator=g)[:r]] = 0.6 + 0.3 * torch.rand(r, generator=g)
    sums, rank = run_rank(ops, y, k)
    assert rank.tolist() == want
    assert float(sums[0]) == 2.0 and float(sums[2]) == 0.0
    check_rank_sums(mode, sums, y, k, what=f"constructed N={N}")


@gpu
@pytest.mark.parametrize("N", [65, 129, 193])
def test_rank_metrics_with_pos(mode, N):
    """The positive away from column 0 (train.compute_HR / compute_NDCG): its own column counts neither above nor as a tie."""
    ops, _ = _ops()
    B = 33
    g = torch.Generator().manual_seed(N)
    y = tie_free(B, N, g)
    pos = torch.randint(0, N, (B,), generator=g)
    pos[:4] = torch.tensor([0, 63, 64, N - 1])
    want_rank, ties = ref_counts(y, pos)
    assert int(ties.sum()) == 0
    for p in (pos.to(torch.int32), pos):
        for k in (1, 10, N):
            sums, rank = run_rank(ops, y, k, pos=p)
            assert torch.equal(rank, want_rank)
            check_rank_sums(mode, sums, y, k, pos=pos, what=f"pos N={N} k={k}")
            assert float(sums[2]) == 0.0


@gpu
@pytest.mark.parametrize("N", [66, 193])
def test_rank_metrics_exact_ties(mode, N):
    """The positive's score copied into a known set of columns that sat below it: exact tie count, unchanged ranks."""
    ops, _ = _ops()
    B = 17
    g = torch.Generator().manual_seed(N)
    cols = sorted({1, 2, 63, 64, 65, N - 1})
    base = tie_free(B, N, g)
    base[:, cols] = -1.0 - torch.rand(B, len(cols), generator=g)
    free = torch.tensor([c for c in range(N) if c not in cols])  # (the positive itself sits in none of the tie columns)
    pos = free[torch.randint(0, len(free), (B,), generator=g)]
    pos[0], pos[1] = 0, free[-1]
    n_ties = B * len(cols)
    for p in (None, pos):
        pc = torch.zeros(B, dtype=torch.int64) if p is None else p
        y = base.clone()
        y[:, cols] = y.gather(1, pc.view(-1, 1)).expand(B, len(cols)).clone()
        _, base_rank = run_rank(ops, base, 10, pos=p)
        sums, rank = run_rank(ops, y, 10, pos=p)
        assert torch.equal(rank, base_rank) and torch.equal(rank, ref_counts(base, p)[0])
        assert float(sums[2]) == n_ties
        check_rank_sums(mode, sums, y, 10, pos=p, what=f"ties N={N}")


@gpu
def test_rank_metrics_infinities(mode):
    ops, _ = _ops()
    N = 130
    y = torch.linspace(0.0, 1.0, N).repeat(4, 1)
    y[0, 0] = INF                 # rank 0; two +inf candidates tie with it
    y[0, [5, 129]] = INF
    y[1, 0] = -INF                # below every number: rank N - 2, one tie
    y[1, 64] = -INF
    y[2, 0] = 0.5                 # -inf candidates are below, +inf above
    y[2, [1, 2, 3]] = -INF
    y[2, [70, 71]] = INF
    y[3, 0] = 2.0                 # above every number, below one +inf
    y[3, 128] = INF
    want_rank, want_ties = ref_counts(y)
    assert want_rank.tolist()[:2] == [0, N - 2] and want_ties.tolist() == [2, 1, 0, 0] and int(want_rank[3]) == 1
    for k in (1, 10):
        sums, rank = run_rank(ops, y, k)
        assert torch.equal(rank, want_rank)
        check_rank_sums(mode, sums, y, k, what=f"inf k={k}")


@gpu
@pytest.mark.parametrize("N", [101, 193])
def test_rank_metrics_nan_order(mode, N):
    """NaN ranks above every number and ties with NaN: the reference counts, and for the rows with a
    finite positive the reference's sort formula too."""
    ops, _ = _ops()
    k = 10
    y, want_rank, want_ties = nan_rows(N, k)
    fin_true = one_hot_true(3, N, torch.zeros(3, dtype=torch.int64))
    for kk in (k - 1, k, k + 1):
        sums, rank = run_rank(ops, y, kk)
        assert torch.equal(rank, want_rank), f"{mode} N={N}: ranks {rank.tolist()} != {want_rank.tolist()}"
        assert float(sums[2]) == float(want_ties.sum())
        check_rank_sums(mode, sums, y, kk, what=f"nan N={N} k={kk}")
        fin, _ = run_rank(ops, y[:3].contiguous(), kk)
        assert float(fin[0]) == sort_hr(y[:3], fin_true, kk)
        want = sort_ndcg(y[:3], fin_true, kk, torch.float64)
        assert abs(float(fin[1]) - want) <= ndcg_bound(want, 3)
    # the positive elsewhere
    pos = torch.tensor([N - 1, 64, 0, 7, 3])
    z = y.clone()
    for u in range(5):
        z[u, [0, int(pos[u])]] = z[u, [int(pos[u]), 0]]
    sums, rank = run_rank(ops, z, k, pos=pos)
    assert torch.equal(rank, want_rank) and float(sums[2]) == float(want_ties.sum())
    check_rank_sums(mode, sums, z, k, pos=pos, what=f"nan pos N={N}")


@gpu
def test_rank_metrics_accumulates_into_a_view(mode):
    ops, _ = _ops()
    g = torch.Generator().manual_seed(5)
    y = torch.rand(33, 101, generator=g)
    y[4, 9] = y[4, 0]
    five = torch.tensor([5.0, 2.0, 7.0, SENTINEL, SENTINEL], device="cuda")
    out, rank = ops.rank_metrics(y.cuda(), 10, sums=five[:3], want_rank=True)
    assert out.data_ptr() == five.data_ptr() and rank.dtype == torch.int32
    got = five.cpu()
    assert got[3:].tolist() == [SENTINEL, SENTINEL]
    check_rank_sums(mode, got[:3], y, 10, base=(5.0, 2.0, 7.0), what="view")
    assert float(got[2]) >= 8.0


@gpu
def test_rank_metrics_refusals(mode):
    ops, CarcaHipError = _ops()
    y = torch.rand(8, 20, device="cuda")
    with pytest.raises(CarcaHipError):
        ops.rank_metrics(y, 0)
    for n_pos in (9, 16, 7):  # (a pos shorter than B would be read past its end: the longer ones fail first without the check)
        with pytest.raises(CarcaHipError):
            ops.rank_metrics(y, 10, pos=torch.zeros(n_pos, dtype=torch.int32, device="cuda"))


# --------------------------------------------------------------------------------------------------
# eval_metrics
# --------------------------------------------------------------------------------------------------
def eval_arm(B, N):
    return "eval_metrics fast arm" if N <= 128 and B <= 192 else "eval_metrics general arm"


def eval_batch_inputs(B, N, seed, ties=True):
    """(y in (0, 1), y_true with the positive in column 0, ids about 70 % live with column 0 live)"""
    g = torch.Generator().manual_seed(seed)
    y = torch.rand(B, N, generator=g) * 0.98 + 0.01
    if ties and N > 1:
        for u in range(0, B, 3):
            y[u, 1 + (u * 5) % (N - 1)] = y[u, 0]
            y[u, N - 1] = y[u, 0]
    ids = (torch.rand(B, N, generator=g) < 0.7).int() * torch.randint(1, 90, (B, N), generator=g).int()
    ids[:, 0] = 7
    y_true = torch.zeros(B, N, dtype=torch.int32)
    y_true[:, 0] = 1
    return y, y_true, ids


EVAL_SHAPES = [(1, 1), (1, 2), (16, 65), (17, 66), (192, 85), (193, 84), (128, 128), (127, 129), (16, 1001), (7, 21)]


@gpu
@pytest.mark.parametrize("B,N", EVAL_SHAPES,
                         ids=[f"B{B}xN{N}-{'fast' if N <= 128 and B <= 192 else 'general'}_arm" for B, N in EVAL_SHAPES])
def test_eval_metrics_against_the_references(B, N):
    ops, _ = _ops()
    arm = eval_arm(B, N)
    y, y_true, ids = eval_batch_inputs(B, N, 1000 * B + N)
    mask = (ids != 0).float()
    refs = bce_refs(y.reshape(-1), y_true.reshape(-1).float(), mask.reshape(-1))
    yd, td, idd = y.cuda(), y_true.cuda(), ids.cuda()
    loss, _ = ops.bce_fwd(yd, td, idd, 1e-8)
    for k in sorted({1, 10, N, N + 5}):
        sums = torch.tensor([3.0, 0.0, 2.0, 0.0, 5.0, SENTINEL], device="cuda")
        ops.eval_metrics(yd, td, idd, k, sums)
        got = sums.cpu()
        what = f"B={B} N={N} k={k}"
        check_rank_sums(arm, got[:3], y, k, base=(3.0, 0.0, 2.0), what=what)
        check_loss(arm, got[3], refs, B * N, what)
        assert float(got[3]) == float(loss), f"{what}: the loss bits differ from bce_fwd's"
        assert float(got[4]) == 5.0 + B and float(got[5]) == SENTINEL
        ops.eval_metrics(yd, td, idd, k, sums)  # a second call adds the same terms: every sum doubles exactly
        twice = sums.cpu()
        first = got - torch.tensor([3.0, 0.0, 2.0, 0.0, 5.0, SENTINEL])
        assert torch.equal(twice[:5], got[:5] + first[:5]) and float(twice[5]) == SENTINEL, what


@gpu
def test_eval_metrics_refuses_more_than_16384_scores():
    ops, CarcaHipError = _ops()
    y, y_true, ids = (t.cuda() for t in eval_batch_inputs(129, 128, 3))
    sums = torch.zeros(5, device="cuda")
    with pytest.raises(CarcaHipError):
        ops.eval_metrics(y, y_true, ids, 10, sums)
    assert sums.cpu().tolist() == [0.0] * 5


@gpu
@pytest.mark.parametrize("N", [66, 128, 130], ids=["N66-fast_arm", "N128-fast_arm", "N130-general_arm"])
def test_eval_metrics_column_sweep(N):
    """As test_rank_metrics_column_sweep; at N = 130 the N - 1 users take two calls (B N <= 16384) into the same sums."""
    ops, _ = _ops()
    B = N - 1
    g = torch.Generator().manual_seed(N)
    y = torch.rand(B, N, generator=g) * 0.4
    y[:, 0] = 0.5
    y[torch.arange(B), torch.arange(B) + 1] = 0.9
    y_true = torch.zeros(B, N, dtype=torch.int32)
    y_true[:, 0] = 1
    ids = torch.ones(B, N, dtype=torch.int32)
    per_call = min(B, REGISTER_MAX // N)
    for k, hr in ((1, 0), (2, B)):
        sums = torch.zeros(5, device="cuda")
        for lo in range(0, B, per_call):
            part = slice(lo, min(lo + per_call, B))
            assert eval_arm(part.stop - part.start, N) == eval_arm(B, N)
            ops.eval_metrics(y[part].cuda(), y_true[part].cuda(), ids[part].cuda(), k, sums)
        got = sums.cpu()
        assert float(got[0]) == hr and float(got[2]) == 0 and float(got[4]) == B
        want = hr / math.log2(3.0)
        assert abs(float(got[1]) - want) <= ndcg_bound(want, B)


@gpu
@pytest.mark.parametrize("N", [101, 193], ids=["N101-fast_arm", "N193-general_arm"])
def test_eval_metrics_nan_and_infinite_scores(N):
    """The rank sums under NaN and +-inf scores (the loss of such a batch is not finite and is not looked at)."""
    ops, _ = _ops()
    arm = eval_arm(5, N)
    k = 10
    y, want_rank, want_ties = nan_rows(N, k)
    y_true = torch.zeros(5, N, dtype=torch.int32)
    y_true[:, 0] = 1
    ids = torch.ones(5, N, dtype=torch.int32)
    fin_true = one_hot_true(3, N, torch.zeros(3, dtype=torch.int64))
    for kk in (k - 1, k, k + 1):
        sums = torch.zeros(5, device="cuda")
        ops.eval_metrics(y.cuda(), y_true.cuda(), ids.cuda(), kk, sums)
        got = sums.cpu()
        assert float(got[0]) == float((want_rank < kk).sum()) and float(got[2]) == float(want_ties.sum())
        check_rank_sums(arm, got[:3], y, kk, what=f"nan N={N} k={kk}")
        assert float(got[4]) == 5
        fin = torch.zeros(5, device="cuda")
        ops.eval_metrics(y[:3].cuda(), y_true[:3].cuda(), ids[:3].cuda(), kk, fin)
        assert float(fin[0]) == sort_hr(y[:3], fin_true, kk)
        want = sort_ndcg(y[:3], fin_true, kk, torch.float64)
        assert abs(float(fin[1]) - want) <= ndcg_bound(want, 3)
    z = torch.linspace(0.0, 1.0, N).repeat(3, 1)
    z[0, 0], z[0, 5], z[0, N - 1] = INF, INF, INF
    z[1, 0], z[1, 64] = -INF, -INF
    z[2, 0], z[2, 1], z[2, 70] = 0.505, -INF, INF  # (0.505 is no j / (N - 1))
    sums = torch.zeros(5, device="cuda")
    ops.eval_metrics(z.cuda(), y_true[:3].cuda(), ids[:3].cuda(), k, sums)
    assert ref_counts(z)[1].tolist() == [2, 1, 0]
    check_rank_sums(arm, sums.cpu()[:3], z, k, what=f"inf N={N}")


# --------------------------------------------------------------------------------------------------
# callers: engine.eval_batch, train.compute_HR / compute_NDCG / evaluate over a stub model
# --------------------------------------------------------------------------------------------------
class PreparedScores(torch.nn.Module):
    """A model that returns prepared scores, one tensor per call."""

    def __init__(self, outs):
        super().__init__()
        self.outs, self.calls = list(outs), 0

    def forward(self, profile, targets):
        self.calls += 1
        return self.outs[self.calls - 1]


def stub_batch(y_true, ids, id_dtype):
    B = ids.shape[0]
    p_x = torch.ones(B, 3, dtype=torch.int32)
    return (p_x, None, None, ids.to(id_dtype), None, None, y_true.float())


@gpu
@pytest.mark.parametrize("B,N,id_dtype,route", [
    (128, 101, torch.int32, "eval_metrics fast arm"),
    (33, 101, torch.int64, "rank_metrics + BinaryCrossEntropy"),
    (170, 101, torch.int32, "rank_metrics + bce loop arm"),
], ids=["one_launch-fast_arm", "int64_ids-rank_kernel-bce_register_arm", "over_16384-rank_kernel-bce_loop_arm"])
def test_engine_eval_batch_routes(B, N, id_dtype, route, monkeypatch):
    from carca_replication_amd import engine
    ops, _ = _ops()
    called = []

    def noting(name, fn):
        def call(*a, **kw):
            called.append(name)
            return fn(*a, **kw)
        return call

    for name in ("eval_metrics", "rank_metrics", "bce_fwd"):
        monkeypatch.setattr(ops, name, noting(name, getattr(ops, name)))
    y, y_true, ids = eval_batch_inputs(B, N, 77 + B)
    mask = (ids != 0).float()
    refs = bce_refs(y.reshape(-1), y_true.reshape(-1).float(), mask.reshape(-1))
    model = PreparedScores([y.cuda()])
    batch = tuple(t if t is None else t.cuda() for t in stub_batch(y_true, ids, id_dtype))
    out, sums = engine.eval_batch(model, batch, k=10)
    assert called == (["eval_metrics"] if route.startswith("eval_metrics") else ["rank_metrics", "bce_fwd"]), called
    assert out.data_ptr() == model.outs[0].data_ptr()
    got = sums.cpu()
    check_rank_sums("eval_batch: " + route, got[:3], y, 10, what=route)
    check_loss("eval_batch: " + route, got[3], refs, B * N, route)
    assert float(got[4]) == B


@gpu
@pytest.mark.parametrize("B,N", [(33, 101), (5, 193)])
def test_train_compute_hr_ndcg_against_the_sort_formula(B, N):
    from carca_replication_amd import train

    g = torch.Generator().manual_seed(B + N)
    y = tie_free(B, N, g)
    cols = torch.randint(0, N, (B,), generator=g)
    cols[0], cols[1] = N - 1, 64
    y_true = one_hot_true(B, N, cols)
    for k in (1, 10, N):
        assert train.compute_HR(y.cuda(), y_true.cuda(), k) == sort_hr(y, y_true, k)
        want = sort_ndcg(y, y_true, k, torch.float64)
        got = train.compute_NDCG(y.cuda(), y_true.cuda(), k)
        if want > 0:
            _note("compute_NDCG err/bound", abs(got - want) / ndcg_bound(want, B))
        assert abs(got - want) <= ndcg_bound(want, B)


@gpu
def test_train_evaluate_over_three_batches():
    """(HR, NDCG, mean batch loss) over a three-batch loader: the sort formulas and the float64 loss statement summed over
    the batches.  The loss sum is two more fp32 adds of non-negative terms: eps32 / 2 of the sum each, on top of every
    batch's own rule."""
    from carca_replication_amd import train

    k, N = 10, 101
    sizes = [128, 64, 7]
    batches, outs = [], []
    hr = ndcg = 0.0
    loss64 = loss_bound = 0.0
    for i, B in enumerate(sizes):
        y, y_true, ids = eval_batch_inputs(B, N, 500 + i, ties=False)
        assert int(ref_counts(y)[1].sum()) == 0
        refs = bce_refs(y.reshape(-1), y_true.reshape(-1).float(), (ids != 0).float().reshape(-1))
        hr += sort_hr(y, y_true.float(), k)
        ndcg += sort_ndcg(y, y_true.float(), k, torch.float64)
        l64, l32 = float(refs["loss64"]), float(refs["loss32"])
        loss64 += l64
        loss_bound += 8 * abs(l32 - l64) + 4 * EPS32 * abs(l64)
        batches.append(stub_batch(y_true, ids, torch.int32))
        outs.append(y.cuda())
    loss_bound += 2 * (EPS32 / 2) * loss64
    users = sum(sizes)
    model = PreparedScores(outs)
    got_hr, got_ndcg, got_loss = train.evaluate(model, batches, "cuda", k)
    assert model.calls == 3
    assert got_hr == hr / users
    _note("evaluate NDCG err/bound", abs(got_ndcg - ndcg / users) / (ndcg_bound(ndcg, users) / users))
    assert abs(got_ndcg - ndcg / users) <= ndcg_bound(ndcg, users) / users + 1e-15  # (1e-15: the float64 divisions here)
    _note("evaluate loss err/bound", abs(got_loss - loss64 / 3) / (loss_bound / 3))
    assert abs(got_loss - loss64 / 3) <= loss_bound / 3 + 1e-15
