"""log_prob_items and the off-policy estimators, the parts that need no GPU: the C surface and its
argument checks, the Python argument errors -- each raised before any device work (the models here live on the CPU) --,
policy_log_ratio and off_policy_estimate against closed forms in numpy float64, and the power of the end-to-end test of
tests/test_hip_policy.py shown from the oracle alone: its band can tell the target policy's value from the logging
policy's."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from carca_replication_amd import CarcaHipError, _lib, catalogue, train
from carca_replication_amd.modules import CARCA, KNN
from tests import policy_ref as PR
from tests.model_util import build_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG_INF = float("-inf")


def test_entry_points_declared_bound_and_built():
    D, S, K, X = (C.POINTER(t) for t in (_lib.RecommendDesc, _lib.Candidates, _lib.KnnRecommendDesc, _lib.PolicyItems))
    assert _lib.SIGNATURES["carca_log_prob_items"] == (C.c_int, [D, S, X, C.c_void_p])
    assert _lib.SIGNATURES["carca_knn_log_prob_items"] == (C.c_int, [K, S, X, C.c_void_p])
    assert _lib.SIGNATURES["carca_policy_reduce"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float,
                                                                C.c_void_p])
    declared = _lib.declared_symbols()
    lib = _lib.load()
    for name in ("carca_log_prob_items", "carca_knn_log_prob_items", "carca_policy_reduce"):
        assert name in declared, name
        assert list(getattr(lib, name).argtypes) == _lib.SIGNATURES[name][1]
    assert lib.carca_abi_version() == 3  # (calls were added, none changed)
    assert "policy_items.hip" in _lib.SOURCES and "policy_items.h" in _lib.HEADERS
    # the block's layout: the header's fields, in its order, with its types
    fields = [("temperature", C.c_float), ("items", C.c_void_p), ("n_list", C.c_int32), ("ld_items", C.c_int32),
              ("log_probs", C.c_void_p), ("ld_log_probs", C.c_int32), ("lse", C.c_void_p), ("entropy", C.c_void_p)]
    assert list(_lib.PolicyItems._fields_) == fields
    with open(os.path.join(ROOT, "include", "carca_hip.h")) as f:
        header = f.read()
    body = re.search(r"typedef struct CarcaPolicyItems \{(.*?)\} CarcaPolicyItems;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert decls == ["float temperature", "const int64_t* items", "int n_list", "int ld_items", "float* log_probs",
                     "int ld_log_probs", "float* lse", "float* entropy"]
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert ("int carca_log_prob_items(const CarcaRecommendDesc* desc, const CarcaCandidates* candidates , "
            "const CarcaPolicyItems* policy, void* stream);") in flat
    assert ("int carca_knn_log_prob_items(const CarcaKnnRecommendDesc* desc, const CarcaCandidates* candidates , "
            "const CarcaPolicyItems* policy, void* stream);") in flat
    assert ("int carca_policy_reduce(const float* logits, float* partials, int B, int n_slots, float temperature, "
            "void* stream);") in flat


def test_python_surface():
    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    E = inspect.Parameter.empty
    assert params(CARCA.log_prob_items) == [
        ("self", E), ("profile", E), ("context", E), ("items", E), ("temperature", 1.0), ("exclude", "profile"),
        ("candidates", None), ("allow_composed", False)]
    assert params(KNN.log_prob_items) == [
        ("self", E), ("profile", E), ("context", None), ("items", ...), ("temperature", 1.0), ("exclude", "profile"),
        ("candidates", None)]
    assert params(catalogue.policy_log_ratio) == [("target_log_probs", E), ("logged_log_probs", E), ("mode", "first")]
    assert params(catalogue.off_policy_estimate) == [("log_ratio", E), ("rewards", E), ("clip", None)]
    assert params(train.off_policy_value) == [
        ("model", E), ("logs", E), ("device", E), ("temperature", 1.0), ("mode", "first"), ("clip", None),
        ("exclude", "profile"), ("candidates", None), ("allow_composed", False)]
    assert CARCA.log_prob_items.__doc__ and KNN.log_prob_items.__doc__


def test_argument_errors_are_raised_before_any_device_work(monkeypatch):
    n, B, L, n_ctx = 50, 3, 8, 6
    model = build_model(dict(d=64, H=4, n_blocks=1, embedding="all", decoder="ca"), n, 24, n_ctx, 12, L).eval()
    knn = KNN()
    knn.register_attr_table(torch.zeros(n, 5))

    def launched(*a, **kw):
        raise AssertionError("the model side ran before the arguments were checked")

    monkeypatch.setattr(catalogue, "carca_model_side", launched)
    monkeypatch.setattr(catalogue, "knn_model_side", launched)
    prof = (torch.ones(B, L, dtype=torch.int64), None, torch.zeros(B, L, n_ctx))
    ctx = torch.zeros(B, n_ctx)
    items = torch.ones(B, 4, dtype=torch.int64)
    calls = ((lambda **kw: model.log_prob_items(prof, ctx, **kw), "log_prob_items"),
             (lambda **kw: knn.log_prob_items(prof, None, **kw), r"KNN\.log_prob_items"))
    for call, name in calls:
        for t in (0, 0.0, -1.0, float("inf"), float("nan"), 1e-60, 1e-40, 1e60, "1", None, True):
            with pytest.raises(CarcaHipError, match=rf"^{name}: temperature must be a finite float > 0"):
                call(items=items, temperature=t)
        for bad in (items.float(), torch.ones(B + 1, 4, dtype=torch.int64), torch.ones(B, dtype=torch.int64),
                    torch.ones(B, 4, dtype=torch.bool), [[1] * 4] * B):
            with pytest.raises(CarcaHipError, match=rf"^{name}: items must be an int \[B, N\] tensor"):
                call(items=bad)
        for good in (items, items.to(torch.int32), torch.ones(B, 0, dtype=torch.int64)):
            with pytest.raises(AssertionError, match="the model side ran"):  # good arguments do reach the model side
                call(items=good, temperature=0.25)
    with pytest.raises(CarcaHipError, match=r"^KNN\.log_prob_items: items is required"):
        knn.log_prob_items(prof)
    model.train()
    with pytest.raises(CarcaHipError, match="^log_prob_items: the model is in training mode"):
        model.log_prob_items(prof, ctx, items)


def test_c_entry_points_check_their_arguments_before_any_launch():
    """Null pointers, strides and the temperature: all read before anything is allocated or launched (the pointers are
    never followed).  The descriptor's k, scores and ids_out stay zero: the calls do not read them."""
    lib = _lib.load()
    D = _lib.RecommendDesc(B=1, L=1, n_items=10, d=64, H=1, decoder=1, p_ids=64, ld_p_ids=1, item_q=64, ld_item_q=64,
                           user_q=64, ld_user_q=64)
    K = _lib.KnnRecommendDesc(B=1, L=1, n_items=10, F=4, p_ids=64, ld_p_ids=1, table=64, ld_table=4)
    cand = _lib.Candidates(64, 3)
    for desc, entry, tag in ((D, lib.carca_log_prob_items, b"log_prob_items"),
                             (K, lib.carca_knn_log_prob_items, b"knn_log_prob_items")):
        for cp in (None, C.byref(cand)):
            X = _lib.PolicyItems(temperature=1.0, items=64, n_list=10, ld_items=10, log_probs=64, ld_log_probs=10)

            def call():
                return entry(C.byref(desc), cp, C.byref(X), None)

            for t in (0.0, -1.0, 1e-40, float("inf"), float("nan")):
                X.temperature = t
                assert call() == -2 and tag + b": temperature must be finite and positive" in lib.carca_last_error()
            X.temperature = 1.0
            X.ld_log_probs = 9
            assert call() == -2 and tag + b": row stride shorter than its row" in lib.carca_last_error()
            X.ld_log_probs, X.ld_items = 10, 9
            assert call() == -2 and tag + b": row stride shorter than its row" in lib.carca_last_error()
            X.ld_items, X.log_probs = 10, None
            assert call() == -2 and tag + b": null pointer" in lib.carca_last_error()
            X.log_probs, X.items = 64, None
            assert call() == -2 and tag + b": null pointer" in lib.carca_last_error()
            X.items, X.n_list = 64, -1
            assert call() == -2 and tag in lib.carca_last_error()
            assert entry(C.byref(desc), cp, None, None) == -2 and tag + b": null policy block" in lib.carca_last_error()
        assert entry(None, None, None, None) == -2 and tag + b": null descriptor" in lib.carca_last_error()
        bad = _lib.Candidates(None, 3)
        X = _lib.PolicyItems(temperature=1.0, items=64, n_list=10, ld_items=10, log_probs=64, ld_log_probs=10)
        assert entry(C.byref(desc), C.byref(bad), C.byref(X), None) == -2
    for args in ((None, 64, 1, 8, 1.0), (64, None, 1, 8, 1.0), (64, 64, 0, 8, 1.0), (64, 64, 1, 0, 1.0), (68, 64, 1, 8, 1.0),
                 (64, 64, 1, 8, 0.0), (64, 64, 1, 8, 1e-40), (64, 64, 1, 8, float("nan"))):
        assert lib.carca_policy_reduce(*args, None) == -2 and b"policy_reduce" in lib.carca_last_error()


# ---- the host layer against closed forms ----------------------------------------------------------------------------
def test_policy_log_ratio_against_closed_forms():
    g = torch.Generator().manual_seed(5)
    B, k, n = 7, 4, 30
    za, zb = torch.randn(B, n, generator=g, dtype=torch.float64), torch.randn(B, n, generator=g, dtype=torch.float64)
    la, lb = torch.log_softmax(za, 1), torch.log_softmax(zb, 1)
    pick = torch.stack([torch.randperm(n, generator=g)[:k] for _ in range(B)])
    logged, target = la.gather(1, pick).float(), lb.gather(1, pick).float()
    # the same policy: every ratio exactly 0, in both modes
    for mode in ("first", "list"):
        out = catalogue.policy_log_ratio(logged, logged, mode)
        assert out.dtype == torch.float64 and out.shape == (B,) and bool((out == 0).all())
    # "first": column 0
    got = catalogue.policy_log_ratio(target, logged)
    assert torch.equal(got, target[:, 0].double() - logged[:, 0].double())
    # "list": the Plackett-Luce log-probability of the ordered list, by a float64 loop
    got = catalogue.policy_log_ratio(target, logged, "list").numpy()

    def pl(row):
        left, total = 1.0, 0.0
        for v in row:
            total += v - np.log(left)
            left -= np.exp(v)
        return total

    for b in range(B):
        want = pl(target[b].double().numpy()) - pl(logged[b].double().numpy())
        assert abs(got[b] - want) < 1e-12, b
    # padding: a logged row with fewer than k items; the target's value under the padding does not matter while it is -inf
    lg2, tg2 = logged.clone(), target.clone()
    lg2[2, 2:], tg2[2, 2:] = NEG_INF, NEG_INF
    got = catalogue.policy_log_ratio(tg2, lg2, "list").numpy()
    want = pl(tg2[2, :2].double().numpy()) - pl(lg2[2, :2].double().numpy())
    assert abs(got[2] - want) < 1e-12 and np.isfinite(got).all()
    lg3, tg3 = logged.clone(), target.clone()
    lg3[:, 0], tg3[:, 0] = NEG_INF, NEG_INF  # (a user with no eligible item: nothing logged, ratio 0)
    assert bool((catalogue.policy_log_ratio(tg3, lg3) == 0).all())
    # a -inf target where the log is finite: -inf, weight 0
    tg4 = target.clone()
    tg4[1, 0], tg4[3, 2] = NEG_INF, NEG_INF
    first, lst = catalogue.policy_log_ratio(tg4, logged), catalogue.policy_log_ratio(tg4, logged, "list")
    assert float(first[1]) == NEG_INF and bool(torch.isfinite(first[[0, 2, 3, 4, 5, 6]]).all())
    assert float(lst[1]) == NEG_INF and float(lst[3]) == NEG_INF and not bool(torch.isnan(lst).any())
    assert float(torch.exp(first[1])) == 0.0
    # a finite target where the log says -inf: the logging policy cannot have drawn it
    lg5 = logged.clone()
    lg5[4, 0] = NEG_INF
    with pytest.raises(CarcaHipError, match="^policy_log_ratio: a logged log-probability is -inf where the target's is finite"):
        catalogue.policy_log_ratio(target, lg5)
    lg5 = logged.clone()
    lg5[4, 3] = NEG_INF
    catalogue.policy_log_ratio(target, lg5)  # ("first" reads column 0 only)
    with pytest.raises(CarcaHipError, match="^policy_log_ratio: a logged"):
        catalogue.policy_log_ratio(target, lg5, "list")
    for bad in ((target[0], logged[0]), (target.long(), logged), (target[:, :2], logged), (target[:, :0], logged[:, :0])):
        with pytest.raises(CarcaHipError, match="^policy_log_ratio: "):
            catalogue.policy_log_ratio(*bad)
    with pytest.raises(CarcaHipError, match="^policy_log_ratio: mode must be"):
        catalogue.policy_log_ratio(target, logged, "all")


def test_off_policy_estimate_against_closed_forms():
    g = torch.Generator().manual_seed(6)
    n = 500
    r = (torch.rand(n, generator=g) < 0.4).float()
    # weights all 1: ips = snips = the mean reward exactly, ess = n
    out = catalogue.off_policy_estimate(torch.zeros(n, dtype=torch.float64), r)
    assert sorted(out) == ["clip", "ess", "ips", "max_weight", "n", "snips"]
    assert all(isinstance(out[k], torch.Tensor) and out[k].dtype == torch.float64 and out[k].dim() == 0
               for k in ("ips", "snips", "ess", "max_weight", "n"))
    mean = float(r.double().mean())
    assert float(out["ips"]) == mean and float(out["snips"]) == mean and float(out["ess"]) == n
    assert float(out["max_weight"]) == 1.0 and float(out["n"]) == n and out["clip"] is None
    # random weights, some of them 0 (a -inf ratio)
    lr = torch.randn(n, generator=g, dtype=torch.float64)
    lr[::17] = NEG_INF
    for clip in (None, 1.5, 0.25):
        out = catalogue.off_policy_estimate(lr, r, clip=clip)
        want = PR.estimates(lr.numpy(), r.numpy(), clip)
        for k in ("ips", "snips", "ess", "max_weight", "n"):
            assert float(out[k]) == pytest.approx(want[k], rel=1e-12), (clip, k)
        assert out["clip"] == clip and not any(bool(torch.isnan(out[k])) for k in ("ips", "snips", "ess"))
    assert float(catalogue.off_policy_estimate(lr, r, clip=1.5)["max_weight"]) == 1.5
    assert float(catalogue.off_policy_estimate(lr, r)["max_weight"]) > 1.5  # (so the clip did cap something)
    # a clipped case by hand: w = (1, 2 -> 1.5, 0.5), r = (1, 1, 0)
    out = catalogue.off_policy_estimate(torch.tensor([0.0, np.log(2.0), np.log(0.5)], dtype=torch.float64),
                                        torch.tensor([1.0, 1.0, 0.0]), clip=1.5)
    assert float(out["ips"]) == pytest.approx(2.5 / 3) and float(out["snips"]) == pytest.approx(2.5 / 3.0)
    assert float(out["ess"]) == pytest.approx(9.0 / 3.5)
    for bad in ((lr, r[:-1]), (lr.reshape(1, -1), r.reshape(1, -1)), (lr.tolist(), r)):
        with pytest.raises(CarcaHipError, match="^off_policy_estimate: "):
            catalogue.off_policy_estimate(*bad)
    for clip in (0, -1.0, True, "2"):
        with pytest.raises(CarcaHipError, match="^off_policy_estimate: clip must be"):
            catalogue.off_policy_estimate(lr, r, clip=clip)


def test_policy_ref_stats():
    z = np.log(np.array([0.5, 0.25, 0.125, 0.125])) + 3.0
    lp, lse, H, g1 = PR.policy_stats(z)
    assert np.allclose(np.exp(lp), [0.5, 0.25, 0.125, 0.125]) and lse == pytest.approx(3.0)
    assert H == pytest.approx(1.75 * np.log(2.0)) and PR.entropy_of_log_probs(lp) == pytest.approx(H)
    eps = 1e-6  # the gradient's 1-norm against central differences
    num = sum(abs(PR.policy_stats(z + eps * np.eye(4)[i])[2] - PR.policy_stats(z - eps * np.eye(4)[i])[2]) / (2 * eps)
              for i in range(4))
    assert g1 == pytest.approx(num, rel=1e-6)
    assert PR.policy_stats(np.zeros(0)) == pytest.approx((np.zeros(0), NEG_INF, 0.0, 0.0))
    assert PR.policy_stats(np.zeros(8))[2] == pytest.approx(np.log(8.0))  # a uniform policy chooses among all 8


def test_the_end_to_end_tests_band_has_power():
    """The GPU end-to-end test accepts an IPS estimate within 4.9 sd + 1e-3 of the target's exact value V_B.  From the
    oracle alone: the logging policy's value V_A -- what the unweighted mean reward estimates -- lies more than three
    bands below V_B, so an estimator that ignored its weights would fail; and no item dominates the logging policy."""
    e = PR.e2e_inputs()
    print(f"{len(e['ids'])} eligible items, tau_A = {e['tau_a']:.4f}, V_A = {e['v_a']:.4f}, V_B = {e['v_b']:.4f}, "
          f"{PR.SIGMAS} sd = {PR.SIGMAS * e['sd']:.4f}, band = {e['band']:.4f}, largest weight {e['w'].max():.3f}")
    assert len(e["ids"]) >= 28 and 0 < e["reward"].sum() < len(e["ids"])
    assert e["p_a"].sum() == pytest.approx(1.0) and e["p_b"].sum() == pytest.approx(1.0)
    assert e["v_b"] - e["v_a"] > 3 * e["band"]
    assert e["p_a"].max() < 0.5
    assert (e["p_a"] * e["w"]).sum() == pytest.approx(1.0)  # E_A[w] = 1: the weights are a change of measure
    assert (e["p_a"] * e["w"] * e["reward"]).sum() == pytest.approx(e["v_b"])  # and IPS is unbiased for V_B
