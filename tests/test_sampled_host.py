"""recommend_sampled (Gumbel top-k sampling with logged propensities), the parts that need no GPU:
the C surface and its argument checks, the Python argument errors -- each raised before any device work (the models here
live on the CPU) --, plackett_luce_log_prob against a float64 loop, and the yardsticks of tests/test_hip_sampled.py shown
sound on the host: the reference's own Gumbel top-k passes the distribution test's chi-square on that test's inputs, and
the order test's inputs leave few enough ambiguous pairs."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from carca_replication_amd import CarcaHipError, _lib, catalogue
from carca_replication_amd.modules import CARCA, KNN
from tests import sampling_ref as R
from tests.model_util import build_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_declared_bound_and_built():
    D, S, K, X = (C.POINTER(t) for t in (_lib.RecommendDesc, _lib.Candidates, _lib.KnnRecommendDesc, _lib.Sampling))
    assert _lib.SIGNATURES["carca_recommend_sampled"] == (C.c_int, [D, S, X, C.c_void_p])
    assert _lib.SIGNATURES["carca_knn_recommend_sampled"] == (C.c_int, [K, S, X, C.c_void_p])
    declared = _lib.declared_symbols()
    lib = _lib.load()
    for name in ("carca_recommend_sampled", "carca_knn_recommend_sampled"):
        assert name in declared, name
        assert list(getattr(lib, name).argtypes) == _lib.SIGNATURES[name][1]
    assert lib.carca_abi_version() == 3
    assert "recommend_sampled.hip" in _lib.SOURCES and "sampled_select.h" in _lib.HEADERS
    assert [f[0] for f in _lib.Sampling._fields_] == ["temperature", "seed", "user_keys", "log_probs", "ld_log_probs"]
    with open(os.path.join(ROOT, "include", "carca_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define CARCA_ABI_VERSION 3\b", header)
    for const in ("0x9E3779B1", "0x85EBCA77", "0xC2B2AE3D", "0x7feb352d", "0x846ca68b"):  # the hash is written down
        assert const in header, const


def test_python_surface():
    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    E = inspect.Parameter.empty
    assert params(CARCA.recommend_sampled) == [
        ("self", E), ("profile", E), ("context", E), ("k", 10), ("temperature", 1.0), ("seed", None), ("user_keys", None),
        ("exclude", "profile"), ("candidates", None), ("allow_composed", False)]
    assert params(KNN.recommend_sampled) == [
        ("self", E), ("profile", E), ("context", None), ("k", 10), ("temperature", 1.0), ("seed", None),
        ("user_keys", None), ("exclude", "profile"), ("candidates", None)]
    assert "cancel" in catalogue.plackett_luce_log_prob.__doc__.lower()
    assert CARCA.recommend_sampled.__doc__ and KNN.recommend_sampled.__doc__


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
    calls = ((lambda **kw: model.recommend_sampled(prof, ctx, **kw), "recommend_sampled"),
             (lambda **kw: knn.recommend_sampled(prof, None, **kw), r"KNN\.recommend_sampled"))
    for call, name in calls:
        for k in (0, 4097):
            with pytest.raises(CarcaHipError, match=rf"^{name}: k = {k} outside 1\.\.4096"):
                call(k=k)
        for t in (0, 0.0, -1.0, float("inf"), float("nan"), 1e-60, 1e-40, 1e60, "1", None, True):
            with pytest.raises(CarcaHipError, match=rf"^{name}: temperature must be a finite float > 0"):
                call(k=5, temperature=t)
        for keys in (torch.zeros(B + 1, dtype=torch.int64), torch.zeros(B, 1, dtype=torch.int64), torch.zeros(B),
                     torch.zeros(B, dtype=torch.bool), [0] * B):
            with pytest.raises(CarcaHipError, match=rf"^{name}: user_keys must be None or an int \[B\] tensor"):
                call(k=5, user_keys=keys)
        for seed in (1.5, "7", True):
            with pytest.raises(CarcaHipError, match=rf"^{name}: seed must be an int or None"):
                call(k=5, seed=seed)
        with pytest.raises(AssertionError, match="the model side ran"):  # good arguments do reach the model side
            call(k=4096, temperature=0.25, seed=-1, user_keys=torch.arange(B, dtype=torch.int32))
    model.train()
    with pytest.raises(CarcaHipError, match="^recommend_sampled: the model is in training mode"):
        model.recommend_sampled(prof, ctx, k=5)


def test_seed_none_is_drawn_from_torchs_cpu_generator_and_ints_wrap():
    prof = (torch.ones(2, 3, dtype=torch.int64),)
    torch.manual_seed(11)
    a = [catalogue.sampled_args("x", prof, 3, 1.0, None, None)[2] for _ in range(3)]
    torch.manual_seed(11)
    b = [catalogue.sampled_args("x", prof, 3, 1.0, None, None)[2] for _ in range(3)]
    assert a == b and len(set(a)) == 3
    assert catalogue.sampled_args("x", prof, 3, 2, -1, None) == (3, 2.0, 2 ** 64 - 1)
    assert catalogue.sampled_args("x", prof, 3, 0.1, 2 ** 64 + 5, None)[1:] == (C.c_float(0.1).value, 5)


def test_c_entry_points_check_their_arguments_before_any_launch():
    """Null pointers, the k range, strides and the temperature: all read before anything is allocated or launched (the
    pointers are never followed)."""
    lib = _lib.load()
    D = _lib.RecommendDesc(B=1, L=1, n_items=10, d=64, H=1, k=10, decoder=1, p_ids=64, ld_p_ids=1, item_q=64,
                           ld_item_q=64, user_q=64, ld_user_q=64, scores=64, ld_scores=4097, ids_out=64, ld_ids_out=4097)
    K = _lib.KnnRecommendDesc(B=1, L=1, n_items=10, F=4, k=10, p_ids=64, ld_p_ids=1, table=64, ld_table=4, scores=64,
                              ld_scores=4097, ids_out=64, ld_ids_out=4097)
    cand = _lib.Candidates(64, 3)
    for desc, entry, tag in ((D, lib.carca_recommend_sampled, b"recommend_sampled"),
                             (K, lib.carca_knn_recommend_sampled, b"knn_recommend_sampled")):
        for cp in (None, C.byref(cand)):
            X = _lib.Sampling(temperature=1.0, seed=1, log_probs=64, ld_log_probs=4097)

            def call():
                return entry(C.byref(desc), cp, C.byref(X), None)

            desc.k = 4097
            assert call() == -1 and tag in lib.carca_last_error() and b"4096" in lib.carca_last_error()
            desc.k = 0
            assert call() < 0
            desc.k = 10
            for t in (0.0, -1.0, 1e-40, float("inf"), float("nan")):
                X.temperature = t
                assert call() == -2 and tag + b": temperature must be finite and positive" in lib.carca_last_error()
            X.temperature = 1.0
            X.ld_log_probs = 9
            assert call() == -2 and b"row stride shorter than its row" in lib.carca_last_error()
            X.ld_log_probs, X.log_probs = 10, None
            assert call() == -2 and b"null pointer" in lib.carca_last_error()
            assert entry(C.byref(desc), cp, None, None) == -2 and b"null sampling block" in lib.carca_last_error()
            desc.ld_scores = 9
            X.log_probs = 64
            assert call() == -2
            desc.ld_scores = 4097
        assert entry(None, None, None, None) == -2
    X = _lib.Sampling(temperature=1.0, seed=1)
    assert "carca_sampled_perturb" in _lib.declared_symbols()
    for args in ((None, 64, 64, 1, 8), (64, None, 64, 1, 8), (64, 64, None, 1, 8), (64, 64, 64, 0, 8), (64, 64, 64, 1, 0),
                 (68, 64, 64, 1, 8), (64, 72, 64, 1, 8)):
        assert lib.carca_sampled_perturb(*args, C.byref(X), None) == -2 and b"sampled_perturb" in lib.carca_last_error()
    assert lib.carca_sampled_perturb(64, 64, 64, 1, 8, None, None) == -2
    X.temperature = 0.0
    assert lib.carca_sampled_perturb(64, 64, 64, 1, 8, C.byref(X), None) == -2
    bad = _lib.Candidates(None, 3)
    X = _lib.Sampling(temperature=1.0, seed=1, log_probs=64, ld_log_probs=10)
    assert lib.carca_recommend_sampled(C.byref(D), C.byref(bad), C.byref(X), None) == -2
    assert lib.carca_knn_recommend_sampled(C.byref(K), C.byref(bad), C.byref(X), None) == -2


def test_plackett_luce_log_prob_against_a_float64_loop():
    g = torch.Generator().manual_seed(4)
    z = torch.randn(6, 40, generator=g, dtype=torch.float64) * 2
    lp_all = torch.log_softmax(z, 1)
    rows = []
    for b in range(6):
        k = (1, 7, 40, 12, 3, 40)[b]
        pick = torch.randperm(40, generator=g)[:k]
        row = torch.full((40,), float("-inf"), dtype=torch.float64)
        row[:k] = lp_all[b, pick]
        rows.append(row)
    lp = torch.stack(rows).float()
    got = catalogue.plackett_luce_log_prob(lp)
    assert got.dtype == torch.float64 and got.shape == lp.shape
    for b in range(6):
        left = 1.0
        for j in range(40):
            v = float(lp[b, j])
            if v == float("-inf"):
                assert float(got[b, j]) == float("-inf")
                continue
            head = sum(math.exp(float(lp[b, m])) for m in range(j))
            want = v - math.log1p(-head) if head < 1 else float("inf")
            if left > 1e-3:  # (past it the cancellation the docstring states takes over)
                assert abs(float(got[b, j]) - want) < 1e-9 * max(1.0, 1.0 / left), (b, j)
            left = 1.0 - head - math.exp(v)
    assert float(lp[2].exp().sum()) == pytest.approx(1.0, abs=1e-5)  # (row 2 holds all 40 items)
    with pytest.raises(CarcaHipError):
        catalogue.plackett_luce_log_prob(torch.zeros(3, dtype=torch.float32))


def test_the_hash_and_the_gumbel_range():
    h = R.item_hash(R.user_hash(0x1234567890ABCDEF, [0, 1, -1, 2 ** 40 + 3]), [0, 1, 2, 1000, 2 ** 31 - 1])
    assert h.dtype == np.uint32 and h.shape == (4, 5) and len(set(h.flatten().tolist())) == 20
    assert int(R.mix32(0)) == 0  # (batch_build.hip's finaliser: xor-shifts and odd multiplications, a bijection)
    u = R.uniform(np.array([0, 0xFFFFFFFF, 0x1FF, 0x200], dtype=np.uint32))
    assert u[0] == 2.0 ** -24 and u[1] == 1 - 2.0 ** -24 and u[2] == u[0] and u[3] == 3 * 2.0 ** -24
    assert np.float32(u[1]) == u[1] and np.float32(u[1]) < 1  # exact in fp32, strictly inside (0, 1)
    g = -np.log(-np.log(u[:2]))
    assert g[0] == pytest.approx(R.G_MIN) and g[1] == pytest.approx(R.G_MAX)
    assert R.G_MIN == pytest.approx(-2.8116, abs=1e-4) and R.G_MAX == pytest.approx(16.6355, abs=1e-4)
    # same (seed, key, item) -> same noise wherever it sits; another seed or key -> other noise
    a = R.gumbel(7, [5, 9], [3, 4, 5])
    assert np.array_equal(a[1], R.gumbel(7, [9], [3, 4, 5])[0]) and np.array_equal(a[:, 1], R.gumbel(7, [5, 9], [4])[:, 0])
    assert not np.array_equal(a, R.gumbel(8, [5, 9], [3, 4, 5])) and not np.array_equal(a[0], a[1])
    assert np.array_equal(R.gumbel(7 + 2 ** 64, [5], [3]), R.gumbel(7, [5], [3]))


def test_chi2_critical_is_the_chi_square_quantile():
    for dof, alpha in ((1, 0.05), (10, 0.01), (31, 1e-6)):
        x = R.chi2_critical(dof, alpha)
        sf = float(torch.special.gammaincc(torch.tensor(dof / 2.0, dtype=torch.float64),
                                           torch.tensor(x / 2.0, dtype=torch.float64)))
        assert sf == pytest.approx(alpha, rel=1e-6)
    assert R.chi2_critical(1, 0.05) == pytest.approx(3.841459, abs=1e-5)
    assert R.chi2_critical(10, 0.01) == pytest.approx(23.20925, abs=1e-4)


def test_the_references_gumbel_topk_passes_the_distribution_yardstick():
    """The GPU distribution test's inputs, seed and chi-square, run on the reference's own draw: the hash's Gumbel top-k
    is a Plackett-Luce sample as far as that yardstick can see, so a GPU failure there is the kernels'."""
    _, _, _, _, _, ids, lg, tau, p = R.dist_inputs()
    rows = R.DIST["rows"]
    assert len(ids) >= 28 and p.max() < 0.5
    keys = (lg / tau)[None, :] + R.gumbel(R.DIST["seed"], np.arange(rows), ids)
    order = np.argsort(-keys, axis=1, kind="stable")
    for name, stat, dof, crit in R.dist_check(ids[order[:, 0]], ids[order[:, 1]], ids, p, rows):
        print(f"{name} pick: chi-square {stat:.2f} at {dof} dof, critical value at 1e-6 {crit:.2f}")
        assert dof >= 10 and stat < crit
    # and the yardstick can fail: the second pick drawn from the FIRST pick's distribution is rejected
    wrong = R.chi2_stat(np.array([(ids[order[:, 0]] == i).sum() for i in ids]), R.pl_marginals(p ** 2 / (p ** 2).sum())[0], rows)
    assert wrong[0] > R.chi2_critical(wrong[1], 1e-6)


def test_the_order_tests_inputs_leave_few_ambiguous_pairs():
    """For the inputs, seeds and temperatures of the GPU order test, the share of adjacent reference keys closer than the
    margin -- taken at e_bound, which that test asserts its measured e stays below -- is under the cap, over the test's
    inputs as a whole.  (By geometry the dot decoder alone is above it: its e is the fp32 sigmoid read back at |logit|
    near 8, 3e-4, whatever the kernels do; the figures are printed.)"""
    close = total = 0
    for geo in R.GEOS:
        c_geo = t_geo = 0
        for n in R.SIZES:
            cfg, P, attrs, batch = R.oracle_setup(geo, R.L, R.B, n)
            y = R.oracle_logits(geo, cfg, P, attrs, batch, n).numpy()
            assert np.isfinite(y).all()
            e = R.e_bound(geo, y[:, 1:])
            for tau in R.order_taus(y):
                for b in range(R.B):
                    ids = R.eligible_ids(batch[0][b], n)
                    _, keys = R.perturbed_order(y[b, ids] / tau, ids, 1000 + n, b)
                    gaps = keys[:-1] - keys[1:]
                    assert (gaps >= 0).all()
                    c_geo += int((gaps <= R.order_margin(e, tau)).sum())
                    t_geo += gaps.size
        print(f"{geo}: {c_geo} of {t_geo} adjacent pairs inside the margin ({c_geo / t_geo:.4f})")
        close, total = close + c_geo, total + t_geo
    print(f"all inputs: {close} of {total} ({close / total:.4f})")
    assert close / total < R.AMBIGUOUS_CAP
