"""The host side of the BCE against K shared negatives, gBCE, on the CPU: the kernels' sizing
(ops.sampled_bce_plan), the argument errors of ops.sampled_bce, the engine's names and refusals, beta, the C ABI surface
(header, ctypes struct, signatures), and the fp64 restatement of the loss the GPU tests compare against."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from carca_replication_amd import CarcaHipError, _lib, engine, ops
from carca_replication_amd.sampling import ItemSampler
from tests.test_knn_catalogue_host import _header_fields


def ref_bce(P, Tp, pos, S, s_ids, n_items, beta, C=None):  # noqa: N803
    """The loss in the dtype of its operands (fp64 in the tests), differentiable by torch.autograd:
    sum over valid r of ( beta sp(-P[r] . Tp[r]) + sum_{k in N_r} sp(P[r] . S[k] + P[r] . C[r]) ) / n_valid, with
    N_r = {k : s_k in [1, n_items), s_k != pos_r}; 0 (connected to every operand) without a valid row."""
    pos, s = pos.long().to(P.device), s_ids.long().to(P.device)
    valid = (pos >= 1) & (pos < n_items)
    if not bool(valid.any()):
        return (P.sum() + Tp.sum() + S.sum() + (C.sum() if C is not None else 0.0)) * 0.0
    s_ok = (s >= 1) & (s < n_items)
    Pv, pv = P[valid], pos[valid]
    zp = (Pv * Tp[valid]).sum(1)
    zs = Pv @ S.T
    if C is not None:
        zs = zs + (Pv * C[valid]).sum(1, keepdim=True)
    neg = s_ok.view(1, -1) & (s.view(1, -1) != pv.view(-1, 1))
    rows = beta * F.softplus(-zp) + (F.softplus(zs) * neg).sum(1)
    return rows.sum() / valid.sum()


def test_plan_split_counts_and_scratch():
    for R, K, d in [(6400, 256, 128), (6400, 8192, 90), (1, 1, 64), (17, 63, 90), (700, 2048, 192), (100_000, 1000, 256)]:
        p = ops.sampled_bce_plan(R, K, d, n_cus=256)
        per, s_s, s_r = p["samples_per_split"], p["splits_samples"], p["splits_rows"]
        assert per % 64 == 0 and per * s_s >= K and (s_s - 1) * per < K  # covers K, no empty split
        assert 1 <= s_s <= 256 and 1 <= s_r <= 256
        x = ops.sampled_xent_plan(R, K, d, n_cus=256)  # the same skeleton, one extra dP partial in both ...
        assert all(p[k] == x[k] for k in p if k != "scratch_bwd")
        ldo, r64 = (d + 3) // 4 * 4, (lambda n: (n + 63) // 64 * 64)
        dp, ds = r64((s_s + 1) * R * ldo), (r64(s_r * K * ldo) if s_r > 1 else 0)
        assert x["scratch_bwd"] == 2 * r64(R) + 64 + dp + ds
        assert p["scratch_bwd"] == 2 * r64(R) + 64 + max(dp, ds)  # ... but dS's partials reuse the words of dP's
    # hand-computed against csrc/xent_tile.h's XentLayout: 2 ceil64(R) + 64 words of row lists, then 2 ceil64(s_s R)
    # (sum softplus, sum sigmoid) words, or the larger of ceil64((s_s + 1) R ld) dP words and, with s_r > 1,
    # ceil64(s_r K ld) dS words
    hand = {
        # 100 row blocks, 1024 workgroups wanted: 4 of the 4 sample blocks; 256 row splits wanted, 100 row blocks
        (6400, 256, 128): (4, 64, 100, 12864 + 2 * 25600, 12864 + max(5 * 6400 * 128, 100 * 256 * 128)),
        (6400, 8192, 128): (11, 768, 8, 12864 + 140800, 12864 + max(9830400, 8388608)),
        # 20 row blocks, 64 sample blocks: 52 splits wanted -> 2 blocks each -> 32 splits; 16 row splits (dS's set larger)
        (1280, 4096, 64): (32, 128, 16, 2624 + 2 * 40960, 2624 + max(33 * 1280 * 64, 16 * 4096 * 64)),
        (17, 63, 90): (1, 64, 1, 192 + 128, 192 + 3136),
        (1, 1, 64): (1, 64, 1, 320, 320),
    }
    for (R, K, d), want in hand.items():
        p = ops.sampled_bce_plan(R, K, d, n_cus=256)
        assert (p["splits_samples"], p["samples_per_split"], p["splits_rows"], p["scratch_fwd"], p["scratch_bwd"]) == want
    with pytest.raises(CarcaHipError):
        ops.sampled_bce_plan(0, 10, 8)
    with pytest.raises(CarcaHipError):
        ops.sampled_bce_plan(10, 0, 8)
    with pytest.raises(CarcaHipError):
        ops.sampled_bce_plan(10, 10, 0)


def test_op_argument_errors():
    P, Tp, S = torch.zeros(5, 8), torch.zeros(5, 8), torch.zeros(7, 8)
    pos, s = torch.ones(5, dtype=torch.int64), torch.ones(7, dtype=torch.int64)
    with pytest.raises(CarcaHipError, match="expected P"):
        ops.sampled_bce(P, Tp[:4], pos, S, s, 10, 0.5)
    with pytest.raises(CarcaHipError, match="expected P"):
        ops.sampled_bce(P, Tp, pos, S[:, :6], s, 10, 0.5)
    with pytest.raises(CarcaHipError, match="C must have the shape of P"):
        ops.sampled_bce(P, Tp, pos, S, s, 10, 0.5, C=torch.zeros(5, 7))
    with pytest.raises(CarcaHipError, match="entries"):
        ops.sampled_bce(P, Tp, pos[:4], S, s, 10, 0.5)
    with pytest.raises(CarcaHipError, match="entries"):
        ops.sampled_bce(P, Tp, pos, S, s[:6], 10, 0.5)
    with pytest.raises(CarcaHipError, match="at least one sample"):
        ops.sampled_bce(P, Tp, pos, S[:0], s[:0], 10, 0.5)
    with pytest.raises(CarcaHipError, match="integer"):
        ops.sampled_bce(P, Tp, pos.float(), S, s, 10, 0.5)
    with pytest.raises(CarcaHipError, match="integer"):
        ops.sampled_bce(P, Tp, pos, S, s.float(), 10, 0.5)
    with pytest.raises(CarcaHipError, match="sampled_bce: P, Tp, S and C must be float32"):
        ops.sampled_bce(P.double(), Tp, pos, S, s, 10, 0.5)
    with pytest.raises(CarcaHipError, match="sampled_bce: P, Tp, S and C must be float32"):
        ops.sampled_bce(P, Tp, pos, S, s, 10, 0.5, C=torch.zeros(5, 8, dtype=torch.float64))
    with pytest.raises(CarcaHipError, match="n_items"):
        ops.sampled_bce(P, Tp, pos, S, s, 1, 0.5)
    for beta in (-0.1, 1.5):
        with pytest.raises(CarcaHipError, match="beta"):
            ops.sampled_bce(P, Tp, pos, S, s, 10, beta)
    with pytest.raises(CarcaHipError, match="CPU"):  # no CPU implementation: the op runs on the GPU only
        ops.sampled_bce(P, Tp, pos, S, s, 10, 0.5, C=torch.zeros(5, 8))


def test_engine_knows_the_loss_and_its_defaults():
    assert "sampled_bce" in engine.LOSSES
    assert engine.SAMPLED_BCE_DEFAULT_K == 256 and engine.SAMPLED_BCE_T == 0.75
    assert engine.SAMPLED_DEFAULT_K == 8192  # (the sampled softmax keeps its own)


def test_a_counts_sampler_is_refused(tmp_path):
    from carca_replication_amd.train import train

    sampler = ItemSampler(10, 4, counts=torch.arange(10), device="cpu")
    batch = tuple(torch.zeros(1, 2) for _ in range(7))
    with pytest.raises(ValueError, match="uniform"):
        engine.train_step(None, None, batch, loss="sampled_bce", sampler=sampler)
    with pytest.raises(ValueError, match="uniform"):
        train(model=None, train_loader=None, val_loader=None, test_loader=None, device="cpu", optim=None, epochs=1,
              datadir=str(tmp_path), loss="sampled_bce", sampler=sampler)
    # the other losses still refuse any sampler
    for loss in ("bce", "softmax"):
        with pytest.raises(ValueError, match="sampler"):
            engine.train_step(None, None, batch, loss=loss, sampler=ItemSampler(10, 4, device="cpu"))


def test_graphed_training_is_refused(tmp_path):
    from carca_replication_amd.train import train

    with pytest.raises(CarcaHipError, match="graphed"):
        train(model=None, train_loader=None, val_loader=None, test_loader=None, device="cpu", optim=None, epochs=1,
              datadir=str(tmp_path), loss="sampled_bce", graphed=True)


def test_beta_and_the_range_of_t():
    K, n_items = 256, 1025  # alpha = 256 / 1024 = 0.25
    assert ops.sampled_bce_beta(K, n_items, 0.0) == 1.0       # plain BCE over K negatives
    assert ops.sampled_bce_beta(K, n_items, 1.0) == 0.25      # fully calibrated: beta = alpha
    assert ops.sampled_bce_beta(K, n_items, 0.75) == 1.0 - 0.75 * 0.75
    assert ops.sampled_bce_beta(5000, 1025, 1.0) == 1.0       # (more samples than items: the rate saturates at 1)
    for t in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match="t must lie in"):
            ops.sampled_bce_beta(K, n_items, t)


def test_model_method_takes_t_with_the_papers_default():
    import inspect

    from carca_replication_amd.modules import CARCA

    sig = inspect.signature(CARCA.sampled_bce_loss)
    assert list(sig.parameters)[1:] == ["profile", "pos", "pos_ctx", "samples", "t"] and sig.parameters["t"].default == 0.75


def test_header_struct_and_signatures_agree():
    assert _header_fields("CarcaSampledBceDesc") == [f[0] for f in _lib.SampledBceDesc._fields_]
    D = _lib.SampledBceDesc
    # the C layout on LP64: 4 ints, then pointer / int pairs (each int padded to the next pointer)
    assert D.P.offset == 16 and D.C.offset == 48 and D.ld_c.offset == 56 and D.pos.offset == 64
    assert D.beta.offset == 96 and D.splits_samples.offset == 100 and D.scratch.offset == 112
    assert D.scratch_floats.offset == 120 and D.zpos.offset == 128 and D.dS.offset == 200 and C.sizeof(D) == 208
    declared = _lib.declared_symbols()
    for fn in ("carca_sampled_bce_fwd", "carca_sampled_bce_bwd"):
        assert fn in declared
        res, args = _lib.SIGNATURES[fn]
        assert res is C.c_int and args == [C.POINTER(D), C.c_void_p]
    assert "sampled_bce.hip" in _lib.SOURCES and "xent_stage.h" in _lib.HEADERS


def test_k1_t0_is_binary_cross_entropy_with_logits():
    """One negative and beta = 1: the restated loss is the reference's BCE over (positive logit, negative logit), summed
    and divided by the valid rows."""
    g = torch.Generator().manual_seed(0)
    R, d, n_items = 40, 16, 50
    P, Tp, C_ = (torch.randn(R, d, generator=g, dtype=torch.float64) for _ in range(3))
    S = torch.randn(1, d, generator=g, dtype=torch.float64)
    pos = torch.randint(1, n_items, (R,), generator=g)
    pos[::7] = 0
    s = torch.tensor([n_items + 5])  # an id no row has as its positive ... and no class at all: every negative masked
    assert float(ref_bce(P, Tp, pos, S, s, n_items, 1.0, C_)) == pytest.approx(
        float(F.softplus(-(P * Tp).sum(1))[pos != 0].sum() / (pos != 0).sum()), rel=1e-12)
    s = torch.tensor([n_items - 1])
    pos[pos == n_items - 1] = 1  # (no accidental hit: every valid row has exactly one negative)
    valid = pos != 0
    zp = (P * Tp).sum(1)[valid]
    zn = (P @ S.T).squeeze(1)[valid] + (P * C_).sum(1)[valid]
    logits = torch.cat([zp, zn])
    labels = torch.cat([torch.ones_like(zp), torch.zeros_like(zn)])
    want = F.binary_cross_entropy_with_logits(logits, labels, reduction="sum") / valid.sum()
    got = ref_bce(P, Tp, pos, S, s, n_items, ops.sampled_bce_beta(1, n_items, 0.0), C_)
    assert float(got) == pytest.approx(float(want), rel=1e-12)
