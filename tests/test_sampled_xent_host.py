"""The host side of the sampled softmax, on the CPU: the proposal sampler (sampling.ItemSampler),
the kernels' sizing (ops.sampled_xent_plan), the argument errors of ops.sampled_xent, and the identity the GPU tests build
on -- with every id sampled once under a uniform Q, the logQ-corrected sampled softmax is the full softmax of section 13."""
import math

import pytest
import torch
import torch.nn.functional as F

from carca_replication_amd import CarcaHipError, engine, ops
from carca_replication_amd.sampling import ItemSampler


def test_log_q_normalises_over_ids_from_one():
    counts = torch.tensor([1e6, 0, 3, 10, 0, 7, 100])
    for alpha in (1.0, 0.5, 2.0):
        s = ItemSampler(7, 4, counts=counts, alpha=alpha, device="cpu")
        lq = s.log_q()
        assert lq.dtype == torch.float32 and lq.shape == (7,)
        assert lq[0].item() == -math.inf
        assert abs(float(lq[1:].double().exp().sum()) - 1.0) < 1e-6
        want = (counts[1:].double() + 1) ** alpha
        assert torch.allclose(lq[1:].double(), torch.log(want / want.sum()), atol=1e-6)
    u = ItemSampler(7, 4, device="cpu").log_q()
    assert u[0].item() == -math.inf and torch.allclose(u[1:], torch.full((6,), -math.log(6.0)))


def test_alpha_zero_is_the_uniform_proposal():
    counts = torch.randint(0, 1000, (50,))
    a = ItemSampler(50, 8, counts=counts, alpha=0.0, device="cpu").log_q()
    b = ItemSampler(50, 8, device="cpu").log_q()
    assert torch.allclose(a[1:], b[1:], atol=1e-6) and a[0].item() == b[0].item() == -math.inf


def test_sampler_draws_lie_in_range_and_repeat_under_a_seed():
    for counts in (None, torch.arange(30) ** 2):
        s = ItemSampler(30, 5000, counts=counts, device="cpu")
        torch.manual_seed(4)
        a = s.sample()
        torch.manual_seed(4)
        b = s.sample()
        assert a.shape == (5000,) and torch.equal(a, b)
        assert int(a.min()) >= 1 and int(a.max()) < 30


def test_sampler_errors():
    with pytest.raises(ValueError):
        ItemSampler(1, 4)
    with pytest.raises(ValueError):
        ItemSampler(10, 0)
    with pytest.raises(ValueError):
        ItemSampler(10, 4, counts=torch.ones(9), device="cpu")
    with pytest.raises(ValueError):
        ItemSampler(10, 4, counts=-torch.ones(10), device="cpu")


def test_plan_split_counts_and_scratch():
    for R, K, d in [(6400, 65536, 128), (6400, 8192, 90), (1, 1, 64), (17, 63, 90), (3400, 8192, 192),
                    (100_000, 1000, 256), (1, 65, 256)]:
        p = ops.sampled_xent_plan(R, K, d, n_cus=256)
        per, s_s, s_r = p["samples_per_split"], p["splits_samples"], p["splits_rows"]
        assert per % 64 == 0 and per * s_s >= K and (s_s - 1) * per < K  # covers K, no empty split
        assert 1 <= s_s <= 256 and 1 <= s_r <= 256
        ldo = (d + 3) // 4 * 4
        r64 = lambda n: (n + 63) // 64 * 64  # noqa: E731
        head = 2 * r64(R) + 64
        assert p["scratch_fwd"] == head + 2 * r64(s_s * R)
        assert p["scratch_bwd"] == head + r64((s_s + 1) * R * ldo) + (r64(s_r * K * ldo) if s_r > 1 else 0)
    # hand-computed against csrc/sampled_xent.hip's SxLayout: 2 ceil64(R) + 64 words of row lists, then 2 ceil64(s_s R)
    # (max, sum) words, or ceil64((s_s + 1) R ld) dP words and, with s_r > 1, ceil64(s_r K ld) dS words
    hand = {(6400, 8192, 128): (11, 768, 8, 12864 + 140800, 12864 + 9830400 + 8388608),
            (6400, 65536, 128): (11, 6016, 1, 12864 + 140800, 12864 + 9830400),
            (17, 63, 90): (1, 64, 1, 192 + 128, 192 + 3136),
            (1, 1, 64): (1, 64, 1, 320, 320)}
    for (R, K, d), want in hand.items():
        p = ops.sampled_xent_plan(R, K, d, n_cus=256)
        assert (p["splits_samples"], p["samples_per_split"], p["splits_rows"], p["scratch_fwd"], p["scratch_bwd"]) == want
    big = ops.sampled_xent_plan(6400, 65536, 128, n_cus=256)
    assert max(big["scratch_fwd"], big["scratch_bwd"]) * 4 < 0.1 * 6400 * 65536 * 4  # far below one [R, K] buffer
    assert big["splits_samples"] * 100 >= 1024  # the forward's grid fills the chip (4 workgroups per CU)
    with pytest.raises(CarcaHipError):
        ops.sampled_xent_plan(0, 10, 8)
    with pytest.raises(CarcaHipError):
        ops.sampled_xent_plan(10, 0, 8)


def test_op_argument_errors():
    P, Tp, S = torch.zeros(5, 8), torch.zeros(5, 8), torch.zeros(7, 8)
    pos, s, lq = torch.ones(5, dtype=torch.int64), torch.ones(7, dtype=torch.int64), torch.zeros(10)
    with pytest.raises(CarcaHipError, match="expected P"):
        ops.sampled_xent(P, Tp[:4], pos, S, s, lq)
    with pytest.raises(CarcaHipError, match="expected P"):
        ops.sampled_xent(P, Tp, pos, S[:, :6], s, lq)
    with pytest.raises(CarcaHipError, match="entries"):
        ops.sampled_xent(P, Tp, pos[:4], S, s, lq)
    with pytest.raises(CarcaHipError, match="entries"):
        ops.sampled_xent(P, Tp, pos, S, s[:6], lq)
    with pytest.raises(CarcaHipError, match="integer"):
        ops.sampled_xent(P, Tp, pos.float(), S, s, lq)
    with pytest.raises(CarcaHipError, match="log_q"):
        ops.sampled_xent(P, Tp, pos, S, s, lq.view(2, 5))
    with pytest.raises(CarcaHipError, match="sampled_xent: P, Tp and S must be float32"):
        ops.sampled_xent(P.double(), Tp, pos, S, s, lq)
    with pytest.raises(CarcaHipError, match="CPU"):  # no CPU implementation: the op runs on the GPU only
        ops.sampled_xent(P, Tp, pos, S, s, lq)


def test_engine_knows_the_sampled_loss():
    assert "sampled_softmax" in engine.LOSSES and engine.SAMPLED_DEFAULT_K == 8192


def test_a_sampler_is_refused_for_the_other_losses(tmp_path):
    from carca_replication_amd.train import train

    sampler = ItemSampler(10, 4, device="cpu")
    batch = tuple(torch.zeros(1, 2) for _ in range(7))
    for loss in ("bce", "softmax"):
        with pytest.raises(ValueError, match="sampler"):
            engine.train_step(None, None, batch, loss=loss, sampler=sampler)
        with pytest.raises(ValueError, match="sampler"):
            train(model=None, train_loader=None, val_loader=None, test_loader=None, device="cpu", optim=None, epochs=1,
                  datadir=str(tmp_path), loss=loss, sampler=sampler)


def _sampled_ref(P, Tp, pos, S, s, log_q):
    n, K = log_q.numel(), s.numel()
    valid = (pos >= 1) & (pos < n)
    s_ok = (s >= 1) & (s < n)
    bs = torch.where(s_ok, -(log_q[torch.where(s_ok, s, 0)] + math.log(K)), torch.zeros((), dtype=P.dtype))
    pv = pos[valid]
    zp = (P[valid] * Tp[valid]).sum(1) - (log_q[pv] + math.log(K))
    zs = (P[valid] @ S.T + bs).masked_fill(~(s_ok.view(1, -1) & (s.view(1, -1) != pv.view(-1, 1))), -math.inf)
    return (torch.logsumexp(torch.cat([zp.view(-1, 1), zs], 1), 1) - zp).mean()


def test_every_sample_under_uniform_q_is_the_full_softmax():
    g = torch.Generator().manual_seed(0)
    n, d, R = 40, 8, 30
    P = torch.randn(R, d, generator=g, dtype=torch.float64)
    T = torch.randn(n, d, generator=g, dtype=torch.float64)
    pos = torch.randint(0, n, (R,), generator=g)
    s = torch.arange(1, n)
    log_q = torch.full((n,), -math.log(n - 1), dtype=torch.float64)
    log_q[0] = -math.inf
    valid = (pos >= 1) & (pos < n)
    full = F.cross_entropy(P[valid] @ T[1:].T, pos[valid] - 1)
    assert abs(_sampled_ref(P, T[pos], pos, T[s], s, log_q).item() - full.item()) < 1e-12
