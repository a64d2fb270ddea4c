"""train.full_rank_metrics (the aggregation behind train.evaluate_full_ranks) against the reference's own formulas
(train.py:15-32: sort the row, gather the labels, HR = positives in the first k columns, NDCG = sum of 1 / log2(rank + 2)
over them), applied to tie-free score matrices over all columns, for cutoffs on both sides of 128; MRR directly."""
import math

import pytest
import torch

from carca_replication_amd.train import full_rank_metrics


def _reference_hr_ndcg(y_pred, y_true, k):
    _, idxs = torch.sort(y_pred, descending=True)
    y_true_sort = torch.gather(y_true, dim=1, index=idxs)
    top_k = y_true_sort[:, :k]
    ranks = torch.nonzero(top_k)[:, 1]
    return float(torch.sum(top_k)), float(torch.sum(1.0 / torch.log2(ranks.to(torch.float64) + 2)))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_full_rank_metrics_match_reference_formulas(seed):
    gen = torch.Generator().manual_seed(seed)
    B, n = 300, 700
    y = torch.randperm(B * n, generator=gen).reshape(B, n).to(torch.float64)  # distinct scores: no ties
    pos = torch.randint(0, n, (B,), generator=gen)
    y_true = torch.zeros(B, n, dtype=torch.int64)
    y_true[torch.arange(B), pos] = 1
    ranks = (y > y[torch.arange(B), pos].unsqueeze(1)).sum(1)  # 0-based rank of the positive among every column
    ks = (1, 5, 10, 20, 50, 128, 129, 400, n)
    got = full_rank_metrics(ranks, ks)
    assert got["users"] == B
    for k in ks:
        hr, ndcg = _reference_hr_ndcg(y, y_true, k)
        assert got[f"HR@{k}"] == pytest.approx(hr / B, abs=1e-12)
        assert got[f"NDCG@{k}"] == pytest.approx(ndcg / B, abs=1e-12)
    assert got[f"HR@{n}"] == 1.0
    mrr = sum(1.0 / (int(r) + 1) for r in ranks) / B
    assert got["MRR"] == pytest.approx(mrr, abs=1e-12)
    assert got["mean_rank"] == pytest.approx(float(ranks.double().mean()), abs=1e-9)


def test_full_rank_metrics_edge_cases():
    ranks = torch.tensor([[0, -1], [3, 127], [128, 1_000_000]])
    got = full_rank_metrics(ranks, ks=(1, 128, 129))
    assert got["users"] == 5  # rank -1 (an id outside the catalogue) counts nowhere
    assert got["HR@1"] == pytest.approx(1 / 5)
    assert got["HR@128"] == pytest.approx(3 / 5)
    assert got["HR@129"] == pytest.approx(4 / 5)
    assert got["NDCG@129"] == pytest.approx((1 + 1 / math.log2(5) + 1 / math.log2(129) + 1 / math.log2(130)) / 5)
    assert got["MRR"] == pytest.approx((1 + 1 / 4 + 1 / 128 + 1 / 129 + 1 / 1_000_001) / 5)
    with pytest.raises(ValueError):
        full_rank_metrics(ranks, ks=(0, 5))
    assert full_rank_metrics(torch.full((4,), -1), ks=(1,))["users"] == 0
