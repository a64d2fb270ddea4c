"""Proposal distributions for the sampled softmax (ops.sampled_xent, CARCA.sampled_softmax_loss).

ItemSampler draws K item ids i.i.d. with replacement from a proposal Q over [1, n_items) on the device, from torch's
generator (torch.manual_seed repeats a run), and gives log Q for the logQ correction.  Sampling is not on the hot path:
torch.randint for the uniform proposal, torch.searchsorted over a cached CDF otherwise."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor


class ItemSampler:
    """Q uniform over [1, n_items) when counts is None; otherwise Q(i) proportional to (counts[i] + 1) ** alpha for
    i >= 1 (every id >= 1 has Q > 0; alpha = 0 is uniform, alpha = 1 the popularity).  Id 0 is never drawn.
    counts: [n_items] non-negative (counts[0] is ignored).  n_samples: K, the ids each sample() returns."""

    def __init__(self, n_items: int, n_samples: int, counts: Optional[Tensor] = None, alpha: float = 1.0,
                 device=None):
        if int(n_items) < 2:
            raise ValueError(f"ItemSampler: n_items must be at least 2 (ids 1 .. n_items-1), got {n_items}")
        if int(n_samples) < 1:
            raise ValueError(f"ItemSampler: n_samples must be positive, got {n_samples}")
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.n_items, self.n_samples, self.device = int(n_items), int(n_samples), torch.device(device)
        self.alpha = float(alpha)
        self._cdf = None
        if counts is None:
            q = torch.full((self.n_items - 1,), 1.0 / (self.n_items - 1), dtype=torch.float64)
        else:
            c = torch.as_tensor(counts).detach().to("cpu", torch.float64).reshape(-1)
            if c.numel() != self.n_items:
                raise ValueError(f"ItemSampler: counts must have n_items = {self.n_items} entries, got {c.numel()}")
            if bool((c[1:] < 0).any()) or not bool(torch.isfinite(c).all()):
                raise ValueError("ItemSampler: counts must be finite and non-negative")
            w = (c[1:] + 1.0) ** self.alpha
            q = w / w.sum()
            cdf = torch.cumsum(q, 0)
            cdf[-1] = 1.0  # (a uniform draw u < 1 always lands on an id < n_items)
            self._cdf = cdf.to(self.device)
        lq = torch.empty(self.n_items, dtype=torch.float64)
        lq[0] = -float("inf")
        lq[1:] = torch.log(q)
        self._log_q = lq.to(torch.float32).to(self.device)

    def log_q(self) -> Tensor:
        """[n_items] fp32 on the sampler's device: log Q(i), -inf at id 0."""
        return self._log_q

    def sample(self) -> Tensor:
        """[n_samples] int64 ids in [1, n_items), drawn i.i.d. from Q on the device with torch's generator."""
        if self._cdf is None:
            return torch.randint(1, self.n_items, (self.n_samples,), device=self.device)
        u = torch.rand(self.n_samples, dtype=torch.float64, device=self.device)
        return torch.searchsorted(self._cdf, u, right=True) + 1
