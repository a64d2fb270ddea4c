"""Proposal distributions for the sampled softmax (ops.sampled_xent, CARCA.sampled_softmax_loss).

ItemSampler draws K item ids i.i.d. with replacement from a proposal Q over [1, n_items) on the device, from torch's
generator (torch.manual_seed repeats a run), and gives log Q for the logQ correction.  Sampling is not on the hot path:
torch.randint for the uniform proposal, torch.searchsorted over a cached CDF otherwise.

HardNegativeMiner builds per-user negative lists for CARCA.listed_softmax_loss from the model's own
ranking: CARCA.retrieve's top items per user, minus the user's history and positives."""
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


class HardNegativeMiner:
    """Per-user hard negatives for CARCA.listed_softmax_loss: the n_hard items the current model ranks highest for each
    user after the first skip_top (the very top of a ranking holds the most false negatives), followed by n_uniform ids
    drawn uniformly from [1, n_items) with torch's generator.  skip_top + n_hard <= catalogue.RETRIEVE_KMAX."""

    def __init__(self, n_hard: int, n_uniform: int = 0, skip_top: int = 0):
        n_hard, n_uniform, skip_top = int(n_hard), int(n_uniform), int(skip_top)
        if n_hard < 0 or n_uniform < 0 or skip_top < 0 or n_hard + n_uniform < 1:
            raise ValueError(f"HardNegativeMiner: n_hard, n_uniform and skip_top must be non-negative with at least one "
                             f"negative per list, got {n_hard}, {n_uniform}, {skip_top}")
        self.n_hard, self.n_uniform, self.skip_top = n_hard, n_uniform, skip_top

    def mine(self, model, profile, pos: Tensor):
        """-> catalogue.NegativeLists of [B, n_hard + n_uniform] for profile = (p_x, p_a, p_c) and the positives pos
        [B, L].  The hard part is model.retrieve(profile, None, k = skip_top + n_hard) with the user's profile items and
        positives excluded (the loss itself removes a slot's own positive; the exclusion removes the user's other
        positives and history), columns skip_top onwards; users with fewer eligible items get padding.  Runs under
        no_grad with the model in eval mode, its previous mode restored afterwards.  retrieve rebuilds the item-side
        tables once per weight version, so mining after every optimizer step pays that rebuild every step.  Building the
        lists costs one host sync."""
        from .catalogue import NegativeLists

        emb = model.embeds
        n_items = emb.items_embed.num_embeddings if hasattr(emb, "items_embed") else emb.attr_table().shape[0]
        p_x = profile[0]
        B = p_x.shape[0]
        parts = []
        was_training = model.training
        model.eval()
        try:
            with torch.no_grad():
                if self.n_hard > 0:
                    exclude = torch.cat([p_x.reshape(B, -1), pos.reshape(B, -1).to(p_x.dtype)], 1)
                    _, ids = model.retrieve(profile, None, k=self.skip_top + self.n_hard, exclude=exclude)
                    parts.append(ids[:, self.skip_top:].to(torch.int64))
        finally:
            model.train(was_training)
        if self.n_uniform > 0:
            parts.append(torch.randint(1, n_items, (B, self.n_uniform), device=p_x.device))
        return NegativeLists(torch.cat(parts, 1) if len(parts) > 1 else parts[0], n_items)
