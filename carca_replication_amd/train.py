"""Train / evaluate driver with the reference's contract (src/train.py of r-papso/carca-replication).

Same function names, arguments, return values, console lines and `;`-separated CSV log as the reference
(train.py:56-152), so `scripts/training.py:176-186` drives it unchanged.  What differs underneath:
  * every batch runs the HIP path (engine.train_step / engine.eval_batch);
  * HR@k / NDCG@k come from a sort-free rank count on the device (carca_rank_metrics) and all per-batch
    `.item()` syncs (train.py:21,32,47,97) are gone: sums stay on the device until an epoch / evaluation ends;
  * the best checkpoint keeps the reference's file name (`<epoch>_<HR>_<NDCG>.pth`, train.py:118-124) but holds
    state_dicts -- model, optimizer, scheduler, epoch, metrics -- instead of a pickled module: it reloads with
    torch.load(weights_only=True) (the reference's bare torch.load of a pickled module, train.py:141-142, raises on
    torch >= 2.6), survives refactors of the module classes, and `resume=` continues a run from it.
    load_checkpoint() still accepts the reference's pickled-module files.
"""
from __future__ import annotations

import os
from datetime import datetime
from typing import Tuple, Union

import torch
from torch.optim import Optimizer
from torch.optim.lr_scheduler import _LRScheduler
from torch.utils.data import DataLoader

from . import engine, ops
from ._lib import CarcaHipError
from .modules import Model, to


CHECKPOINT_FORMAT = "carca-state-dict-v1"


def save_checkpoint(path: str, model: Model, optim: Optimizer = None, scheduler=None, **meta) -> None:
    """state_dict checkpoint: tensors + plain python values only, so that
    torch.load(path, weights_only=True) reads it back."""
    ck = {"format": CHECKPOINT_FORMAT, "model": model.state_dict(), "meta": dict(meta)}
    if optim is not None:
        ck["optimizer"] = optim.state_dict()
    if scheduler is not None:
        ck["scheduler"] = scheduler.state_dict()
    tmp = path + ".tmp"
    torch.save(ck, tmp)
    os.replace(tmp, path)  # (an interrupted save never leaves a truncated best checkpoint behind)


def load_checkpoint(path: str, model: Model, optim: Optimizer = None, scheduler=None, device=None,
                    allow_pickle: bool = False) -> dict:
    """Loads `path` into model (and optimizer / scheduler when given and stored); returns the checkpoint's meta dict.
    The file is read with torch.load(weights_only=True): nothing in it is executed, and a truncated or foreign file
    raises.  allow_pickle=True (opt-in, for files the caller trusts) also accepts what the reference writes --
    torch.save(model), a pickled module (train.py:124) -- and copies its parameters; unpickling runs code from the file."""
    if allow_pickle:
        try:
            ck = torch.load(path, map_location=device, weights_only=True)
        except Exception:
            ck = torch.load(path, map_location=device, weights_only=False)
    else:
        ck = torch.load(path, map_location=device, weights_only=True)
    if isinstance(ck, torch.nn.Module):
        model.load_state_dict(ck.state_dict())
        return {}
    if not isinstance(ck, dict) or ck.get("format") != CHECKPOINT_FORMAT:
        raise ValueError(f"{path}: not a {CHECKPOINT_FORMAT} checkpoint")
    model.load_state_dict(ck["model"])
    if optim is not None and "optimizer" in ck:
        optim.load_state_dict(ck["optimizer"])
    if scheduler is not None and "scheduler" in ck:
        scheduler.load_state_dict(ck["scheduler"])
    return ck.get("meta", {})


def _positive_columns(y_true: torch.Tensor) -> torch.Tensor:
    return y_true.argmax(dim=1).to(torch.int32)


def compute_HR(y_pred: torch.Tensor, y_true: torch.Tensor, k: int) -> float:
    """Number of rows whose positive (the 1 in y_true) ranks in the top k (train.py:15-21), tie-free scores."""
    sums, _ = ops.rank_metrics(y_pred, k, pos=_positive_columns(y_true))
    return float(sums[0])


def compute_NDCG(y_pred: torch.Tensor, y_true: torch.Tensor, k: int) -> float:
    """Sum over rows of 1 / log2(rank + 2) for positives ranked in the top k (train.py:24-32)."""
    sums, _ = ops.rank_metrics(y_pred, k, pos=_positive_columns(y_true))
    return float(sums[1])


def evaluate(model: Model, loader: DataLoader, device: str, k: int) -> Tuple[float, float, float]:
    """(HR@k, NDCG@k, mean batch loss) over the loader (train.py:35-53); one host sync at the end.
    The loader yields the reference's 7-tuples, ids-only 5-tuples (CARCADataset(with_attrs=False)) or is a
    device_data.DeviceLoader (batches built in HBM; the model needs its attribute table: register_attr_table)."""
    model = model.eval().to(device)
    sums = torch.zeros(5, dtype=torch.float32, device=device)
    n_batches = 0
    with torch.no_grad():
        for batch in loader:
            engine.eval_batch(model, to(*engine.as_batch7(batch), device=device), k=k, sums=sums)
            n_batches += 1
    hr, ndcg, _ties, loss_sum, users = (float(v) for v in sums.cpu())
    if torch.device(device).type == "cuda":
        ops.poll_errors()  # (the epoch's only host sync just happened: a kernel-side failure of any batch surfaces here)
    return hr / users, ndcg / users, loss_sum / max(n_batches, 1)


def _candidate_set(model, method: str, candidates, device):
    """candidates of evaluate_full / evaluate_full_ranks -> None or a catalogue.CandidateSet on `device`, built once for
    the whole evaluation; a model whose `method` has no candidates argument (KNN) cannot be restricted."""
    import inspect

    from .catalogue import CandidateSet

    if candidates is None:
        return None
    if "candidates" not in inspect.signature(getattr(model, method)).parameters:
        raise CarcaHipError(f"evaluate_full: {type(model).__name__}.{method} takes no candidate set (candidates= is "
                            "CARCA's; pass candidates=None)")
    if not isinstance(candidates, CandidateSet):
        if not isinstance(candidates, torch.Tensor):
            raise CarcaHipError("evaluate_full: candidates must be None, a CandidateSet or a 1-D integer / bool tensor")
        with torch.no_grad():
            n_items = model.embeds.item_table().shape[0]  # (the table the calls below score against, cached)
        candidates = CandidateSet(candidates, n_items, device=device)
    return candidates.to(device)


def _wide_envelope(model, method: str) -> dict:
    """The keyword that lets CARCA.recommend / rank_items take profiles of more than 64 slots and encoder geometries
    with no fused kernel (allow_composed=True; inside the fused envelope it routes to the same kernels), for a model
    whose `method` has it (KNN has no such limit and no such keyword)."""
    import inspect

    return {"allow_composed": True} if "allow_composed" in inspect.signature(getattr(model, method)).parameters else {}


def evaluate_full(model: Model, loader: DataLoader, device: str, k: int, candidates=None) -> Tuple[float, float]:
    """(HR@k, NDCG@k) with the positive o_x[:, 0] ranked against EVERY item of the catalogue instead of the loader's
    sampled negatives (full-ranking protocol; Krichene & Rendle, KDD 2020).  Per batch: model.recommend (CARCA.recommend or
    KNN.recommend) with the positive's context o_c[:, 0] (data.py:185) and the profile's items minus the positive
    excluded; the positive's rank is its position in the top-k list (ties: the smaller id first).  Same loaders as
    evaluate(); one host sync at the end.
    candidates: None, or the item set S the ranking is restricted to (catalogue.CandidateSet, or a raw tensor normalised
    once here; CARCA only): the positive is ranked among S, and a user whose positive is not in S is left out of the
    sums and of the user count (membership is tested on the device, no extra sync)."""
    model = model.eval().to(device)
    cand = _candidate_set(model, "recommend", candidates, device)
    wide = _wide_envelope(model, "recommend")
    sums = torch.zeros(3, dtype=torch.float32, device=device)
    with torch.no_grad():
        for batch in loader:
            p_x, p_a, p_c, o_x, _o_a, o_c, _y = to(*engine.as_batch7(batch), device=device)
            pos = o_x[:, :1].to(torch.int64)
            excl = torch.where(p_x.to(torch.int64) == pos, torch.zeros_like(pos), p_x.to(torch.int64))
            if cand is None:
                _, ids = model.recommend((p_x, p_a, p_c), o_c[:, 0], k=k, exclude=excl, **wide)
                users = ids.shape[0]
            else:  # (a positive outside S is never in the list: it only has to leave the user count)
                _, ids = model.recommend((p_x, p_a, p_c), o_c[:, 0], k=k, exclude=excl, candidates=cand, **wide)
                users = cand.contains(pos).sum()
            hit = ids == pos
            rank = torch.arange(k, device=ids.device, dtype=torch.float32).expand_as(ids)
            sums[0] += hit.sum()
            sums[1] += (hit.to(torch.float32) / torch.log2(rank + 2.0)).sum()
            sums[2] += users
    hr, ndcg, users = (float(v) for v in sums.cpu())
    if torch.device(device).type == "cuda":
        ops.poll_errors()
    return hr / max(users, 1.0), ndcg / max(users, 1.0)


def evaluate_listed(model: Model, loader: DataLoader, device: str, k: int) -> Tuple[float, float]:
    """(HR@k, NDCG@k) under the loader's own protocol -- the positive o_x[:, 0] against the sampled negatives o_x[:, 1:]
    (data.py:180-185) -- served from the per-item tables: per batch model.recommend_from((p_x, p_a, p_c), o_c[:, 0], o_x,
    k, exclude=None), the positive's rank being its position in the returned list (ties: the smaller id first; a
    negative that repeats the positive is the same item).  What evaluate() measures through forward, without the
    feature GEMM over the candidates.  Same loaders as evaluate(); sums stay on the device, one host sync at the end."""
    model = model.eval().to(device)
    wide = _wide_envelope(model, "recommend_from")
    sums = torch.zeros(3, dtype=torch.float32, device=device)
    with torch.no_grad():
        for batch in loader:
            p_x, p_a, p_c, o_x, _o_a, o_c, _y = to(*engine.as_batch7(batch), device=device)
            pos = o_x[:, :1].to(torch.int64)
            _, ids = model.recommend_from((p_x, p_a, p_c), o_c[:, 0], o_x, k=k, exclude=None, **wide)
            hit = (ids == pos) & (pos != 0)
            rank = torch.arange(k, device=ids.device, dtype=torch.float32).expand_as(ids)
            sums[0] += hit.sum()
            sums[1] += (hit.to(torch.float32) / torch.log2(rank + 2.0)).sum()
            sums[2] += ids.shape[0]
    hr, ndcg, users = (float(v) for v in sums.cpu())
    if torch.device(device).type == "cuda":
        ops.poll_errors()
    return hr / max(users, 1.0), ndcg / max(users, 1.0)


def audience(model: Model, loader: DataLoader, device: str, items, k: int = 10
             ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The k best users of the loader for each listed item (CARCA.recommend_users over every batch; DESIGN.md section
    24): (scores [Q, k] float32, users [Q, k] int64, item_ids [Q] int64).  Walks the loader the way evaluate_full does and
    feeds each batch's profile with the held-out context o_c[:, 0] to one catalogue.AudienceTopK; a user's id is its
    running position in the loader, and a user is not eligible for an item of its profile.  items: a CandidateSet or a raw
    tensor normalised once here.  The result does not depend on the loader's batch size.  One host sync at the end."""
    from .catalogue import AudienceTopK

    model = model.eval().to(device)
    if not hasattr(model, "recommend_users"):
        raise CarcaHipError(f"audience: {type(model).__name__} has no recommend_users (the call is CARCA's)")
    n_items = model._catalogue_size()
    with torch.no_grad():
        if n_items is None:
            n_items = model.embeds.item_table().shape[0]  # (the table the updates below score against, cached)
        state = AudienceTopK(items, k, n_items, device=device)
        for batch in loader:
            p_x, p_a, p_c, _o_x, _o_a, o_c, _y = to(*engine.as_batch7(batch), device=device)
            state.update(model, (p_x, p_a, p_c), o_c[:, 0], allow_composed=True, _what="audience")
        out = state.result()
    if torch.device(device).type == "cuda":
        torch.cuda.current_stream().synchronize()
        ops.poll_errors()
    return out


def evaluate_full_diverse(model: Model, loader: DataLoader, device: str, k: int, pool: int = 128, lam: float = 0.7,
                          metric: str = "cosine", candidates=None) -> dict:
    """evaluate_full's protocol over the diversity re-ranked list (model.recommend_diverse: recommend's `pool` best items
    re-ranked by maximal marginal relevance): the positive o_x[:, 0] with its context against the
    catalogue, the profile's other items excluded.  Returns {"HR@k", "NDCG@k", "ILD@k" (the lists' intra-list diversity,
    mean over users), "coverage@k" (distinct recommended ids / (n_items - 1)), "users"}.  With lam = 1 HR and NDCG are
    evaluate_full's.  Sums and the coverage bitmap stay on the device, one host sync at the end.
    candidates: as evaluate_full's (CARCA only); a user whose positive is not in S is left out of every sum."""
    model = model.eval().to(device)
    cand = _candidate_set(model, "recommend_diverse", candidates, device)
    wide = _wide_envelope(model, "recommend_diverse")
    if cand is not None:
        wide["candidates"] = cand
    sums = torch.zeros(4, dtype=torch.float32, device=device)
    seen = None
    with torch.no_grad():
        for batch in loader:
            p_x, p_a, p_c, o_x, _o_a, o_c, _y = to(*engine.as_batch7(batch), device=device)
            pos = o_x[:, :1].to(torch.int64)
            excl = torch.where(p_x.to(torch.int64) == pos, torch.zeros_like(pos), p_x.to(torch.int64))
            _, ids, ild = model.recommend_diverse((p_x, p_a, p_c), o_c[:, 0], k=k, pool=pool, lam=lam, metric=metric,
                                                  exclude=excl, **wide)
            if seen is None:
                n_items = (model.embeds.item_table() if hasattr(model, "embeds") else model._attr_table).shape[0]
                seen = torch.zeros(n_items, dtype=torch.bool, device=ids.device)
            counted = torch.ones_like(pos, dtype=torch.bool) if cand is None else cand.contains(pos)
            hit = (ids == pos) & counted
            rank = torch.arange(k, device=ids.device, dtype=torch.float32).expand_as(ids)
            sums[0] += hit.sum()
            sums[1] += (hit.to(torch.float32) / torch.log2(rank + 2.0)).sum()
            sums[2] += (ild * counted.reshape(-1)).sum()
            sums[3] += counted.sum()
            seen[torch.where(counted, ids, torch.zeros_like(ids)).reshape(-1)] = True
    if seen is None:
        return {f"HR@{k}": 0.0, f"NDCG@{k}": 0.0, f"ILD@{k}": 0.0, f"coverage@{k}": 0.0, "users": 0}
    seen[0] = False  # (id 0 is padding)
    hr, ndcg, ild_sum, users, distinct = (float(v) for v in torch.cat([sums, seen.sum().reshape(1).to(sums.dtype)]).cpu())
    if torch.device(device).type == "cuda":
        ops.poll_errors()
    den = max(users, 1.0)
    return {f"HR@{k}": hr / den, f"NDCG@{k}": ndcg / den, f"ILD@{k}": ild_sum / den,
            f"coverage@{k}": distinct / max(seen.shape[0] - 1, 1), "users": int(users)}


def _rank_sums(ranks: torch.Tensor, ks) -> torch.Tensor:
    """[hits@k for k in ks, dcg@k for k in ks, sum 1/(rank+1), sum rank, users] (float64, on ranks' device) over the
    entries of ranks >= 0 (rank -1 marks an id outside the catalogue and counts nowhere)."""
    r = ranks.reshape(-1).to(torch.float64)
    valid = r >= 0
    r = torch.where(valid, r, torch.zeros_like(r))
    v = valid.to(torch.float64)
    gain = v / torch.log2(r + 2.0)
    parts = [(v * (r < k)).sum() for k in ks] + [(gain * (r < k)).sum() for k in ks]
    parts += [(v / (r + 1.0)).sum(), (v * r).sum(), v.sum()]
    return torch.stack(parts)


def _metrics_from_sums(sums, ks) -> dict:
    vals = [float(x) for x in sums.cpu()]
    n = len(ks)
    users = vals[-1]
    den = max(users, 1.0)
    out = {f"HR@{k}": vals[i] / den for i, k in enumerate(ks)}
    out.update({f"NDCG@{k}": vals[n + i] / den for i, k in enumerate(ks)})
    out.update(MRR=vals[2 * n] / den, mean_rank=vals[2 * n + 1] / den, users=int(users))
    return out


def full_rank_metrics(ranks: torch.Tensor, ks=(1, 5, 10, 20, 50)) -> dict:
    """Full-ranking metrics from 0-based ranks (pure torch, any device): HR@k = share of ranks < k, NDCG@k = mean of
    [rank < k] / log2(rank + 2) (train.py:15-32 with the positive's rank taken over the whole catalogue), MRR = mean of
    1 / (rank + 1), mean_rank, and users; any k >= 1.  Ranks < 0 (ids outside the catalogue) are left out."""
    ks = _check_ks(ks)
    return _metrics_from_sums(_rank_sums(ranks, ks), ks)


def _check_ks(ks):
    ks = tuple(int(k) for k in ks)
    if not ks or min(ks) < 1:
        raise ValueError(f"cutoffs must be integers >= 1, got {ks}")
    return ks


def evaluate_full_ranks(model: Model, loader: DataLoader, device: str, ks=(1, 5, 10, 20, 50), candidates=None) -> dict:
    """evaluate_full's protocol -- the positive o_x[:, 0] with its context o_c[:, 0] against every item, the profile's
    items other than the positive excluded -- in one pass for every cutoff: the positive's exact rank comes from
    model.rank_items (CARCA.rank_items or KNN.rank_items: a count over the catalogue, no top-k list), so any k >= 1 is
    allowed.  Returns {"HR@k", "NDCG@k" for k in ks, "MRR", "mean_rank", "users"} (full_rank_metrics).  Same loaders as
    evaluate(); sums stay on the device, one host sync at the end.
    candidates: as evaluate_full's: the positive's rank is its rank among S, and a user whose positive is not in S is left
    out of the sums and of "users"."""
    ks = _check_ks(ks)
    model = model.eval().to(device)
    cand = _candidate_set(model, "rank_items", candidates, device)
    wide = _wide_envelope(model, "rank_items")
    sums = torch.zeros(2 * len(ks) + 3, dtype=torch.float64, device=device)
    with torch.no_grad():
        for batch in loader:
            p_x, p_a, p_c, o_x, _o_a, o_c, _y = to(*engine.as_batch7(batch), device=device)
            pos = o_x[:, :1].to(torch.int64)
            excl = torch.where(p_x.to(torch.int64) == pos, torch.zeros_like(pos), p_x.to(torch.int64))
            if cand is None:
                _, ranks = model.rank_items((p_x, p_a, p_c), o_c[:, 0], pos, exclude=excl, **wide)
            else:
                _, ranks = model.rank_items((p_x, p_a, p_c), o_c[:, 0], pos, exclude=excl, candidates=cand, **wide)
                ranks = torch.where(cand.contains(pos), ranks, torch.full_like(ranks, -1))  # (_rank_sums skips them)
            sums += _rank_sums(ranks, ks)
    out = _metrics_from_sums(sums, ks)
    if torch.device(device).type == "cuda":
        ops.poll_errors()
    return out


def off_policy_value(model: Model, logs, device: str, temperature: float = 1.0, mode: str = "first", clip=None,
                     exclude="profile", candidates=None, allow_composed: bool = False) -> dict:
    """What logged traffic would have earned under `model` at `temperature`: IPS / SNIPS estimates over a log that
    recommend_sampled wrote.  logs: an iterable of (profile, context, ids, logged_log_probs,
    rewards) batches -- profile and context as recommend_sampled took them, ids and logged_log_probs [B, k] as it
    returned them, rewards [B], or [B, k]: summed over the list for mode "list", column 0 read for mode "first".  Per
    batch: model.log_prob_items(profile, context, ids, temperature, exclude, candidates) for the target's side,
    catalogue.policy_log_ratio's ratio (mode as there) and off_policy_estimate's sums.  exclude and candidates must be
    what the log was drawn under.  The sums stay on the device in float64; one host sync at the end, where a logged
    -inf under a finite target raises as policy_log_ratio does.  -> off_policy_estimate's dict, as Python floats (n an
    int)."""
    from . import catalogue

    if mode not in ("first", "list"):
        raise CarcaHipError(f'off_policy_value: mode must be "first" or "list", got {mode!r}')
    model = model.eval().to(device)
    wide = {"allow_composed": True} if allow_composed and _wide_envelope(model, "log_prob_items") else {}
    sums = torch.zeros(5, dtype=torch.float64, device=device)
    bad = torch.zeros((), dtype=torch.bool, device=device)
    with torch.no_grad():
        for profile, context, ids, logged, rewards in logs:
            profile = to(*profile, device=device)
            context, ids, logged, rewards = to(context, ids, logged, rewards, device=device)
            target, _, _ = model.log_prob_items(profile, context, ids, temperature=temperature, exclude=exclude,
                                                candidates=candidates, **wide)
            ratio, b = catalogue._policy_log_ratio(target, logged, mode)
            if rewards.dim() == 2:
                rewards = rewards.to(torch.float64).sum(1) if mode == "list" else rewards[:, 0]
            part = catalogue._off_policy_sums(ratio, rewards, clip)
            sums = torch.cat([sums[:3] + part[:3], torch.maximum(sums[3], part[3]).reshape(1), (sums[4] + part[4]).reshape(1)])
            bad |= b
    host = torch.cat([sums, bad.to(torch.float64).reshape(1)]).cpu()  # (the host sync)
    vals = {k: float(v) for k, v in catalogue._off_policy_result(host[:5], clip).items() if k != "clip"}
    if torch.device(device).type == "cuda":
        ops.poll_errors()
    if bool(host[5]):
        raise CarcaHipError(catalogue._RATIO_UNDRAWN.replace("policy_log_ratio", "off_policy_value", 1))
    vals["n"], vals["clip"] = int(vals["n"]), clip
    return vals


def train_off_policy(model: Model, logs, device: str, optim: Optimizer, epochs: int, temperature: float = 1.0,
                     kind: str = "ips", clip=None, exclude="profile", entropy_coef: float = 0.0) -> list:
    """Train `model` on a log that recommend_sampled wrote: engine.off_policy_step over every
    batch of `logs` (off_policy_value's tuples; a re-iterable) for `epochs` epochs.  The model's mode is the caller's
    (dropout follows model.training).  One host sync per epoch, where a logged -inf on a valid row raises.  -> the mean
    objective of each epoch, as Python floats."""
    from . import catalogue
    from .engine import off_policy_step

    model = model.to(device)
    out = []
    for _ in range(epochs):
        total = torch.zeros((), dtype=torch.float64, device=device)
        bad = torch.zeros((), dtype=torch.bool, device=device)
        n = 0
        for profile, context, ids, logged, rewards in logs:
            profile = to(*profile, device=device)
            context, ids, logged, rewards = to(context, ids, logged, rewards, device=device)
            total = total + off_policy_step(model, optim, (profile, context, ids, logged, rewards), temperature, kind, clip,
                                            exclude, entropy_coef, undrawn=bad)
            n += 1
        host = torch.stack([total, bad.to(torch.float64)]).cpu()  # (the host sync)
        if bool(host[1]):
            raise CarcaHipError(catalogue._OBJECTIVE_UNDRAWN.replace("policy_objective", "train_off_policy", 1))
        out.append(float(host[0]) / max(n, 1))
    return out


def train_hard_negatives(model: Model, train_loader, device: str, optim: Optimizer, epochs: int, miner) -> list:
    """Train `model` with the softmax over mined per-user negatives: engine.hard_negative_step over
    every batch of `train_loader` (the training loader's 7- or 5-tuples; a re-iterable) for `epochs` epochs, `miner` a
    sampling.HardNegativeMiner.  The model's mode is the caller's (dropout follows model.training; mining switches to
    eval for its own call).  Every step mines with the current weights, so it rebuilds the item-side tables and syncs
    once; the loss is read once per epoch.  -> the mean loss of each epoch, as Python floats."""
    model = model.to(device)
    out = []
    for _ in range(epochs):
        total = torch.zeros((), dtype=torch.float64, device=device)
        n = 0
        for batch in train_loader:
            dev_batch = to(*engine.as_batch7(batch), device=device)
            total = total + engine.hard_negative_step(model, optim, dev_batch, miner)
            n += 1
        out.append(float(total) / max(n, 1))  # (the epoch's host sync)
    return out


def train(model: Model, train_loader: DataLoader, val_loader: DataLoader, test_loader: DataLoader, device: str,
          optim: Optimizer, epochs: int, top_k: int = 10, verbose: int = 1, early_stop: int = 10,
          datadir: str = "model", scheduler: Union[_LRScheduler, None] = None, graphed: bool = False,
          resume: Union[str, None] = None, resume_trusted: bool = False, loss: str = "bce", sampler=None) -> Model:
    """src/train.py:56-152.  optim: any torch optimizer; optim.Adam / optim.AdamW step in one launch and clip by global
    gradient norm inside the step when built with max_grad_norm -- nothing to pass here.
    Extensions, off by default:
    graphed: batches of the first batch's shape replay their forward + backward from one hipGraph
      (engine.GraphedTrainStep); any other shape (a short last batch) takes the eager step;
    resume: path of a checkpoint written by an earlier run (save_checkpoint): model, optimizer and scheduler state are
      restored and the epoch count continues after the stored one, with the stored best NDCG as the bar to beat;
    resume_trusted: the file named by `resume` may be a whole-module pickle as the reference writes them (train.py:124):
      load_checkpoint(allow_pickle=True) -- unpickling executes code from the file, so only for files the caller trusts;
    loss: "bce" (the reference's objective), "softmax" (full-catalogue softmax cross-entropy, engine.train_step),
      "sampled_softmax" (softmax over K shared samples with the logQ correction) or "sampled_bce" (the sigmoid objective
      against K shared negatives, gBCE); only "bce" with graphed=True.  Validation and test stay
      the reference's sampled HR / NDCG either way;
    sampler: the sampled losses only: the proposal the samples are drawn from (sampling.ItemSampler; None = uniform,
      K = min(8192, n_items - 1) for "sampled_softmax", min(256, n_items - 1) for "sampled_bce", which takes a uniform
      sampler only)."""
    objective = loss  # (`loss` names the validation loss below, as in the reference's loop)
    if objective not in engine.LOSSES:
        raise ValueError(f"train: loss must be one of {engine.LOSSES}, got {objective!r}")
    if sampler is not None and objective not in engine.SAMPLED_LOSSES:
        raise ValueError(f'train: a sampler is only read by loss="sampled_softmax" and "sampled_bce", got loss={objective!r}')
    if objective == "sampled_bce":
        engine._check_uniform(sampler, "train")
    if graphed and objective != "bce":
        raise CarcaHipError(f'train: graphed=True captures the BCE step only; loss="{objective}" runs eagerly '
                           '(graphed=False)')
    os.makedirs(datadir, exist_ok=True)
    model = model.train().to(device)
    best, stale, first_epoch = 0.0, 0, 1
    best_path = None  # the checkpoint holding the best weights so far: a resumed run starts with the one it resumes from
    if resume is not None:
        meta = load_checkpoint(resume, model, optim, scheduler, device=device, allow_pickle=resume_trusted)
        best, first_epoch = float(meta.get("NDCG", 0.0)), int(meta.get("epoch", 0)) + 1
        stale, best_path = int(meta.get("stale", 0)), resume
    t0 = datetime.now()
    log = open(f"./{datadir}/{t0.year}-{t0.month}-{t0.day}T{t0.hour}-{t0.minute}-{t0.second}.csv", "a")
    now = lambda: datetime.now().strftime("%H:%M:%S")  # noqa: E731
    epoch = first_epoch - 1
    captured = None
    for epoch in range(first_epoch, epochs + 1):
        loss_sum = torch.zeros((), dtype=torch.float32, device=device)
        for i, batch in enumerate(train_loader, start=1):
            dev_batch = to(*engine.as_batch7(batch), device=device)
            if graphed:
                sig = tuple(None if t is None else (tuple(t.shape), t.dtype) for t in dev_batch)
                if captured is None:
                    captured = (sig, engine.GraphedTrainStep(model, optim, dev_batch))
            if graphed and captured[0] == sig:
                loss_sum += captured[1](dev_batch)
            else:
                loss_sum += engine.train_step(model, optim, dev_batch, loss=objective, sampler=sampler)
            if verbose == 2:  # the reference prints a running mean per batch; that costs a sync per batch here too
                print(f"{now()} - Batch {i:03d}: Loss = {(float(loss_sum) / i):.4f}")
        mean_loss = float(loss_sum) / len(train_loader)
        if verbose in (1, 2):
            print(f"{now()} - Epoch {epoch:03d}: Train Loss = {mean_loss:.4f}")
            log.write(f"{now()};{epoch};train;{mean_loss};;\n")
        if scheduler is not None:
            scheduler.step()

        HR, NDCG, loss = evaluate(model, val_loader, device, top_k)
        model = model.train().to(device)
        if NDCG > best:
            for f in os.listdir(datadir):
                if f.endswith(".pth"):
                    os.remove(os.path.join(datadir, f))
            best, stale = NDCG, 0
            best_path = os.path.join(datadir, f"{epoch:03d}_{HR:.4f}_{NDCG:.4f}.pth")
            save_checkpoint(best_path, model, optim, scheduler,
                            epoch=epoch, HR=float(HR), NDCG=float(NDCG), val_loss=float(loss), stale=0)
        else:
            stale += 1
        if verbose in (1, 2):
            print(f"{now()} - Epoch {epoch:03d}: Val Loss = {loss:.4f} HR = {HR:.4f}, NDCG = {NDCG:.4f}")
            log.write(f"{now()};{epoch};val;{loss};{HR};{NDCG}\n")
        if stale >= early_stop:
            print(f"No improvement in {stale} epochs, early stopping...")
            break
        log.flush()

    if best_path is not None and os.path.exists(best_path):
        # the best epoch's weights (train.py:141-142) -- of THIS run, or the checkpoint it resumed from when no epoch
        # beat it; the optimizer keeps the last epoch's state
        load_checkpoint(best_path, model, device=device)
        model = model.to(device)
    if test_loader is not None:
        HR, NDCG, loss = evaluate(model, test_loader, device, top_k)
        print(f"{now()} - Epoch {epoch:03d}: Test Loss = {loss:.4f} HR = {HR:.4f}, NDCG = {NDCG:.4f}")
        log.write(f"{now()};{epoch};test;{loss};{HR};{NDCG}\n")
    log.close()
    return model
