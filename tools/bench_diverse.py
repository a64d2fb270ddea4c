"""Diversity re-ranking (CARCA.recommend_diverse / KNN.recommend_diverse / ops.mmr_rerank, csrc/mmr_rerank.hip) timed with
device events at the C2 shapes, B = 128 users, pool P = 128, k = 10, lam = 0.7, metric "cosine":
  carca  12,102 items, n_attrs 4096, d 90, g 450, H 3, 2 blocks: the re-rank runs over the item table (n_cols = 90, the
         LDS-resident instantiation)
  knn    the 12,102 x 4,096 multi-hot attribute table (the streaming instantiation)
Variants, all in ONE process on the same inputs, alternating over --rounds rounds after a warm-up call each (the minimum and
every run are kept):
  recommend_k10      model.recommend(k = 10)                     (untouched code: must keep its time)
  recommend_k128     model.recommend(k = 128)                    (the pool)
  diverse            model.recommend_diverse(k = 10, pool = 128) (pool + re-rank; minus recommend_k128 = the feature's cost)
  rerank             the re-rank alone on recommend_k128's pool, reciprocal norms cached as the models cache them
  aten               the ATen composition on the same pool: gather the pool rows, normalise, bmm, then k rounds of
                     mask / argmax / gather / maximum (no tie rule, no ILD: timing only)
The run also checks that recommend_diverse(lam = 1) returns recommend(k = 10) bit for bit and prints the share of users for
whom the ATen composition picks the same ids as the kernel.
usage: python tools/bench_diverse.py [--reps N] [--rounds N] [--models carca knn] [--out file.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_recommend import _batch, _model, _time  # noqa: E402
from carca_replication_amd import catalogue  # noqa: E402
from carca_replication_amd.modules import KNN  # noqa: E402

B, L, P, K, LAM = 128, 50, 128, 10, 0.7
N_ITEMS, N_ATTRS = 12102, 4096


def _aten(s, ids, X, n_cols, k, lam):
    rows = torch.nn.functional.normalize(X[ids][:, :, :n_cols], dim=2)
    G = torch.bmm(rows, rows.transpose(1, 2))
    live = ids != 0
    lo, hi = s.min(1, keepdim=True).values, s.max(1, keepdim=True).values
    rel = (s - lo) / (hi - lo)
    ar = torch.arange(s.shape[0], device=s.device)
    M = torch.zeros_like(s)
    picks = []
    for t in range(k):
        pick = (lam * rel - (1.0 - lam) * M).masked_fill(~live, float("-inf")).argmax(1)
        picks.append(pick)
        sim = G[ar, :, pick]
        M = sim if t == 0 else torch.maximum(M, sim)
        live[ar, pick] = False
    return ids.gather(1, torch.stack(picks, 1))


def run(name, reps, rounds):
    p_x, p_c, ctx, _ = _batch(B, L, N_ITEMS, 6)
    with torch.no_grad():
        if name == "carca":
            model = _model(N_ITEMS, N_ATTRS, 6, 90, 450, 3, 2, 0.01)
            prof, n_cols = (p_x, None, p_c), 90
            X = model.embeds.item_table()
            reco = lambda k: model.recommend(prof, ctx, k=k)  # noqa: E731
            div = lambda lam: model.recommend_diverse(prof, ctx, k=K, pool=P, lam=lam)  # noqa: E731
        else:
            model = KNN().cuda()
            gen = torch.Generator(device="cuda").manual_seed(0)
            attrs = (torch.rand(N_ITEMS, N_ATTRS, generator=gen, device="cuda") < 0.01).float()
            attrs[0] = 0
            model.register_attr_table(attrs)
            model.int8_table()
            prof, n_cols = (p_x, None, None), N_ATTRS
            X = model._similar_tables()["rows"]
            reco = lambda k: model.recommend(prof, None, k=k)  # noqa: E731
            div = lambda lam: model.recommend_diverse(prof, None, k=K, pool=P, lam=lam)  # noqa: E731
        s, ids = reco(P)
        rn = catalogue.row_rnorm(X, n_cols)
        rerank = lambda: catalogue.mmr_rerank("bench", s, ids, X, n_cols, K, LAM, "cosine", True, lambda: rn)  # noqa: E731
        fns = {"recommend_k10": lambda: reco(K), "recommend_k128": lambda: reco(P), "diverse": lambda: div(LAM),
               "rerank": rerank, "aten": lambda: _aten(s, ids, X, n_cols, K, LAM)}
        a, b = div(1.0), reco(K)
        lam1_bits = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
        same = float((rerank()[1] == fns["aten"]()).all(1).float().mean())
        runs = {v: [] for v in fns}
        for _ in range(rounds):
            for v, fn in fns.items():
                runs[v].append(round(_time(fn, reps), 4))
    ms = {v: min(r) for v, r in runs.items()}
    row = dict(model=name, B=B, P=P, k=K, lam=LAM, n_items=N_ITEMS, n_cols=n_cols, reps=reps, ms=ms, ms_runs=runs,
               feature_cost_ms=round(ms["diverse"] - ms["recommend_k128"], 4), lam1_is_recommend_bits=lam1_bits,
               aten_same_ids_share=round(same, 4),
               lazy_gflop=round(2.0 * (K - 1) * P * n_cols * B / 1e9, 3), gram_gflop=round(2.0 * P * P * n_cols * B / 1e9, 3))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--models", nargs="+", default=["carca", "knn"], choices=["carca", "knn"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [run(m, a.reps, a.rounds) for m in a.models]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
