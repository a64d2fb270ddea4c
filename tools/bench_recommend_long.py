"""CARCA.recommend(k=10) and CARCA.rank_items(N=1) past the fused envelope (allow_composed=True), timed
with device events per batch of 128 users at C2 dimensions (12,102 items, n_attrs 4096, d 90, g 450, H 3, 2 blocks; tables
cached, exclude="profile"):
  L = 64    profile lengths U{3..50}, left-padded: the fused encoder and the whole-user scorer (rc::CaScorer);
  L = 65    the same users with one more pad slot: the composed encoder and the chunked scorer (rc::CaLongScorer) over
            the same valid slots -- the price of leaving the fused envelope;
  L = 200, 1024   full profiles.
Each row also times the profile side alone (catalogue.carca_model_side: embedding, encoder, K / u products), so that
ms - ms_profile_side is what the catalogue launches (the sweep and what follows it) take; the L = 65 to L = 64 ratios of
both are in the last row.  Models and batches are bench_recommend.py's.
usage: python tools/bench_recommend_long.py [--reps N] [--lengths L [L ...]] [--out file.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_recommend import _batch, _model, _time  # noqa: E402
from carca_replication_amd import _lib, catalogue  # noqa: E402


def _profile(L, B, n_items, n_ctx):
    """(p_x, p_c, ctx): bench_recommend's U{3..50} batch at 50 slots, left-padded to L <= 65; full profiles beyond."""
    if L <= 65:
        p_x, p_c, ctx, _ = _batch(B, 50, n_items, n_ctx)
        pad = L - 50
        p_x = torch.cat([p_x.new_zeros(B, pad), p_x], 1)
        p_c = torch.cat([p_c.new_zeros(B, pad, n_ctx), p_c], 1)
        return p_x, p_c, ctx
    gen = torch.Generator().manual_seed(L)
    p_x = torch.randint(1, n_items, (B, L), generator=gen)
    return p_x.cuda(), torch.rand(B, L, n_ctx, generator=gen).cuda(), torch.rand(B, n_ctx, generator=gen).cuda()


def run(lengths, reps):
    n_items, n_attrs, d, g, H, n_ctx, B, k = 12102, 4096, 90, 450, 3, 6, 128, 10
    model = _model(n_items, n_attrs, n_ctx, d, g, H, 2, 0.01)
    items = torch.randint(1, n_items, (B, 1), generator=torch.Generator().manual_seed(3)).cuda()
    rows = []
    with torch.no_grad():
        for L in lengths:
            p_x, p_c, ctx = _profile(L, B, n_items, n_ctx)
            prof = (p_x, None, p_c)
            n = max(2, reps if L <= 200 else reps // 5)
            rec = _time(lambda: model.recommend(prof, ctx, k=k, allow_composed=True), n)
            rnk = _time(lambda: model.rank_items(prof, ctx, items, allow_composed=True), n)
            rec2 = _time(lambda: model.recommend(prof, ctx, k=k, allow_composed=True), n)  # (alternated)
            side = _time(lambda: catalogue.carca_model_side(model, prof, ctx, "bench", allow_composed=True), n)
            rec = min(rec, rec2)
            route = catalogue.carca_route("bench", d, [H, H], L, H, True)
            rows.append(dict(config="C2", L=L, B=B, n_items=n_items, d=d, H=H, k=k, valid_slots=int((p_x != 0).sum()),
                             profile_side=route, scorer="CaScorer" if L <= _lib.MAX_L else "CaLongScorer",
                             ms_recommend_k10=round(rec, 4), ms_rank_items_N1=round(rnk, 4),
                             ms_profile_side=round(side, 4), ms_recommend_launches=round(rec - side, 4),
                             ms_rank_launches=round(rnk - side, 4)))
            print(json.dumps(rows[-1]), flush=True)
    by = {r["L"]: r for r in rows}
    if 64 in by and 65 in by:
        ratio = {key: round(by[65][key] / by[64][key], 3) for key in
                 ("ms_recommend_k10", "ms_rank_items_N1", "ms_profile_side", "ms_recommend_launches", "ms_rank_launches")}
        rows.append(dict(config="C2", ratio_L65_to_L64=ratio))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--lengths", type=int, nargs="+", default=[64, 65, 200, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_recommend_long.json"))
    a = ap.parse_args()
    rows = run(a.lengths, a.reps)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
