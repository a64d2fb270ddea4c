"""CARCA.recommend(k=10) and CARCA.rank_items(N=1) restricted to a candidate set (candidates=S: carca_recommend_among /
carca_rank_items_among), timed with device events per batch of 128 users next to the unrestricted
calls on the same batch (tables cached, exclude="profile"), at
  C2  12,102 items, n_attrs 4096, d 90, g 450, H 3, 2 blocks: |S| = 128, 1,210, 6,051, 12,101; and the only alternative
      without candidate sets: forward over S as target groups of 1024, at |S| = 1,210;
  C4  dimensions d 128, g 640, H 4, 1,000,001 items (AllEmbedding over 64 attributes): |S| = 1,000 ... 1,000,000.
S is a seeded draw without replacement, normalised once (catalogue.CandidateSet) outside the timed region.  scratch_bytes
is what the calls allocate beyond their inputs and outputs, from the sizes csrc/recommend.hip and csrc/rank.hip compute.
Models and batches are bench_recommend.py's.
usage: python tools/bench_candidates.py [--reps N] [--config C2|C4] [--candidates N [N ...]] [--out file.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_recommend import _batch, _model, _time  # noqa: E402
from carca_replication_amd.catalogue import CandidateSet  # noqa: E402

CONFIGS = {
    "C2": dict(n_items=12102, n_attrs=4096, d=90, g=450, H=3, sizes=(128, 1210, 6051, 12101), forward_at=1210),
    "C4": dict(n_items=1000001, n_attrs=64, d=128, g=640, H=4, sizes=(1000, 10000, 100000, 1000000), forward_at=None),
}


def run(name, sizes, reps):
    cfg = CONFIGS[name]
    n_items, d, H = cfg["n_items"], cfg["d"], cfg["H"]
    n_ctx, B, L, k = 6, 128, 50, 10
    model = _model(n_items, cfg["n_attrs"], n_ctx, d, cfg["g"], H, 2, 0.01 if cfg["n_attrs"] > 64 else 0.1)
    p_x, p_c, ctx, _ = _batch(B, L, n_items, n_ctx)
    prof = (p_x, None, p_c)
    gen = torch.Generator(device="cuda").manual_seed(3)
    items = torch.randint(1, n_items, (B, 1), generator=gen, device="cuda")
    rows = []
    with torch.no_grad():
        def both(cand):
            rec = _time(lambda: model.recommend(prof, ctx, k=k, candidates=cand), reps)
            rnk = _time(lambda: model.rank_items(prof, ctx, items, candidates=cand), reps)
            rec2 = _time(lambda: model.recommend(prof, ctx, k=k, candidates=cand), reps)  # (alternated)
            return round(min(rec, rec2), 4), round(rnk, 4)

        rec, rnk = both(None)
        rank_scratch = (B * 4 + 255) // 256 * 256 + B * (1 + L) * 8
        rows.append(dict(config=name, n_items=n_items, d=d, H=H, B=B, candidates=None, ms_recommend_k10=rec,
                         ms_rank_items_N1=rnk, scratch_bytes_recommend=B * n_items * 4, scratch_bytes_rank=rank_scratch))
        print(json.dumps(rows[-1]), flush=True)
        for c in sizes:
            S = CandidateSet(torch.randperm(n_items - 1, generator=gen, device="cuda")[:c] + 1, n_items)
            rec, rnk = both(S)
            row = dict(config=name, n_items=n_items, d=d, H=H, B=B, candidates=len(S), ms_recommend_k10=rec,
                       ms_rank_items_N1=rnk, scratch_bytes_recommend=B * max(len(S), 1) * 4,
                       scratch_bytes_rank=rank_scratch)
            if c == cfg["forward_at"]:
                def fwd():
                    for chunk in S.ids.split(1024):
                        ids = chunk.to(torch.int64).expand(B, -1)
                        model(prof, [(ids, None, ctx.unsqueeze(1).expand(B, ids.shape[1], n_ctx))])
                row["ms_forward_over_S"] = round(_time(fwd, max(1, reps // 10)), 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--config", choices=sorted(CONFIGS), default="C2")
    ap.add_argument("--candidates", type=int, nargs="+", default=None, help="set sizes (default: the config's four)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = run(a.config, tuple(a.candidates) if a.candidates else CONFIGS[a.config]["sizes"], a.reps)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
