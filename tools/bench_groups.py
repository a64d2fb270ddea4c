"""CARCA.recommend_by_group(k=10) and recommend_capped(k=10, max_per_group=2) over an ItemGroups of G groups (DESIGN.md
section 23), timed with device events per batch of 128 users, in the same process and session as
  recommend(k=10)   over the whole catalogue: the same sweep, so the floor of both calls;
  the loop          G calls recommend(k=10, candidates=CandidateSet_g) with sets built beforehand: what a page of G
                    carousels costs without item groups (the profile side and three launches per call),
at
  C2  12,102 items, n_attrs 4096, d 90, g 450, H 3, 2 blocks,
  C4  dimensions d 128, g 640, H 4, 1,000,001 items (AllEmbedding over 64 attributes),
with G = 8, 64 and 1024 groups of random membership (every item labelled, seeded).  Tables cached, exclude="profile".
The three single calls are timed in interleaved passes and the smallest pass is kept; the loop is timed once per G with
fewer repetitions (its cost is G times a call's).  Every row also says whether by-group equals the loop bit for bit.
Models and batches are bench_recommend.py's.
usage: python tools/bench_groups.py [--reps N] [--passes N] [--config C2 C4] [--groups G [G ...]] [--out file.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_recommend import _batch, _model, _time  # noqa: E402
from carca_replication_amd.catalogue import CandidateSet, ItemGroups  # noqa: E402

CONFIGS = {
    "C2": dict(n_items=12102, n_attrs=4096, d=90, g=450, H=3),
    "C4": dict(n_items=1000001, n_attrs=64, d=128, g=640, H=4),
}
GROUPS = (8, 64, 1024)


def run(name, groups, reps, passes):
    cfg = CONFIGS[name]
    n_items, d, H = cfg["n_items"], cfg["d"], cfg["H"]
    n_ctx, B, L, k, m = 6, 128, 50, 10, 2
    model = _model(n_items, cfg["n_attrs"], n_ctx, d, cfg["g"], H, 2, 0.01 if cfg["n_attrs"] > 64 else 0.1)
    p_x, p_c, ctx, _ = _batch(B, L, n_items, n_ctx)
    prof = (p_x, None, p_c)
    gen = torch.Generator(device="cuda").manual_seed(5)
    rows = []
    with torch.no_grad():
        for G in groups:
            labels = torch.randint(0, G, (n_items,), generator=gen, device="cuda")
            gr = ItemGroups(labels, n_groups=G)
            sets = [CandidateSet(gr.members(g), n_items) for g in range(G)]
            calls = dict(
                recommend=lambda: model.recommend(prof, ctx, k=k),
                by_group=lambda: model.recommend_by_group(prof, ctx, gr, k=k),
                capped=lambda: model.recommend_capped(prof, ctx, gr, k=k, max_per_group=m))
            best = {key: float("inf") for key in calls}
            for _ in range(passes):  # interleaved: a drift of the machine hits the three alike
                for key, fn in calls.items():
                    best[key] = min(best[key], _time(fn, reps))

            def loop():
                return [model.recommend(prof, ctx, k=k, candidates=s) for s in sets]

            loop_reps = max(2, reps * 8 // G)
            ms_loop = _time(loop, loop_reps)
            got, want = calls["by_group"](), loop()
            same = all(torch.equal(got[0][:, g], want[g][0]) and torch.equal(got[1][:, g], want[g][1]) for g in range(G))
            sizes = [int(s.ids.shape[0]) for s in sets]
            row = dict(config=name, n_items=n_items, d=d, H=H, B=B, k=k, groups=G, group_size_min=min(sizes),
                       group_size_max=max(sizes), reps=reps, passes=passes, loop_reps=loop_reps,
                       ms_recommend=round(best["recommend"], 4), ms_by_group=round(best["by_group"], 4),
                       ms_capped_m2=round(best["capped"], 4), ms_loop_of_G_calls=round(ms_loop, 3),
                       by_group_over_recommend=round(best["by_group"] / best["recommend"], 3),
                       capped_over_recommend=round(best["capped"] / best["recommend"], 3),
                       loop_over_by_group=round(ms_loop / best["by_group"], 2), by_group_equals_loop=bool(same),
                       scratch_bytes_logits=B * (n_items - 1) * 4, scratch_bytes_capped_keys=B * G * m * 8)
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--config", choices=sorted(CONFIGS), nargs="+", default=["C2", "C4"])
    ap.add_argument("--groups", type=int, nargs="+", default=list(GROUPS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for name in a.config:
        rows += run(name, tuple(a.groups), a.reps, a.passes)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
