"""Exact full-catalogue ranks (CARCA.rank_items, csrc/rank.hip) timed with device events next to CARCA.recommend on the
same batch (tables cached, exclude="profile"), at
  C2  B = 128, 12,102 items, n_attrs 4096, d 90, g 450, H 3, 2 blocks: rank_items with N = 1 and N = 101, recommend(k=10);
      then the full-ranking evaluation of 1,024 users (DeviceLoader, batches of 128): evaluate_full_ranks with five
      cutoffs (1, 5, 10, 20, 50) against five evaluate_full calls, wall clock;
  C4  dimensions d 128, g 640, H 4, 1,000,001 items (AllEmbedding over 64 attributes), B = 128: rank_items N = 1, recommend.
Models and batches are bench_recommend.py's.  usage: python tools/bench_rank.py [--reps N] [--no-c4] [--out file.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_recommend import _batch, _model, _time  # noqa: E402
from carca_replication_amd import train as T  # noqa: E402
from carca_replication_amd.device_data import DeviceInteractions, DeviceLoader  # noqa: E402

KS = (1, 5, 10, 20, 50)


def run(name, n_items, n_attrs, d, g, H, reps, evaluation):
    n_ctx, B, L, k = 6, 128, 50, 10
    model = _model(n_items, n_attrs, n_ctx, d, g, H, 2, 0.01 if n_attrs > 64 else 0.1)
    p_x, p_c, ctx, _ = _batch(B, L, n_items, n_ctx)
    prof = (p_x, None, p_c)
    gen = torch.Generator(device="cuda").manual_seed(3)
    out = dict(config=name, n_items=n_items, d=d, H=H, B=B)
    with torch.no_grad():
        rec = _time(lambda: model.recommend(prof, ctx, k=k), reps)
        for N in ((1, 101) if evaluation else (1,)):
            items = torch.randint(1, n_items, (B, N), generator=gen, device="cuda")
            out[f"ms_rank_items_N{N}"] = round(_time(lambda: model.rank_items(prof, ctx, items), reps), 4)
        rec2 = _time(lambda: model.recommend(prof, ctx, k=k), reps)  # (alternated: recommend before and after)
    out["ms_recommend_k10"] = round(min(rec, rec2), 4)
    out["ms_recommend_k10_runs"] = [round(rec, 4), round(rec2, 4)]
    if evaluation:
        rng = np.random.default_rng(5)
        profiles, ctxd = {}, {}
        for u in range(1024):
            profiles[u] = [int(v) for v in rng.integers(1, n_items, size=int(rng.integers(4, 52)))]
            for it in profiles[u]:
                ctxd[(u, it)] = rng.random(n_ctx).astype(np.float32)
        loader = DeviceLoader(DeviceInteractions(profiles, ctxd, n_items), "test", batch_size=128, profile_seq_len=L,
                              target_seq_len=101)

        def wall(fn, r):
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(r):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / r

        r = max(2, reps // 10)
        five = wall(lambda: [T.evaluate_full(model, loader, "cuda", kk) for kk in KS], r)
        one = wall(lambda: T.evaluate_full_ranks(model, loader, "cuda", ks=KS), r)
        five2 = wall(lambda: [T.evaluate_full(model, loader, "cuda", kk) for kk in KS], r)
        out.update(eval_users=1024, ms_evaluate_full_x5=round(min(five, five2), 3),
                   ms_evaluate_full_ranks=round(one, 3), eval_speedup=round(min(five, five2) / one, 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--no-c4", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [run("C2", 12102, 4096, 90, 450, 3, a.reps, True)]
    print(json.dumps(rows[-1]), flush=True)
    if not a.no_c4:
        rows.append(run("C4-dims", 1000001, 64, 128, 640, 4, max(2, a.reps // 10), False))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
