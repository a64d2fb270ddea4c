#!/usr/bin/env python
"""An evaluation epoch's worth of DISTINCT batches with and without the per-item cache of the feature product
(AllEmbedding.feat_cache): 64 dense C2 batches drawn from one 12,102-item catalogue, inputs resident in HBM.

  python tools/bench_eval_cache.py [--cache on|off] [--batches 64] [--reps 3]

Per repetition, after bench.py's pre-heat (PREHEAT_S of the same forwards, untimed) and with every cache entry emptied:
  cold_ms       batch 1 alone, fenced -- with the cache: all misses plus publishing;
  users_per_s   batches 4 .. 64 between two fences (after three batches nearly every item has been seen).
--cache off sets tuning key 21 = 1: the launches of a build without the cache.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache", choices=("on", "off"), default="on")
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()

    import torch

    import bench
    from carca_replication_amd import ops

    c = bench.C2
    dev = torch.device("cuda")
    B, L, N = c["B"], c["L"], c["N"]
    model = bench.build_model(c, dev)
    gen = torch.Generator(device=dev).manual_seed(1234)
    table = torch.rand(c["n_items"], c["n_attrs"], generator=gen, device=dev)
    table[0] = 0.0
    batches = []
    for _ in range(args.batches):
        px = torch.randint(1, c["n_items"], (B, L), generator=gen, device=dev)
        lens = torch.randint(3, L + 1, (B,), generator=gen, device=dev)
        px = px * (torch.arange(L, device=dev)[None, :] >= (L - lens)[:, None])
        ox = torch.randint(1, c["n_items"], (B, N), generator=gen, device=dev)
        pc = torch.rand(B, L, c["n_ctx"], generator=gen, device=dev) * (px != 0)[..., None]
        oc = torch.rand(B, 1, c["n_ctx"], generator=gen, device=dev).expand(B, N, c["n_ctx"]).contiguous()
        batches.append(((px.int(), table[px].contiguous(), pc), (ox.int(), table[ox].contiguous(), oc)))
    ops.set_tuning(ops.TUNE_FEAT_CACHE, 0 if args.cache == "on" else 1)

    def run(b):
        model(profile=b[0], targets=[b[1]])

    reps = []
    with torch.no_grad():
        for _ in range(args.reps):
            t_heat = time.perf_counter()
            while time.perf_counter() - t_heat < bench.PREHEAT_S:
                for b in batches[:8]:
                    run(b)
                torch.cuda.synchronize()
            fc = model.embeds.__dict__.get("_feat_cache")
            if fc is not None:
                fc["state"].zero_()  # (every entry empty again: the epoch starts cold)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(batches[0])
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            first = ops.feat_dedup_rows_computed()
            for b in batches[1:3]:
                run(b)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            for b in batches[3:]:
                run(b)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            reps.append(dict(cold_ms=round(1e3 * (t1 - t0), 4), rows_computed_batch_1=first,
                             rows_computed_last_batch=ops.feat_dedup_rows_computed(),
                             ms_per_batch_4_on=round(1e3 * (t3 - t2) / (len(batches) - 3), 4),
                             users_per_s=round(B * (len(batches) - 3) / (t3 - t2), 1)))
    ops.set_tuning(ops.TUNE_FEAT_CACHE, 0)
    print(json.dumps(dict(what="distinct dense C2 batches, one catalogue", cache=args.cache, batches=len(batches),
                          allocated=model.embeds.__dict__.get("_feat_cache") is not None, reps=reps)), flush=True)


if __name__ == "__main__":
    main()
