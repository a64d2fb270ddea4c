"""Bytes the hit compare of dedup_resolve_kernel REQUESTS per launch in the steady state of bench.py's evaluation step (one
batch repeated: every item's cache entry filled), counted on the host from the batch's ids (seed 1234) the way
profiles/r15_resolve_fetch.json counts: one attribute row = n_attrs x 4 bytes.

  per_row   every kept row reads its own bytes and its item's entry (the build before round 20, or tuning key 22 = 1);
  grouped   the insert launch ranks an item's rows; the row of every GROUP-th rank among the first LIST reads the entry
            once for itself and the next GROUP - 1 ranks, rows past the list read it for themselves.

usage: python tools/resolve_requests.py [--batch 128] [--list 16] [--group 4]      (no GPU needed; one JSON line)"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=bench.C2["B"])
    ap.add_argument("--list", type=int, default=16)
    ap.add_argument("--group", type=int, default=4)
    args = ap.parse_args()
    from carca_replication_amd.synth import eval_batch

    c = dict(bench.C2, B=args.batch)
    profile, target, _ = eval_batch(c["B"], c["L"], c["N"], c["n_items"], c["n_attrs"], c["n_ctx"], seed=1234)
    ids = np.concatenate([profile[0].numpy().ravel(), target[0].numpy().ravel()])
    m = np.bincount(ids[ids != 0])
    m = m[m > 0]
    row = c["n_attrs"] * 4
    kept = int(m.sum())
    listed = np.minimum(m, args.list)
    leaders = int(((listed + args.group - 1) // args.group).sum())
    past = int((m - listed).sum())
    out = dict(config="B=%d" % c["B"], kept_rows=kept, distinct_ids=int(len(m)), max_rows_per_id=int(m.max()),
               LIST=args.list, GROUP=args.group, leaders=leaders, rows_past_list=past, row_bytes=row,
               requested_bytes_per_row=2 * kept * row, requested_bytes_grouped=(kept + leaders + past) * row,
               requested_bytes_floor=(kept + int(len(m))) * row)
    out["grouped_over_per_row"] = round(out["requested_bytes_grouped"] / out["requested_bytes_per_row"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
