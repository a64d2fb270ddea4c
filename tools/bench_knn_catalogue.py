"""Full-catalogue top-k and exact ranks of the KNN baseline (KNN.recommend / KNN.rank_items, csrc/knn_catalogue.hip)
timed with device events, B = 128 users, profile length 50, exclude="profile", at
  C2       12,102 items x 4,096 attributes: a multi-hot 0/1 table (density 1 %, the i8 MFMA path) and the same shape
           as random fp32 (the fp32 MFMA path);
  C4       1,000,001 items x 64 attributes: multi-hot (i8) and random fp32;
each with recommend(k = 10) and rank_items(N = 1), beside the ATen composition (q @ A.T, masked_fill of id 0 and the
profile, topk) -- for timing only: its tie order is not the kernels'.  The split by kernel comes from a separate
rocprofv3 --kernel-trace --stats run of this script (profiles/r09_knn_catalogue.json).
usage: python tools/bench_knn_catalogue.py [--reps N] [--config all|C2|C4] [--out file.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_recommend import _time  # noqa: E402
from carca_replication_amd.modules import KNN  # noqa: E402


def _aten(A, p_x, k):
    q = A[p_x[:, -1]]
    s = q @ A.T
    mask = torch.zeros_like(s, dtype=torch.bool)
    mask.scatter_(1, p_x, True)
    mask[:, 0] = True
    return torch.topk(s.masked_fill_(mask, float("-inf")), k, dim=1)


def run(name, n_items, F, table, reps):
    B, L, k = 128, 50, 10
    g = torch.Generator(device="cuda").manual_seed(1)
    if table == "multihot":
        A = (torch.rand(n_items, F, generator=g, device="cuda") < 0.01).float()
    else:
        A = torch.rand(n_items, F, generator=g, device="cuda") * 2 - 1
    A[0] = 0
    model = KNN().cuda()
    model.register_attr_table(A)
    i8 = model.int8_table() is not None  # (the routing decision: built here, once)
    p_x = torch.randint(1, n_items, (B, L), generator=g, device="cuda")
    items = torch.randint(1, n_items, (B, 1), generator=g, device="cuda")
    prof = (p_x, None, None)
    out = dict(config=name, table=table, path="i8" if i8 else "fp32", n_items=n_items, F=F, B=B)
    with torch.no_grad():
        rec = _time(lambda: model.recommend(prof, None, k=k), reps)
        rank = _time(lambda: model.rank_items(prof, None, items), reps)
        aten = _time(lambda: _aten(A, p_x, k), reps)
        rec2 = _time(lambda: model.recommend(prof, None, k=k), reps)
    out["ms_recommend_k10"] = round(min(rec, rec2), 4)
    out["ms_recommend_k10_runs"] = [round(rec, 4), round(rec2, 4)]
    out["ms_rank_items_N1"] = round(rank, 4)
    out["ms_aten_topk10"] = round(aten, 4)
    out["users_per_s_recommend"] = round(B / (min(rec, rec2) * 1e-3))
    out["gemm_gflop"] = round(2.0 * B * n_items * F / 1e9, 2)
    out["table_mb"] = round(n_items * F * (1 if i8 else 4) / 1e6, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--config", choices=("all", "C2", "C4"), default="all")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    if a.config in ("all", "C2"):
        for table in ("multihot", "fp32"):
            rows.append(run("C2", 12102, 4096, table, a.reps))
            print(json.dumps(rows[-1]), flush=True)
    if a.config in ("all", "C4"):
        for table in ("multihot", "fp32"):
            rows.append(run("C4", 1000001, 64, table, max(3, a.reps // 5)))
            print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
