"""Item-to-item top-k (CARCA.similar_items / KNN.similar_items / ops.similar_rows, csrc/similar_items.hip) timed with
device events, k = 10, exclude_self, over random fp32 tables of the shapes
  C2-carca  12,102 x 90      (the query-stationary kernel, 96 wide)
  C2-knn    12,102 x 4,096   (the streaming kernel)
  C4-carca  1,000,001 x 128  (query-stationary, 128 wide)
  C4-knn    1,000,001 x 64   (query-stationary, 64 wide)
with Q = 128, 1,024 and (C2 only, unless --all-c4) every item as queries.  Variants, each measured in a fresh process
after a warm-up call, the variants of a shape alternating over --rounds rounds (the minimum and every run are kept):
  cosine    similar_items, metric "cosine", the reciprocal norms cached as the models cache them
  dot       similar_items, metric "dot"
  aten      normalize(X[q]) @ normalize(X).T, id 0 and the query masked, topk -- timing only: it has no tie rule
  knn_reco  KNN.recommend(exclude=None) on a profile ending in the query, the dot metric's yardstick (Q <= 65,535)
The split by kernel comes from a separate rocprofv3 --kernel-trace --stats run of one child
(python tools/bench_similar_items.py --child C4-carca 1024 cosine).
--scratch-gib G sets max_scratch_bytes (default 1 GiB, the calls' default): 1,024 queries x 1 M items are 4 GiB of scores, so
the default runs them as four chunks of 256.
usage: python tools/bench_similar_items.py [--shapes NAME ...] [--rounds N] [--all-c4] [--scratch-gib G] [--out file.json]"""
import argparse
import json
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_recommend import _time  # noqa: E402
from carca_replication_amd import catalogue  # noqa: E402
from carca_replication_amd.modules import KNN  # noqa: E402

SHAPES = {"C2-carca": (12102, 90), "C2-knn": (12102, 4096), "C4-carca": (1000001, 128), "C4-knn": (1000001, 64)}
VARIANTS = ("cosine", "dot", "aten", "knn_reco")
K = 10


def _aten(X, q, k):
    Xn = torch.nn.functional.normalize(X, dim=1)
    s = Xn[q] @ Xn.T
    s[:, 0] = float("-inf")
    s.scatter_(1, q[:, None], float("-inf"))
    return torch.topk(s, k, dim=1)


def child(shape, Q, variant, scratch_gib=1):
    n_items, F = SHAPES[shape]
    g = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn(n_items, (F + 3) // 4 * 4, generator=g, device="cuda")
    X[0] = 0
    q = torch.arange(n_items, device="cuda") if Q == 0 else torch.randint(1, n_items, (Q,), generator=g, device="cuda")
    nq = q.shape[0]
    work = nq * n_items * F  # multiply-adds of the scoring product
    reps = 20 if work < 2e11 else 5 if work < 2e12 else 2
    with torch.no_grad():
        if variant in ("cosine", "dot"):
            rn = catalogue.row_rnorm(X, F)
            fn = lambda: catalogue.similar_items("bench", X, F, lambda: rn, q, K, variant, True, None, scratch_gib << 30)  # noqa: E731
        elif variant == "aten":
            fn = lambda: _aten(X[:, :F], q, K)  # noqa: E731
        else:
            model = KNN().cuda()
            model.register_attr_table(X[:, :F])
            model.int8_table()
            prof = (q[:, None], None, None)
            fn = lambda: model.recommend(prof, None, k=K, exclude=None)  # noqa: E731
        ms = _time(fn, reps)
    chunks = len(catalogue.similar_chunks(nq, catalogue.similar_chunk_rows(scratch_gib << 30, n_items)))
    print(json.dumps(dict(shape=shape, n_items=n_items, F=F, Q=nq, variant=variant, ms=round(ms, 4), reps=reps,
                          scratch_gib=scratch_gib, chunks=chunks if variant in ("cosine", "dot") else None,
                          gflop=round(2.0 * work / 1e9, 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=3, metavar=("SHAPE", "Q", "VARIANT"))
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--all-c4", action="store_true", help="also every item as queries at the 1 M-item shapes (minutes per call)")
    ap.add_argument("--scratch-gib", type=int, default=1)
    ap.add_argument("--queries", type=int, nargs="+", default=[128, 1024, 0], help="query counts; 0 = every item")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], int(a.child[1]), a.child[2], a.scratch_gib)
        return
    rows = {}
    for shape in a.shapes:
        n_items = SHAPES[shape][0]
        for Q in a.queries:
            if Q == 0 and n_items > 100000 and not a.all_c4:
                continue
            variants = [v for v in VARIANTS if not (v == "knn_reco" and (Q or n_items) > 65535)]
            for _ in range(a.rounds):
                for v in variants:  # alternating: one fresh process per run
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, str(Q), v,
                                        "--scratch-gib", str(a.scratch_gib)],
                                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
                    if r.returncode != 0:  # (a device fault or an out-of-memory: stop, start nothing more)
                        sys.stderr.write(r.stderr[-2000:])
                        raise SystemExit(f"{shape} Q={Q} {v}: exit {r.returncode}")
                    row = json.loads(r.stdout.strip().splitlines()[-1])
                    e = rows.setdefault((shape, row["Q"], v), dict(row, ms_runs=[]))
                    e["ms_runs"].append(row["ms"])
                    e["ms"] = min(e["ms_runs"])
                    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(list(rows.values()), f, indent=1)


if __name__ == "__main__":
    main()
