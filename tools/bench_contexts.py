"""Several request contexts per user (CARCA.score_items_at / best_context / recommend_at, csrc/recommend_contexts.hip)
timed with device events at C2 (12,102 items, n_attrs 4096, d 90, g 450, H 3, 2 blocks), B = 128 users, profile lengths
U{3..50} left-padded as tools/bench_recommend.py draws them, k = 10, tables cached, C in {1, 2, 8, 24} contexts per user.
Per C, ms per batch of: score_items_at and best_context over lists of N in {101, 1000} ids against the loop of C
score_items calls, and recommend_at over the catalogue against the loop of C recommend calls; at C = 1 the loop is the
single-context call each equals.  model_side is the single-context call's host path without its scoring launch
(catalogue.carca_model_side alone), so score_items - model_side is the single-context kernel's own time, printed beside
the per-context increment (t(C = 8) - t(C = 1)) / 7 of each new call.  The series of one C are interleaved (one call of
each per pass), so a drift of the machine meets all alike; the spread is (max - min) / median of a series' per-pass times.
usage: python tools/bench_contexts.py [--passes N] [--inner N] [--out profiles/r31_contexts.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from carca_replication_amd import catalogue  # noqa: E402
from carca_replication_amd import modules as M  # noqa: E402

N_ITEMS, N_ATTRS, N_CTX, D, G, H, B, L, K = 12102, 4096, 6, 90, 450, 3, 128, 50, 10
CONTEXT_COUNTS = (1, 2, 8, 24)
LIST_SIZES = (101, 1000)


def _model(seed=0):
    torch.manual_seed(seed)
    enc = M.IdentityEncoding()
    model = M.CARCA(D, 0.0, M.AllEmbedding(N_ITEMS, D, G, N_CTX, N_ATTRS, enc),
                    torch.nn.ModuleList([M.SelfAttentionBlock(D, H, 0.0, True) for _ in range(2)]),
                    M.CrossAttentionBlock(D, H, 0.0, True)).cuda().eval()
    gen = torch.Generator(device="cuda").manual_seed(seed)
    attrs = (torch.rand(N_ITEMS, N_ATTRS, generator=gen, device="cuda") < 0.01).float()
    attrs[0] = 0
    model.embeds.register_attr_table(attrs)
    return model


def _batch(seed=1):
    gen = torch.Generator().manual_seed(seed)
    lens = torch.randint(3, L + 1, (B,), generator=gen)
    p_x = torch.randint(1, N_ITEMS, (B, L), generator=gen) * (torch.arange(L) >= (L - lens).unsqueeze(1))
    p_c = torch.rand(B, L, N_CTX, generator=gen) * (p_x != 0).unsqueeze(-1)
    return p_x.cuda(), p_c.cuda(), gen


def _once(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def _interleaved(fns, passes, inner):
    """name -> per-pass ms, one measurement of every series per pass, in turn."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(passes):
        for name, fn in fns.items():
            out[name].append(_once(fn, inner))
    return out


def _summary(ts):
    med = statistics.median(ts)
    return dict(ms=round(med, 4), min=round(min(ts), 4), max=round(max(ts), 4), spread=round((max(ts) - min(ts)) / med, 3))


def run(model, prof, gen, n_c, passes, inner):
    X = torch.rand(B, n_c, N_CTX, generator=gen).cuda()
    xs = [X[:, c].contiguous() for c in range(n_c)]
    lists = {N: torch.randint(1, N_ITEMS, (B, N), generator=gen).cuda() for N in LIST_SIZES}

    def model_side():
        return catalogue.carca_model_side(model, prof, xs[0], "bench")

    fns = {"model_side": model_side}
    for N, items in lists.items():
        fns[f"score_items_at_N{N}"] = lambda items=items: model.score_items_at(prof, X, items)
        fns[f"best_context_N{N}"] = lambda items=items: model.best_context(prof, X, items)
        fns[f"score_items_loop_N{N}"] = lambda items=items: [model.score_items(prof, x, items) for x in xs]
    fns["recommend_at"] = lambda: model.recommend_at(prof, X, k=K)
    fns["recommend_loop"] = lambda: [model.recommend(prof, x, k=K) for x in xs]
    with torch.no_grad():
        series = _interleaved(fns, passes, inner)
    row = dict(config="C2", B=B, C=n_c, k=K, passes=passes, inner=inner)
    for name, ts in series.items():
        row[name] = _summary(ts)
    for N in LIST_SIZES:
        loop = row[f"score_items_loop_N{N}"]["ms"]
        row[f"loop_over_score_items_at_N{N}"] = round(loop / row[f"score_items_at_N{N}"]["ms"], 2)
        row[f"loop_over_best_context_N{N}"] = round(loop / row[f"best_context_N{N}"]["ms"], 2)
    row["loop_over_recommend_at"] = round(row["recommend_loop"]["ms"] / row["recommend_at"]["ms"], 2)
    return row


def increments(rows):
    """(t(C = 8) - t(C = 1)) / 7 of each new call, beside the single-context call's own scoring time at C = 1."""
    by_c = {r["C"]: r for r in rows}
    if 1 not in by_c or 8 not in by_c:
        return {}
    one, eight = by_c[1], by_c[8]
    out = dict(summary="per-context increment, ms", model_side_ms=one["model_side"]["ms"])
    names = [f"{call}_N{N}" for N in LIST_SIZES for call in ("score_items_at", "best_context")] + ["recommend_at"]
    for name in names:
        out[name] = round((eight[name]["ms"] - one[name]["ms"]) / 7, 4)
    for N in LIST_SIZES:
        out[f"score_items_kernel_N{N}"] = round(one[f"score_items_loop_N{N}"]["ms"] - one["model_side"]["ms"], 4)
    out["recommend_kernels"] = round(one["recommend_loop"]["ms"] - one["model_side"]["ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join("profiles", "r31_contexts.json"))
    a = ap.parse_args()
    model = _model()
    p_x, p_c, gen = _batch()
    rows = []
    for n_c in CONTEXT_COUNTS:
        rows.append(run(model, (p_x, None, p_c), gen, n_c, a.passes, a.inner))
        print(json.dumps(rows[-1]), flush=True)
    rows.append(increments(rows))
    print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
