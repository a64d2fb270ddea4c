"""A candidate list per user (CARCA.score_items / recommend_from, csrc/recommend_lists.hip) timed with device events at C2
(12,102 items, n_attrs 4096, d 90, g 450, H 3, 2 blocks), B = 128 users, profile lengths U{3..50} left-padded as
tools/bench_recommend.py draws them, lists of N in {101, 1000, 5000} ids drawn with replacement, k = 10, tables cached.
Per N, ms per batch of: score_items, recommend_from, and on the same batch recommend(k=10) over the whole catalogue and
the chunked forward + torch.topk over the same lists (groups of up to 1024 candidates).  The series are interleaved
(one call of each per pass), so a drift of the machine meets all four alike; the spread is (max - min) / median of a
series' per-pass times.
usage: python tools/bench_lists.py [--passes N] [--inner N] [--out profiles/r25_lists.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from carca_replication_amd import modules as M  # noqa: E402

N_ITEMS, N_ATTRS, N_CTX, D, G, H, B, L, K = 12102, 4096, 6, 90, 450, 3, 128, 50, 10


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
    return p_x.cuda(), p_c.cuda(), torch.rand(B, N_CTX, generator=gen).cuda(), gen


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


def run(model, prof, ctx, gen, N, passes, inner):
    items = torch.randint(1, N_ITEMS, (B, N), generator=gen).cuda()

    def chunked():
        ys = []
        for lo in range(0, N, 1024):
            ids = items[:, lo:lo + 1024].contiguous()
            oc = ctx.unsqueeze(1).expand(B, ids.shape[1], N_CTX)
            ys.append(model(prof, [(ids, None, oc)]).reshape(B, -1))
        return torch.topk(torch.cat(ys, 1), K, dim=1)

    fns = {
        "score_items": lambda: model.score_items(prof, ctx, items),
        "recommend_from": lambda: model.recommend_from(prof, ctx, items, k=K),
        "recommend": lambda: model.recommend(prof, ctx, k=K),
        "chunked_forward_topk": chunked,
    }
    with torch.no_grad():
        series = _interleaved(fns, passes, inner)
    row = dict(config="C2", B=B, N=N, k=K, passes=passes, inner=inner)
    for name, ts in series.items():
        row[name] = _summary(ts)
    row["recommend_over_recommend_from"] = round(row["recommend"]["ms"] / row["recommend_from"]["ms"], 2)
    row["chunked_over_recommend_from"] = round(row["chunked_forward_topk"]["ms"] / row["recommend_from"]["ms"], 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "r25_lists.json"))
    a = ap.parse_args()
    model = _model()
    p_x, p_c, ctx, gen = _batch()
    rows = []
    for N in (101, 1000, 5000):
        rows.append(run(model, (p_x, None, p_c), ctx, gen, N, a.passes, a.inner))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
