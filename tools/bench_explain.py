"""Which profile slots drive a score (CARCA.explain_items / explain_top_slots / recommend_explained,
csrc/explain_lists.hip) timed with device events at C2 (12,102 items, n_attrs 4096, d 90, g 450,
H 3, 2 blocks), B = 128 users, profile lengths U{3..50} left-padded as tools/bench_lists.py draws them, tables cached.
One process measures one of two sets of interleaved series (one call of each per pass, so a drift of the machine meets
all alike; the spread is (max - min) / median of a series' per-pass times) and appends one record to --out:
  --set explain   per N in {10, 101, 1000}: explain_items, explain_top_slots(m=3), score_items, and an ATen composition of
                  explain_top_slots' outputs from the same staged tensors (the model side of the call itself, then einsum
                  of the gathered item-query rows with K, softmax over the valid slots, einsum with U, topk);
  --set serve     recommend_explained(k=10, m=3) where the package has it, recommend(k=10), score_items at N = 10: what a
                  user pays for a list with its reasons, and for the scores alone.
--package-root imports the package from another checkout (the parent commit's tree with its own built library), and
--label names the build in the record: run the two builds in alternation, a fresh process per run.
Gates: explain_top_slots <= the ATen composition at N = 101 and 1000; recommend_explained <
the parent's recommend + the parent's score_items at N = 10.
usage: python tools/bench_explain.py --set explain|serve [--label this] [--package-root DIR] [--passes N] [--inner N]
                                     [--out profiles/r27_explain.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

N_ITEMS, N_ATTRS, N_CTX, D, G, H, B, L, K, M_TOP = 12102, 4096, 6, 90, 450, 3, 128, 50, 10, 3


def _model(M, seed=0):
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


def aten_top_slots(pkg, model, prof, ctx, items, m):
    """explain_top_slots' outputs composed in ATen from the tensors the call itself stages (catalogue.carca_model_side):
    -> (slots [B, N, m], slot_items [B, N, m], contrib [B, N, m])."""
    side = pkg.catalogue.carca_model_side(model, prof, ctx, "bench_explain")
    qt, kk, uu, dq = side.qt, side.kk, side.uu, side.dq
    dh = D // H
    p_x = prof[0]
    valid = p_x != 0
    q = (qt[items][..., :D] + dq[:, None, :D]).view(B, -1, H, dh)
    k = kk.view(B, L, -1)[..., :D].view(B, L, H, dh)
    s = torch.einsum("bnhd,blhd->bhnl", q, k) / dh ** 0.5
    s = s.masked_fill(~valid[:, None, None, :], float("-inf"))
    w = torch.softmax(s, dim=-1)
    c = torch.einsum("bhnl,blh->bnl", w, uu.view(B, L, -1)[..., :H])
    top = torch.topk(c.masked_fill(~valid[:, None, :], float("-inf")), m, dim=-1)
    return top.indices, torch.gather(p_x[:, None, :].expand(-1, c.shape[1], -1), 2, top.indices), top.values


def run_explain(pkg, model, prof, ctx, gen, N, passes, inner):
    items = torch.randint(1, N_ITEMS, (B, N), generator=gen).cuda()
    # the composition computes what the kernel computes (every user here has a valid slot)
    got = model.explain_top_slots(prof, ctx, items, m=M_TOP)
    ref = aten_top_slots(pkg, model, prof, ctx, items, M_TOP)
    err = float((got[4] - ref[2]).abs().max())
    agree = float((got[2] == ref[0]).float().mean())
    fns = {
        "explain_items": lambda: model.explain_items(prof, ctx, items),
        "explain_top_slots": lambda: model.explain_top_slots(prof, ctx, items, m=M_TOP),
        "aten_top_slots": lambda: aten_top_slots(pkg, model, prof, ctx, items, M_TOP),
        "score_items": lambda: model.score_items(prof, ctx, items),
    }
    with torch.no_grad():
        series = _interleaved(fns, passes, inner)
    row = dict(N=N, m=M_TOP, aten_max_abs_diff=err, aten_slot_agreement=round(agree, 4))
    for name, ts in series.items():
        row[name] = _summary(ts)
    row["aten_over_explain_top_slots"] = round(row["aten_top_slots"]["ms"] / row["explain_top_slots"]["ms"], 2)
    return row


def run_serve(model, prof, ctx, gen, passes, inner):
    items = torch.randint(1, N_ITEMS, (B, K), generator=gen).cuda()
    fns = {
        "recommend": lambda: model.recommend(prof, ctx, k=K),
        "score_items_N10": lambda: model.score_items(prof, ctx, items),
    }
    if hasattr(model, "recommend_explained"):
        fns["recommend_explained"] = lambda: model.recommend_explained(prof, ctx, k=K, m=M_TOP)
    with torch.no_grad():
        series = _interleaved(fns, passes, inner)
    row = dict(k=K, m=M_TOP)
    for name, ts in series.items():
        row[name] = _summary(ts)
    row["recommend_plus_score_items"] = round(row["recommend"]["ms"] + row["score_items_N10"]["ms"], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", choices=("explain", "serve"), required=True)
    ap.add_argument("--label", default="this")
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--passes", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "r27_explain.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    import carca_replication_amd as pkg  # noqa: E402
    from carca_replication_amd import _lib, catalogue, modules  # noqa: E402,F401

    model = _model(modules)
    p_x, p_c, ctx, gen = _batch()
    prof = (p_x, None, p_c)
    rec = dict(config="C2", B=B, set=a.set, build=a.label, passes=a.passes, inner=a.inner)
    if a.set == "explain":
        rec["rows"] = [run_explain(pkg, model, prof, ctx, gen, N, a.passes, a.inner) for N in (10, 101, 1000)]
    else:
        rec["rows"] = [run_serve(model, prof, ctx, gen, a.passes, a.inner)]
    print(json.dumps(rec), flush=True)
    if a.out:
        recs = []
        if os.path.exists(a.out):
            with open(a.out) as f:
                recs = json.load(f)
        recs.append(rec)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
