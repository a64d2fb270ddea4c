"""Bit fingerprints of the full-catalogue calls (CARCA.recommend / rank_items over csrc/catalogue_sweep.h, recommend.hip and
rank.hip; KNN.recommend / rank_items over csrc/knn_catalogue.hip; DESIGN.md sections 10-12): for a fixed list of seeded
cases, one sha256 per output tensor -- `scores` and `ids` of recommend, `scores` and `ranks` of rank_items.  These kernels
use integer atomics only and every float sum in them has one fixed order, so a change that only moves code must leave
every line as it was: run the script once per build (a fresh process each, --package-root naming the tree whose package
is imported) on the same machine and compare the listings line for line.  The sweep grid depends on the CU count (first
line).  The cases: the three decoders (cross-attention with and without residual, DotProduct, WeightedDotProduct
normalised and not) with and without a context matrix (AllEmbedding, IdEmbedding); a geometry of each DPI (64, 96, 128),
(96, 48, 2) and (128, 64, 2) among them; a user with an empty profile and one with a single item; n_items off the 256-item
tile; more users than user chunks; k = 1, 10, 128; lists of 1, 101 and 128 ids holding id 0, out-of-range, repeated and
excluded ids; exclude = "profile", None and a [B, 1100] tensor with zeros and duplicates; fewer eligible items than k;
KNN in table mode on a multi-hot table (i8) and on real-valued tables (fp32, F % 4 != 0 too) and in dense mode; the C2
shapes of tools/bench_recommend.py and tools/bench_knn_catalogue.py.  Every CARCA case ends with the calls restricted to
candidate sets (lines named .../among-...): a tenth of the catalogue, a set of 257 ids (one past a
tile; the whole catalogue where it is smaller) and the empty set, drawn after everything else so that the unrestricted
lines keep their inputs; --no-candidates leaves them out, for a tree from before the candidate sets.  Last come the
similar_items lines (csrc/similar_items.hip, csrc/row_stream.h; section 17): ops.similar_rows at a width for the
query-stationary kernel and five for the streaming one, cosine and dot, with and without the query's own row and a
candidate list, for 5 and 70 queries (invalid and repeated ids among them) and every item, one call per width and metric
forced into six chunks; and KNN.similar_items on a table it uses as it is and on one it pads.
usage: python tools/catalogue_bits.py [--package-root DIR] [--no-candidates] [--out listing.txt]"""
import argparse
import hashlib
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--no-candidates", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.package_root))

import torch  # noqa: E402

from carca_replication_amd import modules as M  # noqa: E402
from carca_replication_amd import ops  # noqa: E402

# (name, d, H, embedding, decoder, residual / normalised, L, B, n_items, n_attrs, g, blocks)
CARCA_CASES = [
    ("ca-res-all-64x4", 64, 4, "all", "ca", True, 16, 100, 3001, 12, 24, 1),       # (DPI, DHP, H) = (64, 16, 4)
    ("ca-nores-id-96x2", 96, 2, "id", "ca", False, 17, 100, 3001, 0, 0, 1),        # (96, 48, 2), no context matrix
    ("ca-res-all-128x2", 128, 2, "all", "ca", True, 50, 100, 3001, 12, 24, 2),     # (128, 64, 2)
    ("ca-res-id-90x3", 90, 3, "id", "ca", True, 64, 7, 700, 0, 0, 1),              # (96, 32, 3), d < DPI
    ("dot-id-64", 64, 2, "id", "dot", False, 16, 100, 3001, 0, 0, 1),
    ("dot-all-128", 128, 4, "all", "dot", False, 16, 100, 3001, 12, 24, 1),
    ("wdot-all-90", 90, 3, "all", "wdot", False, 50, 100, 3001, 12, 24, 1),        # DPI 96
    ("wdot-l2-all-128", 128, 4, "all", "wdot", True, 17, 100, 3001, 12, 24, 1),
    ("wdot-l2-id-64", 64, 1, "id", "wdot", True, 17, 100, 3001, 0, 0, 1),
    ("few-items-ca", 64, 4, "all", "ca", True, 16, 5, 40, 12, 24, 1),              # fewer eligible items than k
    ("few-items-dot", 64, 2, "id", "dot", False, 16, 5, 40, 0, 0, 1),
]
C2 = ("C2", 90, 3, "all", "ca", True, 50, 128, 12102, 4096, 450, 2)
N_CTX = 6
# (name, table kind, n_items, F, B, L, dense mode)
KNN_CASES = [
    ("multihot-i8", "multihot", 3001, 200, 100, 9, False),
    ("real-fp32-f130", "real", 3001, 130, 100, 9, False),      # F % 4 != 0: the scalar-load variant
    ("real-fp32-f128", "real", 3001, 128, 70, 1, False),
    ("dense", "multihot", 3001, 200, 100, 9, True),
    ("few-items", "multihot", 40, 64, 5, 9, False),
    ("C2-i8", "multihot", 12102, 4096, 128, 50, False),
    ("C2-fp32", "real", 12102, 4096, 128, 50, False),
]
# row widths of the similar_items cases: 90 the query-stationary kernel, the others the streaming one (csrc/row_stream.h) at
# 9, 16, 17, 65 and 257 chunks of 16 columns
SIMILAR_WIDTHS = [90, 132, 256, 260, 1028, 4102]
SIMILAR_METRICS = ("cosine", "dot")
# (name, table kind, n_items, F): KNN.similar_items on the table itself and on its zero-padded copy (F % 4 != 0)
KNN_SIMILAR_CASES = [("multihot-f200", "multihot", 3001, 200), ("real-f130", "real", 3001, 130)]


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _profile(g, B, L, n_items):
    lens = torch.randint(1, L + 1, (B,), generator=g)
    p_x = torch.randint(1, n_items, (B, L), generator=g) * (torch.arange(L) >= (L - lens).unsqueeze(1))
    if B > 2:
        p_x[1] = 0                      # an empty profile
        p_x[2, :L - 1] = 0              # a single item
    return p_x


def _lists(g, B, N, n_items, p_x):
    it = torch.randint(1, n_items, (B, N), generator=g)
    if N >= 5:
        it[0, 0] = 0                    # padding id
        it[0, 1] = n_items + 3          # out of range
        it[0, 2] = it[0, 3]             # repeated
        it[0, 4] = p_x[0, -1]           # a profile item: excluded under "profile", still ranked
        it[B - 1, N - 1] = -7
        it[B - 1, 0] = 2 ** 40 + 7      # beyond int32
    return it


def _exclude(g, B, n_items, lists):
    """[B, 1100] (more than the correction kernel's chunk of 1,024): zeros, duplicates, ids outside the catalogue and
    one listed item per user."""
    ex = torch.randint(0, n_items, (B, 1100), generator=g)
    ex[:, 5::7] = 0
    ex[:, 1050:1080] = ex[:, 20:50]
    ex[:, 3] = n_items
    ex[:, 4] = -4
    ex[:, 1099] = lists[:, 0]
    return ex


def _calls(name, model, prof, ctx, g, B, n_items, p_x, among=False):
    """The six calls of a case: k = 1 / 10 / 128 and N = 1 / 101 / 128 against the three kinds of exclusion; with `among`,
    four more per candidate set."""
    lists = {N: _lists(g, B, N, n_items, p_x) for N in (1, 101, 128)}
    ex = _exclude(g, B, n_items, lists[101]).cuda()
    out = []
    with torch.no_grad():
        for k, e, tag in ((1, ex, "tensor"), (10, None, "none"), (128, "profile", "profile")):
            s, i = model.recommend(prof, ctx, k=k, exclude=e)
            out += [(f"{name}/recommend-k{k}-{tag}/scores", _sha(s)), (f"{name}/recommend-k{k}-{tag}/ids", _sha(i))]
        for N, e, tag in ((1, "profile", "profile"), (101, ex, "tensor"), (128, None, "none")):
            s, r = model.rank_items(prof, ctx, lists[N].cuda(), exclude=e)
            out += [(f"{name}/rank-N{N}-{tag}/scores", _sha(s)), (f"{name}/rank-N{N}-{tag}/ranks", _sha(r))]
        for c in (max(1, n_items // 10), min(257, n_items - 1), 0) if among else ():
            S = (torch.randperm(n_items - 1, generator=g)[:c] + 1).cuda()  # (unsorted: the call normalises it)
            for k, e, tag in ((10, ex, "tensor"), (128, "profile", "profile")):
                s, i = model.recommend(prof, ctx, k=k, exclude=e, candidates=S)
                out += [(f"{name}/among-{c}/recommend-k{k}-{tag}/scores", _sha(s)),
                        (f"{name}/among-{c}/recommend-k{k}-{tag}/ids", _sha(i))]
            for N, e, tag in ((1, "profile", "profile"), (101, ex, "tensor")):
                s, r = model.rank_items(prof, ctx, lists[N].cuda(), exclude=e, candidates=S)
                out += [(f"{name}/among-{c}/rank-N{N}-{tag}/scores", _sha(s)),
                        (f"{name}/among-{c}/rank-N{N}-{tag}/ranks", _sha(r))]
    return out


def carca_case(seed, name, d, H, emb, dec, flag, L, B, n_items, n_attrs, g_dim, nb):
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    enc = M.IdentityEncoding()
    n_ctx = N_CTX if emb == "all" else 0
    embeds = (M.AllEmbedding(n_items, d, g_dim, n_ctx, n_attrs, enc) if emb == "all" else M.IdEmbedding(n_items, d, enc))
    decoder = (M.CrossAttentionBlock(d, H, 0.0, flag) if dec == "ca" else
               M.DotProduct() if dec == "dot" else M.WeightedDotProduct(0.9, L, flag, "cpu"))
    blocks = torch.nn.ModuleList([M.SelfAttentionBlock(d, H, 0.0, True) for _ in range(nb)])
    model = M.CARCA(d, 0.0, embeds, blocks, decoder).cuda().eval()
    if emb == "all":
        attrs = (torch.rand(n_items, n_attrs, generator=g) < (0.01 if n_attrs > 64 else 0.3)).float()
        attrs[0] = 0
        model.embeds.register_attr_table(attrs.cuda())
    p_x = _profile(g, B, L, n_items)
    p_c = torch.rand(B, L, n_ctx, generator=g) * (p_x != 0).unsqueeze(-1)
    ctx = torch.rand(B, n_ctx, generator=g).cuda() if n_ctx else None
    return _calls("carca/" + name, model, (p_x.cuda(), None, p_c.cuda()), ctx, g, B, n_items, p_x,
                  among=not args.no_candidates)


def knn_case(seed, name, kind, n_items, F, B, L, dense):
    g = torch.Generator().manual_seed(seed)
    if kind == "multihot":
        A = (torch.rand(n_items, F, generator=g) < (0.01 if F > 1000 else 0.2)).float()
    else:
        A = torch.rand(n_items, F, generator=g) * 2 - 1
    A[0] = 0
    model = M.KNN().cuda()
    model.register_attr_table(A.cuda())
    p_x = _profile(g, B, L, n_items)
    p_a = torch.rand(B, L, F, generator=g).cuda() if dense else None
    return _calls("knn/" + name, model, (p_x.cuda(), p_a, None), None, g, B, n_items, p_x)


def similar_case(seed, K):
    """ops.similar_rows over a randn [333, K] table (five 64-row workgroups and a 13-row wave), its columns past K poisoned."""
    n = 333
    g = torch.Generator().manual_seed(seed)
    ld = (K + 3) // 4 * 4
    X = torch.full((n, ld), float("nan"))
    X[:, :K] = torch.randn(n, K, generator=g)
    X[0, :K] = 0
    X = X.cuda()
    q70 = torch.randint(1, n, (70,), generator=g)
    q70[3], q70[4], q70[5], q70[6], q70[69] = 0, n, -2, q70[7], q70[8]  # invalid ids and duplicates
    queries = {"Q5": q70[:5].cuda(), "Q70": q70.cuda(), "all": None}
    cands = (torch.randperm(n - 1, generator=g)[:150] + 1).cuda()
    out = []
    for metric in SIMILAR_METRICS:
        for self_ in (True, False):
            for S, stag in ((None, "none"), (cands, "among-150")):
                for qtag in ("Q70",) if (S is not None or not self_) else queries:
                    s, i = ops.similar_rows(X, K, queries[qtag], 20, metric, exclude_self=self_, candidates=S)
                    tag = f"similar/K{K}/{metric}-{'noself' if self_ else 'self'}-{stag}-{qtag}"
                    out += [(tag + "/scores", _sha(s)), (tag + "/ids", _sha(i))]
        # every item as a query, in chunks of 64 (six launches of the scoring kernel)
        s, i = ops.similar_rows(X, K, None, 128, metric, max_scratch_bytes=4 * 64 * n + 100)
        out += [(f"similar/K{K}/{metric}-chunked/scores", _sha(s)), (f"similar/K{K}/{metric}-chunked/ids", _sha(i))]
    return out


def knn_similar_case(seed, name, kind, n_items, F):
    g = torch.Generator().manual_seed(seed)
    A = (torch.rand(n_items, F, generator=g) < 0.2).float() if kind == "multihot" else torch.rand(n_items, F, generator=g) * 2 - 1
    A[0] = 0
    model = M.KNN().cuda()
    model.register_attr_table(A.cuda())
    ids = torch.randint(1, n_items, (70,), generator=g).cuda()
    out = []
    for metric in SIMILAR_METRICS:
        s, i = model.similar_items(ids, 20, metric, exclude_self=metric == "cosine")
        out += [(f"knn-similar/{name}/{metric}/scores", _sha(s)), (f"knn-similar/{name}/{metric}/ids", _sha(i))]
    return out


def main():
    assert torch.cuda.is_available(), "catalogue_bits.py needs a GPU"
    lines = [f"# cus={ops.num_cus()}"]
    for i, case in enumerate(CARCA_CASES + [C2]):
        lines += [f"{k} {h}" for k, h in carca_case(300 + i, *case)]
    for i, case in enumerate(KNN_CASES):
        lines += [f"{k} {h}" for k, h in knn_case(400 + i, *case)]
    for i, K in enumerate(SIMILAR_WIDTHS):
        lines += [f"{k} {h}" for k, h in similar_case(500 + i, K)]
    for i, case in enumerate(KNN_SIMILAR_CASES):
        lines += [f"{k} {h}" for k, h in knn_similar_case(600 + i, *case)]
    torch.cuda.synchronize()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
