"""Full-catalogue top-k (CARCA.recommend, csrc/recommend.hip) timed with device events: ms per batch of users, users/s and the
scoring kernel's executed fp32 flops as a fraction of the MI355X fp32 MFMA peak (157.3 TF/s), at
  C2  B = 128, 12,102 items, n_attrs 4096, d 90, g 450, H 3, 2 blocks, k = 10, exclude="profile": tables cached, the table
      build alone, and the chunked-forward alternative (every item as target groups of 1024);
  C4  dimensions d 128, g 640, H 4, 1,000,001 items (AllEmbedding over 64 attributes), B = 128.
Profile lengths U{3..50}, left-padded.  usage: python tools/bench_recommend.py [--reps N] [--no-c4] [--out file.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from carca_replication_amd import modules as M  # noqa: E402

PEAK_TF = 157.3


def _model(n_items, n_attrs, n_ctx, d, g, H, nb, density, seed=0):
    torch.manual_seed(seed)
    enc = M.IdentityEncoding()
    model = M.CARCA(d, 0.0, M.AllEmbedding(n_items, d, g, n_ctx, n_attrs, enc),
                    torch.nn.ModuleList([M.SelfAttentionBlock(d, H, 0.0, True) for _ in range(nb)]),
                    M.CrossAttentionBlock(d, H, 0.0, True)).cuda().eval()
    gen = torch.Generator(device="cuda").manual_seed(seed)
    attrs = (torch.rand(n_items, n_attrs, generator=gen, device="cuda") < density).float()
    attrs[0] = 0
    model.embeds.register_attr_table(attrs)
    return model


def _batch(B, L, n_items, n_ctx, seed=1):
    gen = torch.Generator().manual_seed(seed)
    lens = torch.randint(3, L + 1, (B,), generator=gen)
    p_x = torch.randint(1, n_items, (B, L), generator=gen) * (torch.arange(L) >= (L - lens).unsqueeze(1))
    p_c = torch.rand(B, L, n_ctx, generator=gen) * (p_x != 0).unsqueeze(-1)
    return p_x.cuda(), p_c.cuda(), torch.rand(B, n_ctx, generator=gen).cuda(), int(lens.sum())


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def _invalidate(model):
    for m in model.modules():
        for key in M._TABLE_KEYS:
            m.__dict__.pop(key, None)
    model.embeds.__dict__.pop("_fold_cache", None)


def run(name, n_items, n_attrs, d, g, H, reps, chunked):
    n_ctx, B, L, k = 6, 128, 50, 10
    model = _model(n_items, n_attrs, n_ctx, d, g, H, 2, 0.01 if n_attrs > 64 else 0.1)
    p_x, p_c, ctx, valid = _batch(B, L, n_items, n_ctx)
    with torch.no_grad():
        cached = _time(lambda: model.recommend((p_x, None, p_c), ctx, k=k), reps)

        def build():
            _invalidate(model)
            T = model.embeds.item_table()
            model.embeds.context_matrix(n_ctx)
            model.decoder.recommend_tables(T)
        table = _time(build, max(1, reps // 10))
        out = dict(config=name, n_items=n_items, d=d, H=H, B=B, k=k, ms_cached=round(cached, 4),
                   users_per_s=round(B / cached * 1e3, 1), ms_table_build=round(table, 4))
        # executed flops of the scoring kernel: per (user, item) pair and valid slot, 2 * DPO for the score + the softmax
        dpo = H * ((d // H + 15) // 16 * 16)
        flops = 2.0 * dpo * valid * (n_items - 1)
        out["scoring_gflop"] = round(flops / 1e9, 2)
        out["flop_fraction_of_fp32_mfma_peak"] = round(flops / (cached * 1e-3) / (PEAK_TF * 1e12), 4)
        if chunked:
            def fwd():
                for lo in range(1, n_items, 1024):
                    ids = torch.arange(lo, min(lo + 1024, n_items), device="cuda").expand(B, -1)
                    oc = ctx.unsqueeze(1).expand(B, ids.shape[1], n_ctx)
                    model((p_x, None, p_c), [(ids, None, oc)])
            ch = _time(fwd, max(1, reps // 10))
            out["ms_chunked_forward"] = round(ch, 3)
            out["speedup_vs_chunked"] = round(ch / cached, 1)
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
