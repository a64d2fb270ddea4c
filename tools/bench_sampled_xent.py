"""Sampled softmax cross-entropy with the logQ correction (ops.sampled_xent, csrc/sampled_xent.hip)
timed with device events:
  op   forward + backward of the fused kernels at C2 (12,102 items, d 90) and C4 dimensions (1,000,001 items, d 128) for
       K in {1024, 8192, 65536} shared samples, at the train batch of tools/bench_catalogue_xent.py (B 128, L 50), beside
       section 13's full-catalogue op and the ATen composition (gathered logits, masked logsumexp, autograd) -- each with
       its peak memory beyond the inputs;
  step a whole eager engine.train_step at C2 and C4 dimensions (DotProduct, AllEmbedding over a registered attribute
       table, 2 blocks) for loss = bce, softmax and sampled_softmax (K = 8192).  At C4 the item table is a touched-row
       Adam table: timed with a fresh optimizer (the sampled step keeps it sparse) and after one softmax step has marked
       every row (dense Adam from then on).
The split by kernel comes from a separate rocprofv3 --kernel-trace --stats run of this script.
usage: python tools/bench_sampled_xent.py [--reps N] [--config all|op|step|C2|C4] [--no-aten] [--out file.json]"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_catalogue_xent import PEAK_TFLOPS, _batch, _peak  # noqa: E402
from bench_recommend import _time  # noqa: E402
from carca_replication_amd import engine, ops  # noqa: E402
from carca_replication_amd import modules as M  # noqa: E402
from carca_replication_amd.optim import Adam  # noqa: E402
from carca_replication_amd.sampling import ItemSampler  # noqa: E402

B, L = 128, 50


def run_op(name, n_items, d, K, reps, aten, full):
    _, pos, _, _, valid = _batch(B, L, n_items, 1)
    R = B * L
    ld = (d + 3) // 4 * 4
    g = torch.Generator(device="cuda").manual_seed(2)
    P = torch.zeros(R, ld, device="cuda")
    P[:, :d] = torch.randn(R, d, generator=g, device="cuda")
    T = torch.zeros(n_items, ld, device="cuda")
    T[:, :d] = torch.randn(n_items, d, generator=g, device="cuda") / d ** 0.5
    pos = pos.reshape(-1)
    s = torch.randint(1, n_items, (K,), device="cuda", generator=g)
    log_q = torch.full((n_items,), -math.log(n_items - 1), device="cuda")
    log_q[0] = -float("inf")
    Tp, S = T[pos.long()], T[s]
    pos32, s32, bp, bs = ops.sampled_xent_corrections(pos, s, log_q)
    one = torch.ones(1, device="cuda")
    out = dict(config=name, R=R, valid_rows=valid, n_items=n_items, d=d, K=K)

    def fwd():
        return ops.sampled_xent_fwd(P, Tp, bp, pos32, S, s32, bs, n_items, d)

    def fwd_bwd():
        _, lse, row_loss = fwd()
        return ops.sampled_xent_bwd(P, Tp, bp, pos32, S, s32, bs, n_items, lse, row_loss, one, d)

    plan = ops.sampled_xent_plan(R, K, d, ops.num_cus())
    out["plan"] = {k: plan[k] for k in ("splits_samples", "samples_per_split", "splits_rows")}
    out["ms_fwd"] = round(_time(fwd, reps), 4)
    runs = [round(_time(fwd_bwd, reps), 4) for _ in range(2)]
    out["ms_fwd_bwd"], out["ms_fwd_bwd_runs"] = min(runs), runs
    out["peak_mb_beyond_inputs"] = _peak(fwd_bwd)
    # five products of 2 R K d each: the forward's logits, the backward's recomputed logits (twice) and its dP, dS
    useful = 5 * 2.0 * valid * K * d
    executed = 5 * 2.0 * (-(-valid // 64) * 64) * (-(-K // 64) * 64) * (-(-d // 16) * 16)
    out["gflop_useful"] = round(useful / 1e9, 2)
    out["gflop_executed"] = round(executed / 1e9, 2)
    out["frac_peak_executed"] = round(executed / (out["ms_fwd_bwd"] * 1e-3) / (PEAK_TFLOPS * 1e12), 3)
    if full:  # section 13's op over the whole catalogue, same rows
        def cx():
            _, lse = ops.catalogue_xent_fwd(P, T, pos32, d)
            return ops.catalogue_xent_bwd(P, T, pos32, lse, one, d)

        out["ms_catalogue_xent_fwd_bwd"] = round(_time(cx, max(2, reps // 5)), 4)
    if aten:
        Pa = P[:, :d].clone().requires_grad_(True)
        Ta = Tp[:, :d].clone().requires_grad_(True)
        Sa = S[:, :d].clone().requires_grad_(True)
        ok = (pos >= 1) & (pos < n_items)
        rows = ok.nonzero().view(-1)
        pv = pos[rows].long()
        hit = s.view(1, -1) == pv.view(-1, 1)

        def aten_fb():
            Pa.grad = Ta.grad = Sa.grad = None
            Pv = Pa[rows]
            zp = (Pv * Ta[rows]).sum(1) + bp[rows]
            zs = (Pv @ Sa.T + bs).masked_fill(hit, -float("inf"))
            loss = (torch.logsumexp(torch.cat([zp.view(-1, 1), zs], 1), 1) - zp).mean()
            loss.backward()

        try:
            out["ms_aten_fwd_bwd"] = round(_time(aten_fb, reps), 4)
            out["aten_peak_mb_beyond_inputs"] = _peak(aten_fb)
        except torch.cuda.OutOfMemoryError:
            out["ms_aten_fwd_bwd"] = "out of memory"
        Pa.grad = Ta.grad = Sa.grad = None
        torch.cuda.empty_cache()
    return out


def run_step(name, n_items, d, g_, H, n_attrs, reps, touched_row):
    n_ctx = 6
    torch.manual_seed(0)
    model = M.CARCA(d, 0.0, M.AllEmbedding(n_items, d, g_, n_ctx, n_attrs, M.IdentityEncoding()),
                    torch.nn.ModuleList([M.SelfAttentionBlock(d, H, 0.0, True) for _ in range(2)]),
                    M.DotProduct()).cuda().train()
    gen = torch.Generator(device="cuda").manual_seed(0)
    attrs = (torch.rand(n_items, n_attrs, generator=gen, device="cuda") < 0.01).float()
    attrs[0] = 0
    model.embeds.register_attr_table(attrs)
    p_x, pos, neg, p_c, valid = _batch(B, L, n_items, n_ctx)
    o_x = torch.cat([pos, neg], 1)
    y_true = torch.cat([(pos != 0).float(), torch.zeros(B, L, device="cuda")], 1)
    batch = (p_x, None, p_c, o_x, None, torch.cat([p_c, p_c], 1), y_true)
    sampler = ItemSampler(n_items, 8192)
    out = dict(config=name, B=B, L=L, valid_rows=valid, n_items=n_items, d=d, K=8192)

    def step(kind):
        return lambda: engine.train_step(model, optim, batch, loss=kind,
                                         sampler=sampler if kind == "sampled_softmax" else None)

    optim = Adam(model.parameters(), lr=1e-4)
    kinds = ("bce", "sampled_softmax")
    if touched_row:  # fresh optimizer: the BCE and sampled steps keep the item table's Adam sparse
        for kind in kinds + kinds:
            out.setdefault(f"ms_step_{kind}_sparse_runs", []).append(round(_time(step(kind), reps), 4))
        for kind in kinds:
            out[f"ms_step_{kind}_sparse"] = min(out[f"ms_step_{kind}_sparse_runs"])
            out[f"peak_mb_step_{kind}_sparse"] = _peak(step(kind))
        st = optim.state[model.embeds.items_embed.weight]
        out["rows_touched_before_softmax"] = int(st["row_touched"].sum()) if "row_touched" in st else None
    # a softmax step marks every row: dense Adam from here on
    kinds = ("bce", "softmax", "sampled_softmax")
    sreps = max(2, reps // 5) if touched_row else reps
    for kind in kinds + kinds:
        out.setdefault(f"ms_step_{kind}_runs", []).append(round(_time(step(kind), sreps if kind == "softmax" else reps), 4))
    for kind in kinds:
        out[f"ms_step_{kind}"] = min(out[f"ms_step_{kind}_runs"])
        out[f"peak_mb_step_{kind}"] = _peak(step(kind))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--config", default="all")
    ap.add_argument("--no-aten", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), cus=ops.num_cus(), results=[])

    def emit(r):
        res["results"].append(r)
        print(json.dumps(r), flush=True)

    if a.config in ("all", "op", "C2"):
        for K in (1024, 8192, 65536):
            emit(run_op("C2", 12102, 90, K, a.reps, not a.no_aten, K == 1024))
    if a.config in ("all", "op", "C4"):
        for K in (1024, 8192, 65536):
            emit(run_op("C4", 1_000_001, 128, K, a.reps, not a.no_aten, K == 1024))
    if a.config in ("all", "step", "C2"):
        emit(run_step("C2-train-step", 12102, 90, 450, 3, 4096, a.reps, False))
    if a.config in ("all", "step", "C4"):
        emit(run_step("C4-train-step", 1_000_001, 128, 640, 4, 4096, max(2, a.reps // 2), True))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
