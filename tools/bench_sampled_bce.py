"""BCE against K shared negatives, gBCE (ops.sampled_bce, csrc/sampled_bce.hip) timed with device
events:
  op   forward + backward of the fused kernels (with the context rows C) at C2 (12,102 items, d 90) and C4 dimensions
       (1,000,001 items, d 128) for K in {256, 1024, 8192} shared samples, at the train batch of
       tools/bench_sampled_xent.py (B 128, L 50; 6,400 rows), with the peak memory beyond the inputs.  --kind xent times
       section 14's ops.sampled_xent_fwd / _bwd at the same shapes instead: the yardstick.  One kind per process, so that
       a driver can alternate fresh processes of the two;
  step a whole eager engine.train_step at C2 and C4 dimensions (DotProduct, AllEmbedding over a registered attribute
       table, 2 blocks) with a fresh optimizer (at C4 the item table is a touched-row Adam table, and all three steps keep
       it sparse) for loss = bce, sampled_softmax (K = 8192) and sampled_bce (K = 256), with each step's peak memory.
The split by kernel comes from a separate rocprofv3 --kernel-trace --stats run of this script.
usage: python tools/bench_sampled_bce.py [--reps N] [--config all|op|step|C2|C4] [--kind bce|xent] [--package-root DIR]
       [--out file.json]"""
import argparse
import json
import math
import os
import sys

import torch

_root = argparse.ArgumentParser(add_help=False)
_root.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(_root.parse_known_args()[0].package_root))  # (the tree whose package is imported)
from carca_replication_amd import engine, ops  # noqa: E402  (before the helper tools: they put their own tree in front)
from carca_replication_amd import modules as M  # noqa: E402
from carca_replication_amd.optim import Adam  # noqa: E402
from carca_replication_amd.sampling import ItemSampler  # noqa: E402
from bench_catalogue_xent import PEAK_TFLOPS, _batch, _peak  # noqa: E402
from bench_recommend import _time  # noqa: E402

B, L = 128, 50
KS = (256, 1024, 8192)


def run_op(name, n_items, d, K, reps, kind):
    _, pos, _, _, valid = _batch(B, L, n_items, 1)
    R = B * L
    ld = (d + 3) // 4 * 4
    g = torch.Generator(device="cuda").manual_seed(2)
    P = torch.zeros(R, ld, device="cuda")
    P[:, :d] = torch.randn(R, d, generator=g, device="cuda")
    T = torch.zeros(n_items, ld, device="cuda")
    T[:, :d] = torch.randn(n_items, d, generator=g, device="cuda") / d ** 0.5
    Cr = torch.zeros(R, ld, device="cuda")
    Cr[:, :d] = torch.randn(R, d, generator=g, device="cuda") / d ** 0.5
    pos = pos.reshape(-1)
    s = torch.randint(1, n_items, (K,), device="cuda", generator=g)
    Tp, S = T[pos.long()], T[s]
    one = torch.ones(1, device="cuda")
    out = dict(kind=kind, config=name, R=R, valid_rows=valid, n_items=n_items, d=d, K=K)
    if kind == "bce":
        pos32, s32 = pos.int(), s.int()
        beta = ops.sampled_bce_beta(K, n_items, engine.SAMPLED_BCE_T)

        def fwd():
            return ops.sampled_bce_fwd(P, Tp, Cr, pos32, S, s32, n_items, beta, d)

        def fwd_bwd():
            _, saved, _ = fwd()
            return ops.sampled_bce_bwd(P, Tp, Cr, pos32, S, s32, n_items, beta, saved, one, d)

        plan = ops.sampled_bce_plan(R, K, d, ops.num_cus())
    else:
        log_q = torch.full((n_items,), -math.log(n_items - 1), device="cuda")
        log_q[0] = -float("inf")
        pos32, s32, bp, bs = ops.sampled_xent_corrections(pos, s, log_q)

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
    executed = 5 * 2.0 * (-(-valid // 64) * 64) * (-(-K // 64) * 64) * (-(-d // 16) * 16)
    out["gflop_executed"] = round(executed / 1e9, 2)
    out["frac_peak_executed"] = round(executed / (out["ms_fwd_bwd"] * 1e-3) / (PEAK_TFLOPS * 1e12), 3)
    return out


def run_step(name, n_items, d, g_, H, n_attrs, reps):
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
    samplers = dict(bce=None, sampled_softmax=ItemSampler(n_items, 8192),
                    sampled_bce=ItemSampler(n_items, engine.SAMPLED_BCE_DEFAULT_K))
    out = dict(config=name, B=B, L=L, valid_rows=valid, n_items=n_items, d=d, K_sampled_softmax=8192,
               K_sampled_bce=engine.SAMPLED_BCE_DEFAULT_K)
    optim = Adam(model.parameters(), lr=1e-4)  # fresh: every one of the three steps keeps a touched-row table sparse

    def step(kind):
        return lambda: engine.train_step(model, optim, batch, loss=kind, sampler=samplers[kind])

    kinds = tuple(samplers)
    for kind in kinds + kinds:
        out.setdefault(f"ms_step_{kind}_runs", []).append(round(_time(step(kind), reps), 4))
    for kind in kinds:
        out[f"ms_step_{kind}"] = min(out[f"ms_step_{kind}_runs"])
        out[f"peak_mb_step_{kind}"] = _peak(step(kind))
    st = optim.state[model.embeds.items_embed.weight]
    out["rows_touched"] = int(st["row_touched"].sum()) if "row_touched" in st else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--config", default="all")
    ap.add_argument("--kind", default="bce", choices=("bce", "xent"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--package-root", default=None, help="the tree whose package is imported (--kind xent on another "
                    "build of the library: the yardstick)")
    a = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), cus=ops.num_cus(), package=os.path.relpath(os.path.dirname(ops.__file__)), results=[])

    def emit(r):
        res["results"].append(r)
        print(json.dumps(r), flush=True)

    if a.config in ("all", "op", "C2"):
        for K in KS:
            emit(run_op("C2", 12102, 90, K, a.reps, a.kind))
    if a.config in ("all", "op", "C4"):
        for K in KS:
            emit(run_op("C4", 1_000_001, 128, K, a.reps, a.kind))
    if a.config in ("all", "step", "C2"):
        emit(run_step("C2-train-step", 12102, 90, 450, 3, 4096, a.reps))
    if a.config in ("all", "step", "C4"):
        emit(run_step("C4-train-step", 1_000_001, 128, 640, 4, 4096, max(2, a.reps // 2)))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
