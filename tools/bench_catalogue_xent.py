"""Full-catalogue softmax cross-entropy (ops.catalogue_xent, csrc/catalogue_xent.hip) timed with
device events:
  op   forward + backward of the fused kernels at C2 train shapes (B 128, L 50, lengths U{3..50} as BASELINE draws them,
       12,102 items, d 90) and at C4 dimensions (1,000,001 items, d 128, the same batch), beside the ATen composition
       (P @ T.T, F.cross_entropy, autograd) -- each with its peak memory beyond the inputs;
  step a whole engine.train_step at C2 with loss="softmax" against the BCE step (DotProduct decoder, AllEmbedding over a
       registered attribute table, 2 blocks).
The split by kernel comes from a separate rocprofv3 --kernel-trace --stats run of this script.
usage: python tools/bench_catalogue_xent.py [--reps N] [--config all|C2|C4|step] [--no-aten] [--out file.json]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_recommend import _time  # noqa: E402
from carca_replication_amd import engine, ops  # noqa: E402
from carca_replication_amd import modules as M  # noqa: E402

PEAK_TFLOPS = 157.3  # fp32 MFMA


def _batch(B, L, n_items, n_ctx, seed=1):
    gen = torch.Generator().manual_seed(seed)
    lens = torch.randint(3, L + 1, (B,), generator=gen)
    live = torch.arange(L) >= (L - lens).unsqueeze(1)
    p_x = torch.randint(1, n_items, (B, L), generator=gen) * live
    pos = torch.randint(1, n_items, (B, L), generator=gen) * live
    neg = torch.randint(1, n_items, (B, L), generator=gen) * live
    p_c = torch.rand(B, L, n_ctx, generator=gen) * live.unsqueeze(-1)
    return p_x.int().cuda(), pos.int().cuda(), neg.int().cuda(), p_c.cuda(), int(lens.sum())


def _peak(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def run_op(name, n_items, d, reps, aten):
    B, L = 128, 50
    _, pos, _, _, valid = _batch(B, L, n_items, 1)
    R = B * L
    ld = (d + 3) // 4 * 4
    g = torch.Generator(device="cuda").manual_seed(2)
    P = torch.zeros(R, ld, device="cuda")
    P[:, :d] = torch.randn(R, d, generator=g, device="cuda")
    T = torch.zeros(n_items, ld, device="cuda")
    T[:, :d] = torch.randn(n_items, d, generator=g, device="cuda") / d ** 0.5
    pos = pos.reshape(-1)
    one = torch.ones(1, device="cuda")
    out = dict(config=name, R=R, valid_rows=valid, n_items=n_items, d=d)

    def fwd():
        return ops.catalogue_xent_fwd(P, T, pos, d)

    def fwd_bwd():
        _, lse = fwd()
        return ops.catalogue_xent_bwd(P, T, pos, lse, one, d)

    plan = ops.catalogue_xent_plan(R, n_items, d, ops.num_cus())
    out["plan"] = {k: plan[k] for k in ("splits_items", "items_per_split", "splits_rows")}
    ms_f = _time(fwd, reps)
    ms_fb = _time(fwd_bwd, reps)
    ms_fb2 = _time(fwd_bwd, reps)
    out["ms_fwd"] = round(ms_f, 4)
    out["ms_fwd_bwd"] = round(min(ms_fb, ms_fb2), 4)
    out["ms_fwd_bwd_runs"] = [round(ms_fb, 4), round(ms_fb2, 4)]
    out["peak_mb_beyond_inputs"] = _peak(fwd_bwd)
    useful = 5 * 2.0 * valid * (n_items - 1) * d
    executed = 5 * 2.0 * (-(-valid // 64) * 64) * (-(-n_items // 64) * 64) * (-(-d // 16) * 16)
    out["gflop_useful"] = round(useful / 1e9, 1)
    out["gflop_executed"] = round(executed / 1e9, 1)
    out["frac_peak_executed"] = round(executed / (out["ms_fwd_bwd"] * 1e-3) / (PEAK_TFLOPS * 1e12), 3)
    out["frac_peak_useful"] = round(useful / (out["ms_fwd_bwd"] * 1e-3) / (PEAK_TFLOPS * 1e12), 3)
    if aten:
        Pa = P[:, :d].clone().requires_grad_(True)
        Ta = T[:, :d].clone().requires_grad_(True)
        ok = (pos >= 1) & (pos < n_items)
        rows = ok.nonzero().view(-1)
        tgt = pos[rows].long() - 1

        def aten_fb():
            Pa.grad = Ta.grad = None
            loss = F.cross_entropy(Pa[rows] @ Ta[1:].T, tgt)
            loss.backward()

        try:
            out["ms_aten_fwd_bwd"] = round(_time(aten_fb, reps), 4)
            out["aten_peak_mb_beyond_inputs"] = _peak(aten_fb)
        except torch.cuda.OutOfMemoryError:
            out["ms_aten_fwd_bwd"] = "out of memory"
        Pa.grad = Ta.grad = None
        torch.cuda.empty_cache()
    return out


def run_step(reps):
    n_items, n_attrs, n_ctx, d, g, H, B, L = 12102, 4096, 6, 90, 450, 3, 128, 50
    torch.manual_seed(0)
    model = M.CARCA(d, 0.0, M.AllEmbedding(n_items, d, g, n_ctx, n_attrs, M.IdentityEncoding()),
                    torch.nn.ModuleList([M.SelfAttentionBlock(d, H, 0.0, True) for _ in range(2)]),
                    M.DotProduct()).cuda().train()
    gen = torch.Generator(device="cuda").manual_seed(0)
    attrs = (torch.rand(n_items, n_attrs, generator=gen, device="cuda") < 0.01).float()
    attrs[0] = 0
    model.embeds.register_attr_table(attrs)
    from carca_replication_amd.optim import Adam

    optim = Adam(model.parameters(), lr=1e-4)
    p_x, pos, neg, p_c, valid = _batch(B, L, n_items, n_ctx)
    o_x = torch.cat([pos, neg], 1)
    y_true = torch.cat([(pos != 0).float(), torch.zeros(B, L, device="cuda")], 1)
    batch = (p_x, None, p_c, o_x, None, torch.cat([p_c, p_c], 1), y_true)
    out = dict(config="C2-train-step", B=B, L=L, valid_rows=valid, n_items=n_items, d=d)
    for kind in ("bce", "softmax", "bce", "softmax"):
        ms = _time(lambda: engine.train_step(model, optim, batch, loss=kind), reps)
        out.setdefault(f"ms_step_{kind}_runs", []).append(round(ms, 4))
    for kind in ("bce", "softmax"):
        out[f"ms_step_{kind}"] = min(out[f"ms_step_{kind}_runs"])
        out[f"peak_mb_step_{kind}"] = _peak(lambda: engine.train_step(model, optim, batch, loss=kind))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--config", default="all")
    ap.add_argument("--no-aten", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), cus=ops.num_cus(), results=[])
    if a.config in ("all", "C2"):
        res["results"].append(run_op("C2", 12102, 90, a.reps, not a.no_aten))
        print(json.dumps(res["results"][-1]), flush=True)
    if a.config in ("all", "C4"):
        res["results"].append(run_op("C4", 1_000_001, 128, max(2, a.reps // 5), not a.no_aten))
        print(json.dumps(res["results"][-1]), flush=True)
    if a.config in ("all", "step"):
        res["results"].append(run_step(a.reps))
        print(json.dumps(res["results"][-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
