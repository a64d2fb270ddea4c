"""Softmax cross-entropy over per-user negative lists (ops.listed_xent, csrc/listed_xent.hip) timed
with device events:
  op   forward + backward of the fused kernels at C2 (12,102 items, d 90) and C4 dimensions (1,000,001 items, d 128) for
       N in {128, 1024, 4096} entries per user, at the train batch of tools/bench_catalogue_xent.py (G = B = 128 lists,
       rows_per_list = L = 50, about half the rows valid), beside (a) the ATen composition (a gathered [G, N, d] copy of
       the item rows, bmm, masked logsumexp, autograd, whose index_add_ backward uses float atomics) and (b)
       ops.sampled_xent at K = N shared samples and the same rows: full 64-row tiles and no gather, a floor and not a
       target.  The three are measured in turn, --rounds times; medians with min and max, and each one's peak memory
       beyond the inputs;
  step engine.hard_negative_step at C2 and C4 dimensions (DotProduct, AllEmbedding over a registered attribute table, 2
       blocks) with n_hard = 1000 and n_uniform = 0 / 1000, split into the mining (the item-side table rebuild timed
       apart from a retrieve over warm tables), the loss forward + backward and the optimizer, beside the bce and
       sampled_softmax train_steps.
The split by kernel comes from a separate rocprofv3 --kernel-trace --stats run of this script.
usage: python tools/bench_listed_xent.py [--reps N] [--rounds N] [--config all|op|step|C2|C4] [--no-aten] [--out file.json]"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_catalogue_xent import _batch, _peak  # noqa: E402
from bench_recommend import _invalidate, _time  # noqa: E402
from carca_replication_amd import engine, ops  # noqa: E402
from carca_replication_amd import modules as M  # noqa: E402
from carca_replication_amd.catalogue import NegativeLists  # noqa: E402
from carca_replication_amd.optim import Adam  # noqa: E402
from carca_replication_amd.sampling import HardNegativeMiner, ItemSampler  # noqa: E402

B, L = 128, 50


def _stats(runs):
    return dict(median=round(statistics.median(runs), 4), min=round(min(runs), 4), max=round(max(runs), 4))


def run_op(name, n_items, d, N, reps, rounds, aten):
    _, pos, _, _, valid = _batch(B, L, n_items, 1)
    R = B * L
    ld = (d + 3) // 4 * 4
    g = torch.Generator(device="cuda").manual_seed(2)
    P = torch.zeros(R, ld, device="cuda")
    P[:, :d] = torch.randn(R, d, generator=g, device="cuda")
    T = torch.zeros(n_items, ld, device="cuda")
    T[:, :d] = torch.randn(n_items, d, generator=g, device="cuda") / d ** 0.5
    pos = pos.reshape(-1)
    nl = NegativeLists(torch.randint(1, n_items, (B, N), device="cuda", generator=g), n_items)
    U = len(nl)
    Tp, S = T[pos.long()], T[nl.ids.long()]
    pos32 = pos.to(torch.int32)
    one = torch.ones(1, device="cuda")
    plan = ops.listed_xent_plan(B, L, N, U, d, ops.num_cus())
    out = dict(config=name, G=B, rows_per_list=L, R=R, valid_rows=valid, n_items=n_items, d=d, N=N, U=U,
               plan={k: plan[k] for k in ("splits", "entries_per_split")}, scratch_bwd_mb=round(plan["scratch_bwd"] * 4 / 2 ** 20, 1))

    def fwd():
        return ops.listed_xent_fwd(P, Tp, pos32, S, nl.lists, nl.index, L, None, None, n_items, d)

    def fwd_bwd():
        _, lse, row_loss = fwd()
        return ops.listed_xent_bwd(P, Tp, pos32, S, nl.lists, nl.index, L, None, None, n_items, (nl.csr_off, nl.csr_ent),
                                   lse, row_loss, one, d)

    # (b) K = N samples shared by the batch: the same products on full tiles, no gather
    s = torch.randint(1, n_items, (N,), device="cuda", generator=g)
    log_q = torch.full((n_items,), -math.log(n_items - 1), device="cuda")
    log_q[0] = -float("inf")
    Ss = T[s]
    p32, s32, bp, bs = ops.sampled_xent_corrections(pos, s, log_q)

    def sampled_fb():
        _, lse, row_loss = ops.sampled_xent_fwd(P, Tp, bp, p32, Ss, s32, bs, n_items, d)
        return ops.sampled_xent_bwd(P, Tp, bp, p32, Ss, s32, bs, n_items, lse, row_loss, one, d)

    series = {"listed": fwd_bwd, "sampled": sampled_fb}
    if aten:  # (a) gather, bmm, masked logsumexp, autograd
        Pa = P[:, :d].clone().requires_grad_(True)
        Ta = Tp[:, :d].clone().requires_grad_(True)
        Sa = S[:, :d].clone().requires_grad_(True)
        ok = ((pos >= 1) & (pos < n_items)).view(B, L)
        idx = nl.index.long().clamp(min=0)
        dead = (nl.index < 0).view(B, 1, N) | (nl.lists.view(B, 1, N) == pos.view(B, L, 1))
        nvalid = ok.sum()

        def aten_fb():
            Pa.grad = Ta.grad = Sa.grad = None
            zp = (Pa * Ta).sum(1).view(B, L)
            zs = torch.bmm(Pa.view(B, L, d), Sa[idx].transpose(1, 2)).masked_fill(dead, -float("inf"))
            row = torch.logsumexp(torch.cat([zp.unsqueeze(2), zs], 2), 2) - zp
            loss = (row * ok).sum() / nvalid
            loss.backward()

        series["aten"] = aten_fb
    runs = {k: [] for k in series}
    for _ in range(rounds):  # in turn: a drift of the clocks lands on every series alike
        for k, fn in series.items():
            runs[k].append(_time(fn, reps))
    out["ms_fwd"] = round(_time(fwd, reps), 4)
    for k in series:
        out[f"ms_{k}_fwd_bwd"] = _stats(runs[k])
        out[f"{k}_peak_mb_beyond_inputs"] = _peak(series[k])
    out["ratio_to_sampled"] = round(out["ms_listed_fwd_bwd"]["median"] / out["ms_sampled_fwd_bwd"]["median"], 2)
    out["own_tile_fill"] = round(valid / B / 64, 2)  # valid rows per 64-row own tile (one tile per group at L = 50)
    if aten:
        out["bar_median_le_aten_max"] = out["ms_listed_fwd_bwd"]["median"] <= out["ms_aten_fwd_bwd"]["max"]
        Pa.grad = Ta.grad = Sa.grad = None
    torch.cuda.empty_cache()
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
    prof = (p_x, None, p_c)
    optim = Adam(model.parameters(), lr=1e-4)
    sampler = ItemSampler(n_items, 8192)
    out = dict(config=name, B=B, L=L, valid_rows=valid, n_items=n_items, d=d, n_hard=1000)
    for kind in ("bce", "sampled_softmax"):
        out[f"ms_step_{kind}"] = round(_time(lambda: engine.train_step(
            model, optim, batch, loss=kind, sampler=sampler if kind == "sampled_softmax" else None), reps), 4)
    for n_uniform in (0, 1000):
        miner = HardNegativeMiner(n_hard=1000, n_uniform=n_uniform)
        key = f"uniform{n_uniform}"
        out[f"ms_step_hard_{key}"] = round(_time(lambda: engine.hard_negative_step(model, optim, batch, miner), reps), 4)

        def mine_cold():
            _invalidate(model)
            return miner.mine(model, prof, pos)

        out[f"ms_mine_with_table_rebuild_{key}"] = round(_time(mine_cold, reps), 4)
        out[f"ms_mine_warm_tables_{key}"] = round(_time(lambda: miner.mine(model, prof, pos), reps), 4)
        nl = miner.mine(model, prof, pos)
        out[f"U_{key}"] = len(nl)

        def loss_fb():
            optim.zero_grad(set_to_none=True)
            model.listed_softmax_loss(prof, pos, nl).backward()

        out[f"ms_loss_fwd_bwd_{key}"] = round(_time(loss_fb, reps), 4)
        out[f"ms_optimizer_{key}"] = round(_time(optim.step, reps), 4)
        out[f"peak_mb_step_hard_{key}"] = _peak(lambda: engine.hard_negative_step(model, optim, batch, miner))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--config", default="all")
    ap.add_argument("--no-aten", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), cus=ops.num_cus(), results=[])

    def emit(r):
        res["results"].append(r)
        print(json.dumps(r), flush=True)

    if a.config in ("all", "op", "C2"):
        for N in (128, 1024, 4096):
            emit(run_op("C2", 12102, 90, N, a.reps, a.rounds, not a.no_aten))
    if a.config in ("all", "op", "C4"):
        for N in (128, 1024, 4096):
            emit(run_op("C4", 1_000_001, 128, N, a.reps, a.rounds, not a.no_aten))
    if a.config in ("all", "step", "C2"):
        emit(run_step("C2-hard-negative-step", 12102, 90, 450, 3, 4096, a.reps))
    if a.config in ("all", "step", "C4"):
        emit(run_step("C4-hard-negative-step", 1_000_001, 128, 640, 4, 4096, max(2, a.reps // 4)))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
