"""Row log-softmax with a temperature and per-row exclusion (ops.policy_xent_fwd / _bwd, csrc/policy_xent.hip; DESIGN.md
section 29) timed with device events against ops.catalogue_xent_fwd / _bwd at the same shapes, interleaved in one process:
rounds of passes over every configuration in turn, the median over the rounds, and the baseline's own max - min over the
rounds as the margin.  Shapes: C2 (12,102 items, d 90) and C4 dimensions (1,000,001 items, d 128), B 128, L 50.
  base      catalogue_xent forward + backward over the batch's valid rows (section 13's op, unchanged);
  i         policy_xent over the same rows, no lists: the same products plus one multiply per logit; i_ent with the entropy;
  base128 / i128   the two at R = 128, every row valid;
  ii        the bandit shape as engine.off_policy_step runs it (last_slot_only): the 128 rows of the last slot, exclude =
            "profile" (one list of L ids per row), the lists sorted and transposed inside the timed region; ii_ent with the
            entropy; ii - i128 is what the exclusion costs;
  ii_rows   the same through the general route: all [B, L] rows of which only the last slot's 128 are valid, a list of L
            ids per row; ii_rows_none without lists.
usage: python tools/bench_policy_xent.py [--reps N] [--rounds N] [--config all|C2|C4] [--out file.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_catalogue_xent import _batch  # noqa: E402
from bench_recommend import _time  # noqa: E402
from carca_replication_amd import catalogue_xent, ops  # noqa: E402


def _operand(rows, d, g, scale=1.0):
    ld = (d + 3) // 4 * 4
    x = torch.zeros(rows, ld, device="cuda")
    x[:, :d] = torch.randn(rows, d, generator=g, device="cuda") * scale
    return x


def run(name, n_items, d, reps, rounds):
    B, L, tau = 128, 50, 0.5
    p_x, pos, _, _, n_valid = _batch(B, L, n_items, 1)
    R = B * L
    g = torch.Generator(device="cuda").manual_seed(2)
    P, T = _operand(R, d, g), _operand(n_items, d, g, d ** -0.5)
    P128 = P[:128].contiguous()
    pos_all = pos.reshape(-1)
    pos128 = torch.randint(1, n_items, (128,), generator=g, device="cuda").int()
    last = torch.zeros(B, L, dtype=torch.int32, device="cuda")
    last[:, L - 1] = pos128
    last = last.reshape(-1)
    one = torch.ones(1, device="cuda")
    c = torch.randn(R, generator=g, device="cuda")
    h = torch.randn(R, generator=g, device="cuda") * 0.01

    def base(Pm, items):
        def f():
            _, lse = ops.catalogue_xent_fwd(Pm, T, items, d)
            return ops.catalogue_xent_bwd(Pm, T, items, lse, one, d)
        return f

    def policy(Pm, items, ent, lists):
        n = Pm.shape[0]

        def f():
            ex = None
            if lists == "rows":
                ex = ops.policy_exclusion(catalogue_xent.profile_exclusion(p_x).reshape(R, L), R, n_items)
            elif lists == "last":
                ex = ops.policy_exclusion(p_x, B, n_items)
            lp, valid, H, lse = ops.policy_xent_fwd(Pm, T, items, d, tau, ex, ent)
            return ops.policy_xent_bwd(Pm, T, items, d, tau, ex, lse, c[:n], h[:n] if ent else None, H, valid)
        return f

    cases = dict(base=base(P, pos_all), i=policy(P, pos_all, False, None), i_ent=policy(P, pos_all, True, None),
                 base128=base(P128, pos128), i128=policy(P128, pos128, False, None),
                 ii=policy(P128, pos128, False, "last"), ii_ent=policy(P128, pos128, True, "last"),
                 ii_rows=policy(P, last, False, "rows"), ii_rows_none=policy(P, last, False, None))
    runs = {k: [] for k in cases}
    for _ in range(rounds):
        for k, f in cases.items():
            runs[k].append(_time(f, reps))
    med = {k: statistics.median(v) for k, v in runs.items()}
    spread = max(runs["base"]) - min(runs["base"])
    spread128 = max(runs["base128"]) - min(runs["base128"])
    out = dict(config=name, n_items=n_items, d=d, R=R, valid_rows=n_valid, temperature=tau, reps=reps, rounds=rounds,
               ms_median={k: round(v, 4) for k, v in med.items()},
               ms_runs={k: [round(x, 4) for x in v] for k, v in runs.items()},
               base_spread_ms=round(spread, 4), base128_spread_ms=round(spread128, 4),
               i_minus_base_ms=round(med["i"] - med["base"], 4),
               i_within_base_spread=bool(med["i"] - med["base"] <= spread),
               entropy_cost_ms=round(med["i_ent"] - med["i"], 4),
               ii_minus_i128_ms=round(med["ii"] - med["i128"], 4),
               ii_no_more_than_i128=bool(med["ii"] <= med["i128"]),
               exclusion_cost_ms=round(med["ii"] - med["i128"], 4),
               exclusion_within_base128_spread=bool(med["ii"] - med["i128"] <= spread128),
               exclusion_cost_rows_ms=round(med["ii_rows"] - med["ii_rows_none"], 4))
    # the lists' host side alone (device-side torch ops): the sort of the forward, the transposed build of the backward
    ex = ops.policy_exclusion(p_x, B, n_items)
    valid = ops.policy_valid_rows(pos128, ex, n_items)
    out["ms_lists_sort"] = round(_time(lambda: ops.policy_exclusion(p_x, B, n_items), reps), 4)
    out["ms_lists_transpose"] = round(_time(lambda: ops.policy_transposed_lists(ex, valid, n_items), reps), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--config", default="all")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), cus=ops.num_cus(), results=[])
    if a.config in ("all", "C2"):
        res["results"].append(run("C2", 12102, 90, a.reps, a.rounds))
        print(json.dumps(res["results"][-1]), flush=True)
    if a.config in ("all", "C4"):
        res["results"].append(run("C4", 1_000_001, 128, max(2, a.reps // 5), a.rounds))
        print(json.dumps(res["results"][-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
