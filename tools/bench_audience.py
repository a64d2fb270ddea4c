"""CARCA.recommend_users(k=10) -- the k best users of a batch for each of Q listed items -- timed
with device events at C2 dimensions (12,102 items, n_attrs 4096, d 90, g 450, H 3, 2 blocks), for 128 and 4096 users per
call and Q = 1, 64, 1024 and the whole catalogue, in the same process and session as
  recommend(k=1, candidates=S)   the same scoring and exclusion launches behind the same model side, with a small selection
                                 launch in place of the merge: what the call costs before it selects anything;
  the ATen composition           score_items on the list broadcast to every user, a masked fill for the exclusion and
                                 torch.topk over dim 0.  The broadcast list and the [B, Q] exclusion mask are built
                                 beforehand and not timed, which favours this route; it has no tie rule, selects on
                                 linked scores and materialises [B, Q] twice.
The model side all three share (the profile encoder and the per-user tables, catalogue.carca_model_side) is timed alone as
well, so that the launches behind it can be read off by subtraction.  The four are timed in interleaved passes and the
smallest pass is kept.  Every row also says whether recommend_users'
scores equal the composition's values bit for bit, and the time per update of a 64-update walk through one
catalogue.AudienceTopK (128 users per update, running user ids).  Models and batches are bench_recommend.py's.
usage: python tools/bench_audience.py [--reps N] [--passes N] [--users B [B ...]] [--items Q [Q ...]] [--out file.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_recommend import _batch, _model, _time  # noqa: E402
from carca_replication_amd import catalogue  # noqa: E402
from carca_replication_amd.catalogue import AudienceTopK, CandidateSet  # noqa: E402

C2 = dict(n_items=12102, n_attrs=4096, d=90, g=450, H=3)
USERS = (128, 4096)
ITEMS = (1, 64, 1024, 0)  # 0: the whole catalogue
WALK = 64


def run(users, items, reps, passes):
    n_items, d, H = C2["n_items"], C2["d"], C2["H"]
    n_ctx, L, k = 6, 50, 10
    model = _model(n_items, C2["n_attrs"], n_ctx, d, C2["g"], H, 2, 0.01)
    gen = torch.Generator().manual_seed(7)
    rows = []
    with torch.no_grad():
        for B in users:
            p_x, p_c, ctx, _ = _batch(B, L, n_items, n_ctx)
            prof = (p_x, None, p_c)
            for Q in items:
                Q = Q or n_items - 1
                ids = (torch.randperm(n_items - 1, generator=gen)[:Q] + 1).cuda()
                S = CandidateSet(ids, n_items)
                lst = S.ids.view(1, Q).expand(B, Q).contiguous()
                excluded = torch.zeros(B, Q, dtype=torch.bool, device="cuda")
                for slot in range(L):
                    excluded |= p_x[:, slot:slot + 1] == S.ids.view(1, Q)
                kk = min(k, B)

                def aten():
                    s = model.score_items(prof, ctx, lst).masked_fill_(excluded, float("-inf"))
                    return torch.topk(s, kk, dim=0)

                calls = dict(users=lambda: model.recommend_users(prof, ctx, S, k=k),
                             scoring=lambda: model.recommend(prof, ctx, k=1, candidates=S),
                             aten=aten,
                             side=lambda: catalogue.carca_model_side(model, prof, ctx, "bench"))
                r = max(2, reps // 8) if B * Q > 1 << 22 else reps
                best = {key: float("inf") for key in calls}
                for _ in range(passes):  # interleaved: a drift of the machine hits them alike
                    for key, fn in calls.items():
                        best[key] = min(best[key], _time(fn, r))
                got, want = calls["users"]()[0][:, :kk], aten().values.t()
                same = torch.equal(torch.where(torch.isinf(want), torch.zeros_like(want), want), got)
                row = dict(config="C2", n_items=n_items, d=d, H=H, B=B, Q=Q, k=k, reps=r, passes=passes,
                           ms_recommend_users=round(best["users"], 4), ms_scoring_launches=round(best["scoring"], 4),
                           ms_aten_composition=round(best["aten"], 4), ms_model_side=round(best["side"], 4),
                           ms_scoring_minus_model_side=round(best["scoring"] - best["side"], 4),
                           ms_merge_minus_select=round(best["users"] - best["scoring"], 4),
                           users_over_scoring=round(best["users"] / best["scoring"], 3),
                           aten_over_users=round(best["aten"] / best["users"], 3), scores_equal_aten=bool(same),
                           scratch_bytes_logits=B * Q * 4, state_bytes=Q * k * 8)
                if B == users[0]:
                    state = AudienceTopK(S, k, n_items)

                    def walk():
                        state.reset()
                        for _ in range(WALK):
                            state.update(model, prof, ctx)

                    row["ms_per_update_of_64"] = round(_time(walk, max(1, r // 8)) / WALK, 4)
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--users", type=int, nargs="+", default=list(USERS))
    ap.add_argument("--items", type=int, nargs="+", default=list(ITEMS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = run(tuple(a.users), tuple(a.items), a.reps, a.passes)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
