"""CARCA.retrieve (the deep top-k) timed with device events, ms per batch of users, at
  C2       12,102 items, n_attrs 4096, d 90, g 450, H 3, 2 blocks, B = 128 users,
  C4       dimensions d 128, g 640, H 4, 1,000,001 items (AllEmbedding over 64 attributes), B = 128,
  C4-4096  the same model, B = 4096 (a 16 GiB logit scratch),
for k = 128, 1000 and 4096, with the shipped number of parts per user and with one part (ops.TUNE_RETRIEVE_PARTS), and
k = 1000 with every number of parts in --parts; in the same process and in interleaved passes with
  recommend(k=128)   the like-for-like call: the same sweep and exclusion, rc_select_kernel's eight passes at most;
  ATen               what a caller writes without retrieve: score_items over arange(1, n_items) for every user, then
                     torch.topk(k) (k = 1000, 4096), in chunks of users whose B * N fits score_items' int.
Each call is timed --passes times over --reps repetitions; a row holds the smallest, the median and the largest pass.
Tables cached, exclude="profile".  Models and batches are bench_recommend.py's.

--trace K S runs retrieve(k=K) alone with S parts forced (0 = shipped), for a rocprofv3 --kernel-trace --stats run of
its own; --kernel-stats FILE [FILE ...] turns such runs' kernel_stats.csv into the per-launch split (sweep, exclusion,
stage 1, stage 2) and prints it.
usage: python tools/bench_retrieve.py [--shape C2 C4 C4-4096] [--reps N] [--passes N] [--parts S [S ...]] [--out file.json]
       python tools/bench_retrieve.py --shape C4 --trace 1000 0
       python tools/bench_retrieve.py --kernel-stats a_kernel_stats.csv"""
import argparse
import csv
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_recommend import _batch, _model, _time  # noqa: E402
from carca_replication_amd import ops  # noqa: E402

SHAPES = {
    "C2": dict(n_items=12102, n_attrs=4096, d=90, g=450, H=3, B=128),
    "C4": dict(n_items=1000001, n_attrs=64, d=128, g=640, H=4, B=128),
    "C4-4096": dict(n_items=1000001, n_attrs=64, d=128, g=640, H=4, B=4096),
}
KS = (128, 1000, 4096)
LAUNCHES = (("sweep", "sweep_kernel"), ("sweep", "sweep_long_kernel"), ("exclusion", "rc_exclude_kernel"),
            ("stage1", "ds_part_kernel"), ("stage2", "ds_merge_kernel"))


def shipped_parts(B, n_slots, k):
    """What csrc/deep_select.h's ds_parts picks with tuning key 24 at 0 (mirrored here to label the rows)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    S = 1
    if n_slots > 32768 and B < 2 * cus:
        S = min((n_slots + 16383) // 16384, (8 * cus + B - 1) // B)
    S = max(1, min(S, 64, n_slots))
    while S > 1 and B * S * min(k, (n_slots + S - 1) // S) * 8 > 1 << 30:
        S -= 1
    return S


class forced_parts:
    def __init__(self, S):
        self.S = S

    def __enter__(self):
        ops.set_tuning(ops.TUNE_RETRIEVE_PARTS, self.S)

    def __exit__(self, *exc):
        ops.set_tuning(ops.TUNE_RETRIEVE_PARTS, 0)


def _setup(name):
    cfg = SHAPES[name]
    n_ctx, L = 6, 50
    model = _model(cfg["n_items"], cfg["n_attrs"], n_ctx, cfg["d"], cfg["g"], cfg["H"], 2,
                   0.01 if cfg["n_attrs"] > 64 else 0.1)
    p_x, p_c, ctx, _ = _batch(cfg["B"], L, cfg["n_items"], n_ctx)
    return cfg, model, (p_x, None, p_c), ctx


def run(name, reps, passes, parts):
    cfg, model, prof, ctx = _setup(name)
    n_items, B = cfg["n_items"], cfg["B"]
    users = max(1, min(B, 1024, (2 ** 31 - 1) // n_items))  # score_items takes B * N < 2^31
    # every user's list of all items, built once outside the timed calls (int32, dense: score_items reads it as it is)
    every = torch.arange(1, n_items, device="cuda", dtype=torch.int32).expand(users, -1).contiguous()

    def retrieve(k, S):
        def call():
            with forced_parts(S):
                return model.retrieve(prof, ctx, k=k)
        return call

    def aten(k):
        def call():
            out = []
            for lo in range(0, B, users):
                sub = tuple(None if t is None else t[lo:lo + users] for t in prof)
                sc = model.score_items(sub, ctx[lo:lo + users], every[:sub[0].shape[0]])
                s, i = torch.topk(sc, k, dim=1)
                out.append((s, i + 1))
            return out
        return call

    calls = {"recommend_k128": lambda: model.recommend(prof, ctx, k=128)}
    for k in KS:
        calls[f"retrieve_k{k}_shipped"] = retrieve(k, 0)
        calls[f"retrieve_k{k}_parts1"] = retrieve(k, 1)
    for S in parts:
        if S != 1:
            calls[f"retrieve_k1000_parts{S}"] = retrieve(1000, S)
    for k in (1000, 4096):
        calls[f"aten_score_items_topk_k{k}"] = aten(k)
    times = {key: [] for key in calls}
    with torch.no_grad():
        for _ in range(passes):  # interleaved: a drift of the machine hits every call alike
            for key, fn in calls.items():
                times[key].append(_time(fn, reps))
        same = all(torch.equal(a, b) for k in KS for a, b in zip(retrieve(k, 0)(), retrieve(k, 1)()))
        r128, rec = retrieve(128, 0)(), calls["recommend_k128"]()
        same128 = torch.equal(r128[0], rec[0]) and torch.equal(r128[1], rec[1])
    row = dict(shape=name, n_items=n_items, d=cfg["d"], H=cfg["H"], B=B, reps=reps, passes=passes,
               parts_shipped={f"k{k}": shipped_parts(B, n_items, k) for k in KS}, aten_users_per_chunk=users,
               shipped_equals_one_part=bool(same), retrieve128_equals_recommend128=bool(same128),
               scratch_bytes_logits=B * n_items * 4, ms={})
    for key, ts in times.items():
        row["ms"][key] = dict(min=round(min(ts), 4), median=round(statistics.median(ts), 4), max=round(max(ts), 4))
    return row


def trace(name, k, S, reps):
    cfg, model, prof, ctx = _setup(name)
    with torch.no_grad(), forced_parts(S):
        ms = _time(lambda: model.retrieve(prof, ctx, k=k), reps)
    print(json.dumps(dict(shape=name, k=k, parts_forced=S, parts=S or shipped_parts(cfg["B"], cfg["n_items"], k),
                          reps=reps, ms_under_the_profiler=round(ms, 4))), flush=True)


def kernel_split(path):
    """A rocprofv3 kernel_stats.csv of a --trace run -> {launch: mean microseconds per call} over the four launches."""
    out = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            for label, needle in LAUNCHES:
                if needle + "<" in r["Name"] or needle + "(" in r["Name"] or r["Name"].startswith(needle):
                    calls = int(r["Calls"])
                    tot, n = out.get(label, (0.0, 0))
                    out[label] = (tot + float(r["TotalDurationNs"]), n + calls)
                    break
    return {label: round(tot / n / 1e3, 2) for label, (tot, n) in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), nargs="+", default=["C2", "C4", "C4-4096"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--parts", type=int, nargs="+", default=[1, 2, 4, 8, 16, 64])
    ap.add_argument("--trace", type=int, nargs=2, metavar=("K", "S"), default=None)
    ap.add_argument("--kernel-stats", nargs="+", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        for path in a.kernel_stats:
            print(json.dumps(dict(file=os.path.basename(path), us_per_launch=kernel_split(path))), flush=True)
        return
    if a.trace:
        for name in a.shape:
            trace(name, a.trace[0], a.trace[1], a.reps)
        return
    rows = []
    for name in a.shape:
        rows.append(run(name, a.reps, a.passes, tuple(a.parts)))
        print(json.dumps(rows[-1]), flush=True)
        if a.out:  # (written after every shape: a later shape that runs out of time loses nothing)
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
