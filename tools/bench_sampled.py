"""CARCA.recommend_sampled (Gumbel top-k sampling with logged propensities) timed with device
events, ms per batch of users, at
  C2   12,102 items, n_attrs 4096, d 90, g 450, H 3, 2 blocks, B = 128 users,
  C4   dimensions d 128, g 640, H 4, 1,000,001 items (AllEmbedding over 64 attributes), B = 128,
for k = 10, 128 and 1000; in the same process and in interleaved passes with
  recommend(k)   (k <= 128) and
  retrieve(k)    the like-for-like calls: the same sweep, exclusion and -- retrieve -- the same selection, so
                 recommend_sampled(k) - retrieve(k) is the perturb pass plus the finishing launch.
Each call is timed --passes times over --reps repetitions; a row holds the smallest, the median and the largest pass.
In the same process the perturb pass is timed alone with device events (carca_sampled_perturb over a [B, n_items] fp32
buffer of random logits with id 0 excluded) and set against the bytes it moves, one read and one write of that buffer.
Tables cached, exclude="profile", temperature 1, a fixed seed.  Models and batches are bench_recommend.py's.

--trace K runs recommend_sampled(k=K) alone, for a rocprofv3 --kernel-trace --stats run of its own;
--kernel-stats FILE [FILE ...] turns such runs' kernel_stats.csv into the per-launch split (sweep, exclusion, perturb,
stage 1, stage 2, finish) and prints it; with --bytes N also the perturb launch's achieved bytes per second.
usage: python tools/bench_sampled.py [--shape C2 C4] [--reps N] [--passes N] [--out profiles/r34_sampled.json]
       python tools/bench_sampled.py --shape C4 --trace 1000
       python tools/bench_sampled.py --kernel-stats a_kernel_stats.csv --bytes 1024001024"""
import argparse
import csv
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctypes as C  # noqa: E402

from bench_recommend import _batch, _model, _time  # noqa: E402
from carca_replication_amd import _lib, ops  # noqa: E402

SHAPES = {
    "C2": dict(n_items=12102, n_attrs=4096, d=90, g=450, H=3, B=128),
    "C4": dict(n_items=1000001, n_attrs=64, d=128, g=640, H=4, B=128),
}
KS = (10, 128, 1000)
SEED = 34
LAUNCHES = (("sweep", "sweep_kernel"), ("sweep", "sweep_long_kernel"), ("exclusion", "rc_exclude_kernel"),
            ("perturb", "sp_perturb_kernel"), ("stage1", "ds_part_kernel"), ("stage2", "ds_merge_kernel"),
            ("finish", "sp_finish_kernel"))


def _setup(name):
    cfg = SHAPES[name]
    n_ctx, L = 6, 50
    model = _model(cfg["n_items"], cfg["n_attrs"], n_ctx, cfg["d"], cfg["g"], cfg["H"], 2,
                   0.01 if cfg["n_attrs"] > 64 else 0.1)
    p_x, p_c, ctx, _ = _batch(cfg["B"], L, cfg["n_items"], n_ctx)
    return cfg, model, (p_x, None, p_c), ctx


def perturb_bytes(B, n_items):
    return 2 * 4 * B * n_items


def perturb_alone(B, n_items, reps, passes):
    """The perturb launch by itself: -> dict(ms min / median / max over the passes, tb_per_s at the median)."""
    g = torch.Generator(device="cuda").manual_seed(SEED)
    logits = torch.randn(B, n_items, device="cuda", generator=g) * 3
    logits.view(torch.int32)[:, 0] = -1  # the exclusion sentinel's bits over id 0
    pert = torch.empty_like(logits)
    part = torch.empty(B, (n_items + 1023) // 1024, 2, device="cuda")
    X = _lib.Sampling(temperature=1.0, seed=SEED)
    lib = _lib.load()

    def call():
        _lib.check(lib.carca_sampled_perturb(logits.data_ptr(), pert.data_ptr(), part.data_ptr(), B, n_items, C.byref(X),
                                             ops._stream()), "sampled_perturb")
    ts = [_time(call, 4 * reps) for _ in range(passes)]
    med = statistics.median(ts)
    return dict(min=round(min(ts), 4), median=round(med, 4), max=round(max(ts), 4),
                tb_per_s=round(perturb_bytes(B, n_items) / (med * 1e-3) / 1e12, 3))


def run(name, reps, passes):
    cfg, model, prof, ctx = _setup(name)
    n_items, B = cfg["n_items"], cfg["B"]
    calls = {}
    for k in KS:
        calls[f"recommend_sampled_k{k}"] = lambda k=k: model.recommend_sampled(prof, ctx, k=k, temperature=1.0, seed=SEED)
        calls[f"retrieve_k{k}"] = lambda k=k: model.retrieve(prof, ctx, k=k)
        if k <= 128:
            calls[f"recommend_k{k}"] = lambda k=k: model.recommend(prof, ctx, k=k)
    times = {key: [] for key in calls}
    with torch.no_grad():
        for _ in range(passes):  # interleaved: a drift of the machine hits every call alike
            for key, fn in calls.items():
                times[key].append(_time(fn, reps))
        a, b = calls["recommend_sampled_k1000"](), calls["recommend_sampled_k1000"]()
        same = all(torch.equal(x, y) for x, y in zip(a, b))
        mass = float(torch.exp(a[2].double()).sum(1).max())
    row = dict(shape=name, n_items=n_items, d=cfg["d"], H=cfg["H"], B=B, reps=reps, passes=passes, temperature=1.0,
               same_seed_same_bits=bool(same), largest_drawn_mass_k1000=round(mass, 6),
               scratch_bytes_logits=B * n_items * 4, scratch_bytes_perturbed=B * n_items * 4,
               perturb_bytes_moved=perturb_bytes(B, n_items), ms={}, sampled_minus_retrieve_ms={})
    for key, ts in times.items():
        row["ms"][key] = dict(min=round(min(ts), 4), median=round(statistics.median(ts), 4), max=round(max(ts), 4))
    for k in KS:
        row["sampled_minus_retrieve_ms"][f"k{k}"] = round(
            row["ms"][f"recommend_sampled_k{k}"]["median"] - row["ms"][f"retrieve_k{k}"]["median"], 4)
    del model
    torch.cuda.empty_cache()
    row["perturb_alone"] = perturb_alone(B, n_items, reps, passes)
    return row


def trace(name, k, reps):
    cfg, model, prof, ctx = _setup(name)
    with torch.no_grad():
        ms = _time(lambda: model.recommend_sampled(prof, ctx, k=k, temperature=1.0, seed=SEED), reps)
    print(json.dumps(dict(shape=name, k=k, reps=reps, perturb_bytes_moved=perturb_bytes(cfg["B"], cfg["n_items"]),
                          ms_under_the_profiler=round(ms, 4))), flush=True)


def kernel_split(path):
    """A rocprofv3 kernel_stats.csv of a --trace run -> {launch: mean microseconds per call} over the launches."""
    out = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            for label, needle in LAUNCHES:
                if needle + "<" in r["Name"] or needle + "(" in r["Name"] or r["Name"].startswith(needle):
                    tot, n = out.get(label, (0.0, 0))
                    out[label] = (tot + float(r["TotalDurationNs"]), n + int(r["Calls"]))
                    break
    return {label: round(tot / n / 1e3, 2) for label, (tot, n) in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), nargs="+", default=["C2", "C4"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--trace", type=int, metavar="K", default=None)
    ap.add_argument("--kernel-stats", nargs="+", default=None)
    ap.add_argument("--bytes", type=int, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        for path in a.kernel_stats:
            split = kernel_split(path)
            row = dict(file=os.path.basename(path), us_per_launch=split)
            if a.bytes and split.get("perturb"):
                row["perturb_tb_per_s"] = round(a.bytes / (split["perturb"] * 1e-6) / 1e12, 3)
            print(json.dumps(row), flush=True)
        return
    if a.trace:
        for name in a.shape:
            trace(name, a.trace, a.reps)
        return
    rows = []
    for name in a.shape:
        rows.append(run(name, a.reps, a.passes))
        print(json.dumps(rows[-1]), flush=True)
        if a.out:  # (written after every shape: a later shape that runs out of time loses nothing)
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
