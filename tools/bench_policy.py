"""CARCA.log_prob_items (a sampling policy's log-probabilities for listed items) timed with device
events, ms per batch of users, at bench_sampled.py's shapes
  C2   12,102 items, n_attrs 4096, d 90, g 450, H 3, 2 blocks, B = 128 users,
  C4   dimensions d 128, g 640, H 4, 1,000,001 items (AllEmbedding over 64 attributes), B = 128,
for lists of N = 10 and 1000 ids per user; in the same process and in interleaved passes with
  recommend_sampled(k = N)   the call whose log it evaluates: the same sweep and exclusion, then the perturb pass over a
                             second buffer, the selection and its finishing launch, where log_prob_items runs the reduce
                             pass and its own finishing launch;
  retrieve(k = N)            the same sweep and exclusion, then the selection.
Each call is timed --passes times over --reps repetitions; a row holds the smallest, the median and the largest pass.
In the same process the reduce pass is timed alone (carca_policy_reduce over a [B, n_items] fp32 buffer of random logits
with id 0 excluded) against carca_sampled_perturb over the SAME buffer, interleaved, and set against the bytes it moves:
one read of that buffer (the perturb pass: one read and one write).
Two orderings follow from the code and are recorded as booleans: the reduce pass does strictly less than the perturb
pass, and log_prob_items leaves out the selection and the second buffer that recommend_sampled(k = N) pays for.
Tables cached, exclude="profile", temperature 1, a fixed seed.  Models and batches are bench_recommend.py's.
usage: python tools/bench_policy.py [--shape C2 C4] [--reps N] [--passes N] [--out profiles/r35_policy.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctypes as C  # noqa: E402

from bench_recommend import _time  # noqa: E402
from bench_sampled import SEED, SHAPES, _setup  # noqa: E402
from carca_replication_amd import _lib, ops  # noqa: E402

NS = (10, 1000)


def _stats(ts):
    return dict(min=round(min(ts), 4), median=round(statistics.median(ts), 4), max=round(max(ts), 4))


def passes_alone(B, n_items, reps, passes):
    """The reduce launch and the perturb launch by themselves over one buffer, interleaved: -> dict(reduce, perturb: ms
    min / median / max over the passes and tb_per_s at the median)."""
    g = torch.Generator(device="cuda").manual_seed(SEED)
    logits = torch.randn(B, n_items, device="cuda", generator=g) * 3
    logits.view(torch.int32)[:, 0] = -1  # the exclusion sentinel's bits over id 0
    pert = torch.empty_like(logits)
    n_chunks = (n_items + 1023) // 1024
    part2, part3 = torch.empty(B, n_chunks, 2, device="cuda"), torch.empty(B, n_chunks, 3, device="cuda")
    X = _lib.Sampling(temperature=1.0, seed=SEED)
    lib = _lib.load()

    def reduce():
        _lib.check(lib.carca_policy_reduce(logits.data_ptr(), part3.data_ptr(), B, n_items, 1.0, ops._stream()), "policy_reduce")

    def perturb():
        _lib.check(lib.carca_sampled_perturb(logits.data_ptr(), pert.data_ptr(), part2.data_ptr(), B, n_items, C.byref(X),
                                             ops._stream()), "sampled_perturb")
    ts = {"reduce": [], "perturb": []}
    for _ in range(passes):
        ts["reduce"].append(_time(reduce, 4 * reps))
        ts["perturb"].append(_time(perturb, 4 * reps))
    same = torch.equal(part3[:, :, :2].contiguous().view(torch.int32), part2.view(torch.int32))
    out = {"partials_bit_equal": bool(same)}
    for key, nbytes in (("reduce", 4 * B * n_items), ("perturb", 2 * 4 * B * n_items)):
        out[key] = dict(_stats(ts[key]), bytes_moved=nbytes,
                        tb_per_s=round(nbytes / (statistics.median(ts[key]) * 1e-3) / 1e12, 3))
    out["reduce_not_slower_than_perturb"] = out["reduce"]["median"] <= out["perturb"]["median"]
    return out


def run(name, reps, passes):
    cfg, model, prof, ctx = _setup(name)
    n_items, B = cfg["n_items"], cfg["B"]
    calls, items = {}, {}
    with torch.no_grad():
        for N in NS:
            _, items[N], logged = model.recommend_sampled(prof, ctx, k=N, temperature=1.0, seed=SEED)
            calls[f"log_prob_items_N{N}"] = lambda N=N: model.log_prob_items(prof, ctx, items[N], temperature=1.0)
            calls[f"recommend_sampled_k{N}"] = lambda N=N: model.recommend_sampled(prof, ctx, k=N, temperature=1.0, seed=SEED)
            calls[f"retrieve_k{N}"] = lambda N=N: model.retrieve(prof, ctx, k=N)
        same = torch.equal(model.log_prob_items(prof, ctx, items[NS[-1]], temperature=1.0)[0], logged)
        entropy = model.log_prob_items(prof, ctx, items[10], temperature=1.0)[2]
        times = {key: [] for key in calls}
        for _ in range(passes):  # interleaved: a drift of the machine hits every call alike
            for key, fn in calls.items():
                times[key].append(_time(fn, reps))
    n_chunks = (n_items + 1023) // 1024
    row = dict(shape=name, n_items=n_items, d=cfg["d"], H=cfg["H"], B=B, reps=reps, passes=passes, temperature=1.0,
               bits_of_recommend_sampled=bool(same), mean_effective_items=round(float(torch.exp(entropy.double()).mean()), 1),
               scratch_bytes_logits=B * n_items * 4, scratch_bytes_partials=B * n_chunks * 12,
               scratch_bytes_recommend_sampled_extra=B * n_items * 4 + B * n_chunks * 8,
               ms={key: _stats(ts) for key, ts in times.items()}, not_slower_than_recommend_sampled={})
    for N in NS:
        row["not_slower_than_recommend_sampled"][f"N{N}"] = \
            row["ms"][f"log_prob_items_N{N}"]["median"] <= row["ms"][f"recommend_sampled_k{N}"]["median"]
    del model
    torch.cuda.empty_cache()
    row["passes_alone"] = passes_alone(B, n_items, reps, passes)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), nargs="+", default=["C2", "C4"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for name in a.shape:
        rows.append(run(name, a.reps, a.passes))
        print(json.dumps(rows[-1]), flush=True)
        if a.out:  # (written after every shape: a later shape that runs out of time loses nothing)
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
