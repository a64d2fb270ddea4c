"""optim.step() alone (carca_adam_step_ex, and carca_grad_norm when clipping), timed with device
events and on the host, in four configurations -- plain Adam, Adam with max_grad_norm, AdamW, AdamW with max_grad_norm --
at two sizes:
  C2  the parameter set of the C2 model (d 90, g 450, H 3, 2 blocks, 12,102 items: 3.09 M elements), every
      gradient dense;
  C4  the same at C4 dimensions (d 128, g 640, H 4, 1,000,001 items) with the 1 M x 128 item table on touched-row Adam:
      its gradient is non-zero in the rows of one C4 train batch (B 128: 6,400 profile + 12,800 target ids), announced with
      mark_rows before every step.  AdamW keeps the table in a group of its own without decay (decay would move
      untouched rows: mark_rows refuses it), everything else decays.
Gradients are synthetic (randn): the step's cost does not depend on their values.  The configurations alternate over
--rounds rounds in one process; every run is kept.  --package-root times another build of the package (an earlier
commit: only the configurations it has).
--reps is the steps per timed window at C2 (a step is ~0.03 ms: a short window times the clock); C4 takes a quarter.
usage: python tools/bench_optim.py [--reps N] [--rounds N] [--config all|C2|C4] [--package-root DIR] [--out file.json]"""
import argparse
import json
import os
import sys
import time

import torch

_root = argparse.ArgumentParser(add_help=False)
_root.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.abspath(_root.parse_known_args()[0].package_root))  # (the tree whose package is imported)
from carca_replication_amd import ops  # noqa: E402
from carca_replication_amd import optim as O  # noqa: E402
from tests.model_util import build_model  # noqa: E402

SIZES = dict(C2=dict(d=90, g=450, H=3, n_items=12102), C4=dict(d=128, g=640, H=4, n_items=1_000_001))
B, L, N_ATTRS, N_CTX = 128, 50, 4096, 6
CONFIGS = ("plain", "clipped", "adamw", "clipped_adamw")
MAX_NORM = 1.0  # (far below the synthetic gradients' norm: every step is clipped -- the cost is the same either way)


def _optimizer(config, params, table):
    clip = dict(max_grad_norm=MAX_NORM) if config.startswith("clipped") else {}
    if not config.endswith("adamw"):
        return O.Adam(params, lr=1e-4, betas=(0.9, 0.98), **clip)
    cls = getattr(O, "AdamW")
    if table is None:
        return cls(params, lr=1e-4, betas=(0.9, 0.98), weight_decay=0.01, **clip)
    rest = [p for p in params if p is not table]
    return cls([dict(params=[table], weight_decay=0.0), dict(params=rest)], lr=1e-4, betas=(0.9, 0.98), weight_decay=0.01, **clip)


def run(name, reps, rounds, configs):
    s = SIZES[name]
    torch.manual_seed(0)
    model = build_model(dict(d=s["d"], H=s["H"], n_blocks=2), s["n_items"], s["g"], N_CTX, N_ATTRS, L).cuda()
    params = list(model.parameters())
    gen = torch.Generator(device="cuda").manual_seed(1)
    table = model.embeds.items_embed.weight if name == "C4" else None
    ids = None
    for p in params:
        if p is table:
            ids = torch.randint(1, s["n_items"], (B * 3 * L,), generator=gen, device="cuda").to(torch.int32)
            p.grad = torch.zeros_like(p)
            p.grad[ids.long()] = torch.randn(ids.numel(), p.shape[1], generator=gen, device="cuda")
        else:
            p.grad = torch.randn(p.shape, generator=gen, device="cuda")
    out = dict(config=name, tensors=len(params), elements=sum(p.numel() for p in params), reps=reps,
               touched_rows=None if ids is None else int(torch.unique(ids).numel()))
    opts = {}
    for config in configs:
        opts[config] = opt = _optimizer(config, params, table)
        for _ in range(3):  # state, the cached tables and the code objects
            if table is not None:
                assert opt.mark_rows(table, ids)
            opt.step()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(rounds):
        for config in configs:
            opt = opts[config]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            for _ in range(reps):
                if table is not None:
                    opt.mark_rows(table, ids)
                opt.step()
            b.record()
            host = time.perf_counter() - t0  # (the launches are out; the device may still be running them)
            b.synchronize()
            out.setdefault(f"ms_{config}_runs", []).append(round(a.elapsed_time(b) / reps, 4))
            out.setdefault(f"us_host_{config}_runs", []).append(round(1e6 * host / reps, 1))
    for config in configs:
        out[f"ms_{config}"] = min(out[f"ms_{config}_runs"])
        out[f"us_host_{config}"] = min(out[f"us_host_{config}_runs"])
        norm = getattr(opts[config], "last_grad_norm", None)
        if norm is not None:
            out[f"grad_norm_{config}"] = round(float(norm), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--config", default="all", choices=("all", "C2", "C4"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--package-root", default=None, help="the tree whose package is imported (an earlier commit: the yardstick)")
    a = ap.parse_args()
    configs = CONFIGS if hasattr(O, "AdamW") else CONFIGS[:1]
    res = dict(device=torch.cuda.get_device_name(0), cus=ops.num_cus(), package=os.path.relpath(os.path.dirname(ops.__file__)),
               results=[])
    for name in ("C2", "C4"):
        if a.config in ("all", name):
            r = run(name, a.reps if name == "C2" else max(10, a.reps // 4), a.rounds, configs)
            res["results"].append(r)
            print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
