"""sha256 of the row product's raw output bytes through the one-block-per-CU kernel (csrc/gemm.hip: gemm_rows_cu_kernel,
a client of cu_tile) on seeded inputs, one line per case: the kernel that ran (ops.gemm_rows_log) and each output tensor's
hash.  cu_tile multiplies the same products in the same order whichever kernel calls it, so a change that only moves its
code must leave every line as it was: run the script once per build (a fresh process each, --package-root naming the
tree whose package is imported) on the same machine and compare the listings line for line.
Routes (tests/test_hip_gemm_routes.py): key 0 = 15 and key 0 = 3 at C2 (19,328 rows: gemm_rows_cu_kernel<0,3>), key 0 = 7
at 26,880 rows (gemm_rows_cu_kernel<0,4> where rows are not masked), each with K0 in {4096, 4097, 4099, 4127} (K tails
0 / 1 / 3 / 31), K1 in {0, 6} and mask_rows on and off.
usage: python tools/gemm_tile_bits.py [--package-root DIR] [--out listing.txt]"""
import argparse
import hashlib
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.package_root))

import torch  # noqa: E402

from carca_replication_amd import ops  # noqa: E402

ROUTES = [("c2_k15", 15, [6400, 12928]), ("tiled_k7", 7, [8960, 17920]), ("c2_k3", 3, [6400, 12928])]
N = 450
lines = []
for name, key0, rows in ROUTES:
    for K0 in (4096, 4097, 4099, 4127):
        for K1 in (0, 6):
            torch.manual_seed(1000 * K0 + K1)
            w = (torch.rand(N, K0 + K1, device="cuda") - 0.5) * 0.03
            bias = torch.rand(N, device="cuda") - 0.5
            base = [dict(a0=torch.rand(r, K0, device="cuda"), a1=torch.rand(r, max(K1, 1), device="cuda"),
                         ids=torch.randint(0, 3, (r,), device="cuda", dtype=torch.int32)) for r in rows]
            for mask in (True, False):
                segs = [dict(a0=b["a0"], ids=b["ids"], **({"a1": b["a1"]} if K1 else {})) for b in base]
                kw = dict(bias=bias, mask_rows=mask)
                if K1:
                    kw.update(bt1=w[:, K0:], K1=K1)
                ops.set_tuning(0, key0)
                ops.gemm_rows_log(True)
                try:
                    outs = ops.gemm_rows(segs, w[:, :K0], N, K0, (N + 3) // 4 * 4, **kw)
                    torch.cuda.synchronize()
                    log = ops.gemm_rows_log()
                finally:
                    ops.gemm_rows_log(False)
                    ops.set_tuning(0, 0)
                hs = " ".join(hashlib.sha256(o[:, :N].contiguous().cpu().numpy().tobytes()).hexdigest()[:24] for o in outs)
                lines.append(f"{name} K0={K0} K1={K1} mask={int(mask)} {log} {hs}")
text = "\n".join(lines) + "\n"
sys.stdout.write(text)
if args.out:
    with open(args.out, "w") as f:
        f.write(text)
