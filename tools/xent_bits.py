"""Bit fingerprints of the tile-kernel losses (csrc/catalogue_xent.hip, csrc/sampled_xent.hip, csrc/sampled_bce.hip and
csrc/policy_xent.hip over csrc/xent_tile.h, csrc/xent_stage.h and csrc/xent_direct.h; DESIGN.md sections 13, 14, 16 and
29): for a fixed list of seeded cases, one sha256 per output tensor of ops.catalogue_xent_fwd / _bwd, ops.sampled_xent_fwd
/ _bwd, ops.sampled_bce_fwd / _bwd and ops.policy_xent_fwd / _bwd, over the bytes of the whole strided buffer (so the zero
columns past d count).  Every sum in these kernels has one fixed order,
so a change that only moves code must leave every line as it was: run the script once per build (a fresh process each,
--package-root naming the tree whose package is imported) on the same machine and compare the listings line for line.
The hashes depend on the CU count through the split plan (first line).  The cases: d in {64, 90, 128, 192, 256} with row strides past d; padding rows (pos 0, pos >=
n_items, negative); R = 1; one and several row splits, several class splits with a short last one; sample ids that are
invalid, repeated, or equal to a row's positive; a batch without a valid row; the two benchmark shapes.  gBCE runs the
sampled shapes twice, with the context rows C and without, after the softmax losses' lines (which keep their seeds).
The policy lines come last, over the catalogue's shapes at temperature 0.5 with row gradients c and h of mixed sign:
without lists and entropy (policy/), with the entropy (policy_ent/), with lists of 7 ids holding a duplicate, a 0, a
negative id, an id past the end and, on every fifth row, the row's own item (policy_e7/), with lists of 70 (policy_e70/),
and with every row's own item in its list, so that no row is valid (policy_none/); the list cases compute the entropy.
usage: python tools/xent_bits.py [--package-root DIR] [--out listing.txt]"""
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

# (name, R, classes (n_items, or K), d, row stride, a valid row exists)
SHAPES = [
    ("d64", 300, 1000, 64, 72, True),       # (stride past the 16-column blocks: the zero tail of the one-row-split path)
    ("d90", 300, 1000, 90, 92, True),       # (column masking inside the last 16-byte piece)
    ("d128", 300, 1000, 128, 128, True),
    ("d192", 200, 700, 192, 192, True),     # (NCB = 16)
    ("d256", 200, 700, 256, 260, True),
    ("r1", 1, 500, 90, 92, True),
    ("rows1", 200, 70000, 64, 64, True),    # (one row split: the tile writes the class gradient itself)
    ("novalid", 130, 400, 90, 92, False),
]
BENCH_CATALOGUE = ("bench", 6400, 12102, 90, 92, True)  # (11 item splits, the last short; 6 row splits at 256 CUs)
BENCH_SAMPLED = ("bench", 6400, 8192, 128, 128, True)


def _operand(g, rows, d, ld):
    x = torch.zeros(rows, ld)
    x[:, :d] = torch.randn(rows, d, generator=g) * 0.3
    return x.cuda()


def _pos(g, R, n_items, valid):
    pos = torch.randint(1, n_items, (R,), generator=g, dtype=torch.int32)
    if not valid:
        pos = torch.where(torch.arange(R) % 2 == 0, torch.zeros_like(pos), torch.full_like(pos, n_items))
    elif R > 4:  # padding rows: pos 0, pos >= n_items, negative
        kind = torch.randint(0, 10, (R,), generator=g)
        pos[kind == 0] = 0
        pos[kind == 1] = n_items
        pos[kind == 2] = n_items + 7
        pos[kind == 3] = -2
        pos[0] = 1
    return pos


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _sample_ids(g, K, n_items, pos):
    """K sample ids with invalid ones, duplicates and accidental hits of a row's positive (and of padding rows' ids)."""
    s_ids = torch.randint(1, n_items, (K,), generator=g, dtype=torch.int32)
    s_ids[3::17] = 0
    s_ids[5::29] = n_items
    s_ids[7::31] = -3
    s_ids[11::13] = s_ids[10::13][: s_ids[11::13].numel()]
    hits = torch.arange(2, K, 19)
    s_ids[hits] = pos[hits % pos.numel()]
    return s_ids


def catalogue_case(seed, name, R, n_items, d, ld, valid):
    g = torch.Generator().manual_seed(seed)
    P, T = _operand(g, R, d, ld), _operand(g, n_items, d, ld)
    pos = _pos(g, R, n_items, valid).cuda()
    grad = torch.tensor([0.37], device="cuda")
    loss, lse = ops.catalogue_xent_fwd(P, T, pos, d)
    dP, dT = ops.catalogue_xent_bwd(P, T, pos, lse, grad, d)
    return [(f"catalogue/{name}/{k}", _sha(v)) for k, v in (("loss", loss), ("lse", lse), ("dP", dP), ("dT", dT))]


def sampled_case(seed, name, R, K, d, ld, valid):
    g = torch.Generator().manual_seed(seed)
    n_items = 5000
    P, Tp, S = _operand(g, R, d, ld), _operand(g, R, d, ld), _operand(g, K, d, ld)
    pos = _pos(g, R, n_items, valid)
    s_ids = _sample_ids(g, K, n_items, pos)
    bp = -torch.rand(R, generator=g) * 3 - 1
    bs = -torch.rand(K, generator=g) * 3 - 1
    grad = torch.tensor([0.37], device="cuda")
    a = [x.cuda() for x in (bp, pos, S, s_ids, bs)]
    loss, lse, row_loss = ops.sampled_xent_fwd(P, Tp, a[0], a[1], a[2], a[3], a[4], n_items, d)
    dP, dTp, dS = ops.sampled_xent_bwd(P, Tp, a[0], a[1], a[2], a[3], a[4], n_items, lse, row_loss, grad, d)
    outs = (("loss", loss), ("lse", lse), ("row_loss", row_loss), ("dP", dP), ("dTp", dTp), ("dS", dS))
    return [(f"sampled/{name}/{k}", _sha(v)) for k, v in outs]


def bce_case(seed, with_c, name, R, K, d, ld, valid):
    g = torch.Generator().manual_seed(seed)
    n_items, beta = 5000, 0.8125  # (beta strictly inside (0, 1))
    P, Tp, S = _operand(g, R, d, ld), _operand(g, R, d, ld), _operand(g, K, d, ld)
    Cr = _operand(g, R, d, ld) if with_c else None
    pos = _pos(g, R, n_items, valid)
    s_ids = _sample_ids(g, K, n_items, pos).cuda()
    pos = pos.cuda()
    grad = torch.tensor([0.37], device="cuda")
    loss, saved, row_loss = ops.sampled_bce_fwd(P, Tp, Cr, pos, S, s_ids, n_items, beta, d)
    dP, dTp, dS, dC = ops.sampled_bce_bwd(P, Tp, Cr, pos, S, s_ids, n_items, beta, saved, grad, d)
    outs = (("loss", loss), ("saved", saved), ("row_loss", row_loss), ("dP", dP), ("dTp", dTp), ("dS", dS), ("dC", dC))
    tag = "bce_c" if with_c else "bce"
    return [(f"{tag}/{name}/{k}", _sha(v)) for k, v in outs if v is not None]


def policy_case(seed, kind, name, R, n_items, d, ld, valid):
    g = torch.Generator().manual_seed(seed)
    P, T = _operand(g, R, d, ld), _operand(g, n_items, d, ld)
    items = _pos(g, R, n_items, valid)
    c, h = torch.randn(R, generator=g).cuda(), (torch.randn(R, generator=g) * 0.01).cuda()
    E = dict(policy=0, policy_ent=0, policy_e7=7, policy_e70=70, policy_none=7)[kind]
    ent = kind != "policy"
    ex = None
    if E:
        excl = torch.randint(1, n_items, (R, E), generator=g, dtype=torch.int32)
        excl[:, 0], excl[:, 1], excl[:, 2], excl[:, 3] = 0, -5, n_items + 3, excl[:, 4]
        own = slice(None) if kind == "policy_none" else slice(2, None, 5)
        excl[own, 5] = items[own]
        ex = ops.policy_exclusion(excl.cuda(), R, n_items)
    items = items.cuda()
    log_prob, ok, H, lse = ops.policy_xent_fwd(P, T, items, d, 0.5, ex, ent)
    dP, dT = ops.policy_xent_bwd(P, T, items, d, 0.5, ex, lse, c, h if ent else None, H, ok)
    outs = (("log_prob", log_prob), ("valid", ok), ("entropy", H), ("lse", lse), ("dP", dP), ("dT", dT))
    return [(f"{kind}/{name}/{k}", _sha(v)) for k, v in outs if v is not None]


def main():
    assert torch.cuda.is_available(), "xent_bits.py needs a GPU"
    lines = [f"# cus={ops.num_cus()}"]
    for i, shape in enumerate(SHAPES + [BENCH_CATALOGUE]):
        lines += [f"{k} {h}" for k, h in catalogue_case(100 + i, *shape)]
    for i, shape in enumerate(SHAPES + [BENCH_SAMPLED]):
        lines += [f"{k} {h}" for k, h in sampled_case(200 + i, *shape)]
    for with_c in (True, False):
        for i, shape in enumerate(SHAPES + [BENCH_SAMPLED]):
            lines += [f"{k} {h}" for k, h in bce_case(300 + i, with_c, *shape)]
    for j, kind in enumerate(("policy", "policy_ent", "policy_e7", "policy_e70", "policy_none")):
        for i, shape in enumerate(SHAPES + [BENCH_CATALOGUE]):
            lines += [f"{k} {h}" for k, h in policy_case(400 + 20 * j + i, kind, *shape)]
    torch.cuda.synchronize()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
