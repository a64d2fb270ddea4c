"""Phase anatomy of the SelfAttentionBlock kernels (eval: csrc/sa_eval.hip; TRAIN_KERNEL=1: csrc/sa_block.hip) from
in-kernel s_memtime stamps (diagnostic), per role of a workgroup.  Profiles are left-padded with lengths U{3..50} and the
launch carries the pads_uniform promise, as inside carca_forward (FULL=1: every slot real); at B <= #CUs / 2 a user has two
workgroups, and the idle second workgroup of a one-tile user takes tiles 0 / 1 of a four-tile user (LEND=0: tuning key
23 = 1, the fixed split)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from carca_replication_amd import _lib, ops  # noqa: E402
from tests.model_util import build_model  # noqa: E402

B, L, d, g, H = int(os.environ.get("B", "128")), 50, 90, 450, 3
torch.manual_seed(0)
model = build_model(dict(d=d, H=H, n_blocks=2), 500, g, 6, 64, L).eval().cuda()
dpi, _, _ = ops.padded_dims(d, H)
lens = torch.randint(3, L + 1, (B,))
if os.environ.get("FULL"):  # every slot real (the longest profile sets the launch's duration at B <= #CUs / 2)
    lens[:] = L
ids = ((torch.arange(L)[None, :] >= (L - lens)[:, None]).int() * 3).cuda()
x = torch.zeros(B, L, dpi, device="cuda")
x[..., :d] = torch.randn(B, L, d, device="cuda")
x = x * (ids != 0)[..., None]  # (leading pad rows equal -- zeros -- as inside carca_forward)
sw = model.encoder[0].weights_struct(x.device)
lib = _lib.load()
train = bool(os.environ.get("TRAIN_KERNEL"))
lend = os.environ.get("LEND", "1") != "0" and not train
if train:
    lib.carca_set_tuning(6, 1)
lib.carca_set_tuning(ops.TUNE_SA_LEND, 0 if lend else 1)
run = lambda: ops.sa_block_fwd(x, ids, sw, d, H, True, pads_uniform=not train)  # noqa: E731
for _ in range(5):
    run()
buf = torch.zeros(2 * B * 16, dtype=torch.int64, device="cuda")
lib.carca_set_debug_buffer(buf.data_ptr())
run()
torch.cuda.synchronize()
lib.carca_set_debug_buffer(None)
lent = ops.sa_eval_lent() if not train else 0
st = buf.view(2 * B, 16)[:, :8].cpu().double()

# the role of every workgroup, by the kernel's rule (sa_eval.hip): tiles of a user, donors and recipients in user order
nrows = lens + (lens < L).int()
LT = ((nrows + 15) // 16).tolist()
two = st[1::2, 0].max() > 0  # two workgroups per user
fixed = {4: ("{1,2}", "{0,3}"), 3: ("{2}", "{0,1}"), 2: ("{1}", "{0}"), 1: ("{0}", None)}
role = {}
donors = [u for u in range(B) if LT[u] == 1]
recips = [u for u in range(B) if LT[u] == 4]
if not two:
    role = {u: f"all {LT[u]} tiles" for u in range(B)}
else:
    for u in range(B):
        for part in (0, 1):
            if fixed[LT[u]][part]:
                role[2 * u + part] = f"LT={LT[u]} own {fixed[LT[u]][part]}"
    if lend:
        for r, u in enumerate(recips):
            mine = donors[2 * r:2 * r + 2]
            if mine:
                role[2 * u], role[2 * u + 1] = "LT=4 own {2} (lent)", "LT=4 own {3} (lent)"
            for k, du in enumerate(mine):
                role[2 * du + 1] = "donor {0,1}" if len(mine) == 1 else ("donor {1}" if k == 0 else "donor {0}")
names = ["A0 load x", "A1 LN1", "B K/V", "C1 attn", "C2 LN2", "C3 ffn1", "C4 ffn2"]
print(f"B = {B}, lending {'on' if lend else 'off'}: {len(recips)} four-tile users, {len(donors)} one-tile users, "
      f"sa_eval_lent() = {lent}; median cycles per phase (s_memtime ticks = shader cycles) per role, [count]")
groups = {}
for wg, name in role.items():
    if st[wg, 7] > 0:
        groups.setdefault(name, []).append(wg)
t0 = st[:, 0][st[:, 0] > 0].min()
print(f"  {'role':22s} {'n':>4s} " + " ".join(f"{n:>9s}" for n in names) + f" {'total':>8s} {'max':>8s} {'end@max':>8s}")
for name in sorted(groups):
    s = st[groups[name]]
    dt = s[:, 1:] - s[:, :-1]
    tot = s[:, 7] - s[:, 0]
    print(f"  {name:22s} {len(s):4d} " + " ".join(f"{dt[:, i].median():9.0f}" for i in range(7)) +
          f" {tot.median():8.0f} {tot.max():8.0f} {(s[:, 7] - t0).max():8.0f}")
done = st[st[:, 7] > 0]
print(f"  launch: first start to last end {done[:, 7].max() - t0:9.0f}   start skew "
      f"{(st[:, 0][st[:, 0] > 0].max() - t0):9.0f}   end skew {(done[:, 7].max() - done[:, 7].min()):9.0f}")
