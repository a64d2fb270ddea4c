"""Every row-product kernel (csrc/gemm.hip, gemm_stream.hip, gemm_split.hip: C = A B^T + epilogue) by name, against one
float64 statement of the operation (tests/gemm_ref.py), with every epilogue term its launcher admits and every term it
declines.

KERNELS below is the table: per kernel-name string of test_hip_gemm_routes.KERNEL_NAMES the smallest rows / N / K and
tuning keys that reach it, its block height, and the terms its launcher admits (read off the launchers' `return 1`
conditions).  Every launch runs with ops.gemm_rows_log on and asserts the kernel's name in the log (or, for a declined term,
its absence).  Outputs sit in sentinel-filled buffers: rows around every segment and columns >= ncols_out must be untouched.

Tolerance (the rule of test_hip_row_kernels.py, not derived from the code under test): on the same inputs, uniform in
[-1, 1),
    ref64 = the statement in float64,  ref32 = the statement in float32 by torch,  noise = max|ref32 - ref64|
and a kernel passes when  max|got - ref64| <= 8 noise + 4 eps32 max|ref64|;  the yardstick itself must satisfy
noise <= 16 eps32 max|ref64|.  Masked rows and pad columns are compared bit for bit with +0, a dropped gate with 0 of either
sign (v * 0 keeps v's sign, and v's sign is round-off where v is).  The split-precision kernels are no fp32 products: they
keep the bounds of test_hip_split_gemm.py and get the structural and the decline checks only.

Largest err / noise per kernel on one MI355X run (noise floored at eps32 max|ref64| / 2, the bound's second term; the same
figures on a second run: every kernel here sums in a fixed order):
    gemm_rows_kernel<128,32,32,4,1>  2.28    gemm_rows_kernel<128,32,32,4,0>  2.28    gemm_rows_group_kernel       1.44
    gemm_rows_kernel<128,96,32,1,1>  1.81    gemm_rows_kernel<128,96,32,1,0>  3.32
    gemm_rows_kernel<64,96,32,4,1>   2.23    gemm_rows_kernel<64,96,32,2,1>   2.23
    gemm_rows_cu_kernel<0,3>         3.32    gemm_rows_cu_kernel<0,4>         3.32    gemm_rows_cu_kernel<1>       3.32
    gemm_rows_sk_kernel<1>           7.85    gemm_rows_sk_kernel<2>           7.30    (K0 >= 2048, see below)
    gemm_rows_skc_kernel<0>          3.35    gemm_rows_skc_kernel<1>          3.84    gemm_rows_skc_kernel<2>      4.62
    gemm_rows_skc_kernel<2>+dedup    0.69    gemm_rows_n96_kernel             1.15    gemm_rows_n96s_kernel        1.31
    gemm_rows_cus_kernel<0>          3.41    gemm_rows_cus_kernel<1>          3.43    gemm_rows_cus_kernel<2>      2.90
    embed_fwd (q and e)              1.93    whatever ran for a declined term 8.93    (gemm_rows_cu_kernel<0,3> at K = 2054)
The largest err / (8 noise + 4 eps32 max|ref64|) was 0.94, on the one-row segment of a K = 2054 product: 448 elements
are a small sample of the yardstick's noise.
What the first run found:
  * In the kernels and launchers: none.  Every kernel was reached by its table entry, every admitted term came out
    right, every declined term went to another kernel.
  * In the yardstick: ATen's float32 product on the GPU is one chain over all of K, and at K = 2054 (what
    gemm_rows_sk_kernel needs) its noise measured 16.3 .. 19 eps32 max|ref64| -- past the 16 demanded above, where a CPU gives
    2.4.  The kernels' own error there is 16 .. 23, the same chain.  The statement (gemm_ref.product) therefore sums K in
    chains of 1024 terms, the longest power of two that keeps the demand (9.6 .. 11.5 at K = 2054); for K <= 1024 it is the
    plain product.  This only narrows the bound.
"""
import math

import pytest
import torch

from tests.gemm_ref import cast, exact_zero, gemm_rows_statement

gpu = pytest.mark.gpu
EPS32 = float(torch.finfo(torch.float32).eps)
SENTINEL = -12345.5
N_TAB = 211          # rows of the gather table and of add_table; ids are drawn below it
GATE_SLOPE = 0.3     # (not the default 0.01: a slope applied without its scale must show)

TERMS = ("bias", "alpha", "pos", "add", "add_table", "rowscale", "gate", "mask", "pad")
ALL = frozenset(TERMS)
PLAIN = frozenset({"bias", "alpha", "mask"})


def _r4(n):
    return (n + 3) // 4 * 4


def small(bm):
    return lambda ncols_out: 2 * bm + 3


def nonnarrow(ncols_out):
    """Rows past gemm_rows_choose's narrow bound: 128-row blocks x 96-column blocks >= 384."""
    ncb = (ncols_out + 95) // 96
    return -(-384 // ncb) * 128


def auto_cu(ncols_out):
    """Rows at which gemm_rows_choose takes the one-block-per-CU choice unforced: more than two rounds of 128 x 96 blocks
    (512 < blocks), one round of 384 x 96 ones."""
    ncb = (ncols_out + 95) // 96
    return (512 // ncb + 1) * 128


def K(name, tuning, bm, total, N, K0, K1, admits, *, ns, k0s, k1_ok=(0, 1, 3, 6, 8), forms=("dense", "view", "gather"),
      required=(), ns_declined=(), k0s_declined=(), gate_scale=1.0, aligned=False, split=False, log=None):
    return dict(name=name, log=log or name, tuning=tuning, bm=bm, total=total, N=N, K0=K0, K1=K1, admits=frozenset(admits),
                ns=ns, k0s=k0s, k1_ok=k1_ok, forms=forms, required=frozenset(required), ns_declined=ns_declined,
                k0s_declined=k0s_declined, gate_scale=gate_scale, aligned=aligned, split=split)


W32 = [(31, 31), (32, 32), (33, 36), (64, 64), (65, 68), (90, 96), (97, 97)]      # 32-column tiles
W96 = [(95, 95), (96, 96), (97, 100), (90, 96), (192, 192), (193, 196)]          # 96-column tiles, small
BIG = [(383, 383), (384, 384), (385, 388), (450, 452), (481, 481)]               # 96- and 128-column tiles past the narrow bound
NARROW = [(n, c) for n in (65, 90, 96) for c in sorted({n, 96})]
K32 = (64, 65, 67, 95)                                                          # K step 32: tails 0, 1, 3, 31

KERNELS = [
    # ---- gemm_rows_kernel<BM,BN,BK,PF,BUF>: gemm_rows_epilogue, every term
    K("gemm_rows_kernel<128,32,32,4,1>", {}, 128, small(128), 90, 64, 6, ALL, ns=W32, k0s=K32),
    K("gemm_rows_kernel<128,32,32,4,0>", {0: 4}, 128, small(128), 90, 64, 6, ALL, ns=W32, k0s=K32),
    K("gemm_rows_kernel<128,96,32,1,1>", {0: 1}, 128, small(128), 200, 64, 6, ALL, ns=W96, k0s=K32),
    K("gemm_rows_kernel<128,96,32,1,0>", {0: 4}, 128, nonnarrow, 450, 64, 6, ALL, ns=BIG, k0s=K32),
    K("gemm_rows_kernel<64,96,32,4,1>", {0: 9}, 64, small(64), 90, 64, 6, ALL, ns=W96, k0s=K32),
    K("gemm_rows_kernel<64,96,32,2,1>", {0: 10}, 64, small(64), 90, 64, 6, ALL, ns=W96, k0s=K32),
    # ---- gemm_rows_cu_kernel: 384 x 96 / 384 x 128 tiles, gemm_rows_epilogue (needs K0 >= 64 and rows past the narrow bound)
    K("gemm_rows_cu_kernel<0,3>", {0: 2}, 384, nonnarrow, 450, 64, 6, ALL, ns=BIG, k0s=K32),
    K("gemm_rows_cu_kernel<0,4>", {0: 7}, 384, nonnarrow, 450, 64, 6, ALL, ns=BIG[:4] + [(513, 513)], k0s=K32),
    K("gemm_rows_cu_kernel<1> (stamps)", {0: 3}, 384, nonnarrow, 450, 64, 6, ALL, ns=BIG[2:4], k0s=K32[:2],
      log="gemm_rows_cu_kernel<0,3>"),
    # ---- stream-K over every row: the plain epilogue, gate_scale = 0, K0 >= 2048, one round
    K("gemm_rows_sk_kernel<1>", {0: 23}, 384, auto_cu, 449, 2048, 6, PLAIN, ns=[(449, 449), (353, 353)],
      k0s=(2048, 2049, 2051, 2079), gate_scale=0.0, ns_declined=[(448, 448)], k0s_declined=(2016,)),
    K("gemm_rows_sk_kernel<2>", {0: 23}, 384, auto_cu, 450, 2048, 6, PLAIN, ns=[(450, 450), (354, 354)],
      k0s=(2048, 2049, 2051, 2079), gate_scale=0.0, ns_declined=[(451, 451)], k0s_declined=(2047,)),
    # ---- stream-K over the rows with id != 0: the plain epilogue, mask_rows required (key 19: fewer K steps admitted)
    K("gemm_rows_skc_kernel<0>", {0: 2, 19: 16}, 384, nonnarrow, 448, 512, 6, PLAIN, required=("mask",),
      ns=[(417, 417), (448, 448)], k0s=(512, 513, 515, 543), ns_declined=[(416, 416)]),
    K("gemm_rows_skc_kernel<1>", {0: 2, 19: 16}, 384, nonnarrow, 449, 512, 6, PLAIN, required=("mask",),
      ns=[(449, 449), (353, 353)], k0s=(512, 513, 515, 543)),
    K("gemm_rows_skc_kernel<2>", {0: 2, 19: 16}, 384, nonnarrow, 450, 512, 6, PLAIN, required=("mask",),
      ns=[(450, 450), (354, 354)], k0s=(512, 513, 515, 543), ns_declined=[(451, 451)]),
    # ---- the 80 x 96 kernel: its own epilogue with every term; one k-source, no gather; 16-byte operands unless add_table
    K("gemm_rows_n96_kernel", {0: 11}, 80, small(80), 90, 128, 0, ALL, ns=NARROW, k0s=(128, 132, 129, 131, 159), k1_ok=(0,),
      forms=("dense", "view"), aligned=True, ns_declined=[(64, 64), (97, 100)]),
    # ---- the persistent narrow-output kernel: alpha, bias, pos, add_table, mask, pad; dense rows of one k-source
    K("gemm_rows_n96s_kernel", {0: 27}, 160, small(160), 90, 256, 0, PLAIN | {"pos", "add_table", "pad"}, ns=NARROW,
      k0s=(256, 257, 259, 287), k1_ok=(0,), forms=("dense",), ns_declined=[(64, 64), (97, 100)], k0s_declined=(255,)),
    # ---- the short-K streaming kernel: the plain epilogue, K0 in whole pairs of K steps, K1 in 4 .. 8, dense rows
    K("gemm_rows_cus_kernel<0>", {0: 25}, 384, auto_cu, 448, 128, 6, PLAIN, ns=[(417, 417), (448, 448), (480, 480)],
      k0s=(128, 192), k1_ok=(6, 8), forms=("dense",), ns_declined=[(416, 416)], k0s_declined=(129, 160)),
    K("gemm_rows_cus_kernel<1>", {0: 25}, 384, auto_cu, 449, 128, 6, PLAIN, ns=[(449, 449)],
      k0s=(128, 192), k1_ok=(6, 8), forms=("dense",), k0s_declined=(131,)),
    K("gemm_rows_cus_kernel<2>", {0: 25}, 384, auto_cu, 450, 128, 6, PLAIN, ns=[(450, 450)],
      k0s=(128, 192), k1_ok=(6, 8), forms=("dense",), ns_declined=[(451, 451)], k0s_declined=(159,)),
    # ---- split precision (key 16, bit 4 admits it at a fixture size): structure and declines only
    # (pad columns: within the last 96-column block only)
    K("gemm_rows_split_dma_kernel<", {16: 17}, 384, lambda n: 1000, 450, 128, 6, PLAIN | {"pad"}, ns=[(450, 450), (450, 452)],
      k0s=(128,), aligned=True, split=True, ns_declined=[(480, 484)], k0s_declined=(130,)),
    K("gemm_rows_split_kernel<", {16: 17, 0: 21}, 384, lambda n: 1000, 450, 132, 6, PLAIN | {"pad"}, ns=[(450, 450), (449, 452)],
      k0s=(132, 128), split=True, ns_declined=[(480, 484)], k0s_declined=(130,)),
]
# reached through other entry points (their own tests below): the evaluation forward's dedup and the grouped launch
OTHER_ENTRIES = {"+dedup": "test_dedup_entry_against_float64", "grouped launch": "test_grouped_launch_against_float64"}
BY_NAME = {k["name"]: k for k in KERNELS}
IDS = [k["name"] for k in KERNELS]


# --------------------------------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------------------------------
def row_sets(k, ncols_out):
    """1 to 4 segments, lengths on both sides of the kernel's block height, one 1-row segment; the last segment alone
    carries the rows the route needs."""
    bm, big = k["bm"], k["total"](ncols_out)
    return [[bm + 1, 1, bm - 1, big], [bm, big], [bm - 1, bm + 1, big + 1], [big + bm]]


def make_ids(rows, gen):
    """Zeros in three places: scattered, as the segment's last rows, and as a whole 64-row chunk."""
    ids = torch.randint(1, N_TAB, (rows,), device="cuda", generator=gen).int()
    ids[torch.rand(rows, device="cuda", generator=gen) < 0.15] = 0
    if rows > 4:
        ids[-3:] = 0
    if rows >= 192:
        ids[64:128] = 0
    return ids


def make_case(rows, N, K0, K1=0, *, terms=(), ncols_out=None, form="dense", aligned=False, gate_scale=1.0,
              zero_drops=False, T=7, seed=0):
    """Operands, output buffers and keywords of one ops.gemm_rows call.  form: "dense" (a 2-D column slice with lda > K, at
    a 4-byte-aligned but not 16-byte-aligned address unless `aligned`), "view" ([B, T, K] with strided users) or "gather"
    (rows of a table by id).  a1 always has lda1 > K1."""
    terms = frozenset(terms)
    gen = torch.Generator(device="cuda").manual_seed(seed * 7919 + N * 31 + K0)
    u = lambda *s: torch.rand(*s, device="cuda", generator=gen) * 2 - 1  # noqa: E731
    if ncols_out is None:
        ncols_out = N + 5 if "pad" in terms else N
    ld = _r4(ncols_out) + 4
    if aligned:
        ldb, off, lda = _r4(K0 + K1) + 4, 0, _r4(K0) + 4
    else:
        ldb, off, lda = K0 + K1 + 1, 1, K0 + 5
    w = u(N, ldb)
    if form == "view":
        rows = [-(-r // T) * T for r in rows]
    total = sum(rows)
    buf = torch.full((total + 2 * (len(rows) + 1), ld), SENTINEL, device="cuda")
    segs, spans, r0 = [], [], 2
    for i, r in enumerate(rows):
        sg = dict(ids=make_ids(r, gen), T=T, out=buf[r0:r0 + r])
        spans.append((r0, r))
        r0 += r + 2
        if form == "view":
            sg["a0"] = u(r // T, T + 2, K0)[:, :T]
            if K1:
                sg["a1"] = u(r // T, T + 1, K1)[:, :T]
        else:
            n = N_TAB if form == "gather" else r
            sg["a0"] = u(n, lda)[:, off:off + K0]
            if form == "gather":
                sg["a0_gather"] = True
            if K1:
                sg["a1"] = u(r, K1 + 3)[:, :K1]
        if "pos" in terms:
            sg["add_pos"] = i % 2 == 0
        if "add" in terms:
            sg["add"] = u(r, N + 5)[:, :N]
        if "gate" in terms:
            gate = u(r, N + 2)
            gate[torch.rand(r, N + 2, device="cuda", generator=gen) < 0.25] = 0.0
            sg["gate"] = gate[:, :N]
        if "rowscale" in terms:
            sg["rowscale"] = u(r)
        segs.append(sg)
    kw = dict(bt0=w[:, :K0], N=N, K0=K0, K1=K1, ncols_out=ncols_out, mask_rows="mask" in terms, gate_slope=GATE_SLOPE,
              gate_scale=gate_scale, gate_zero_drops=zero_drops, alpha=0.37 if "alpha" in terms else 1.0)
    if K1:
        kw["bt1"] = w[:, K0:K0 + K1]
    if "bias" in terms:
        kw["bias"] = u(N)
    if "pos" in terms:
        kw["pos"] = u(T, N)
    if "rowscale" in terms:
        kw["colvec"] = u(N)
    if "add_table" in terms:
        kw["add_table"] = u(N_TAB, N + 6)[:, :N]
    return dict(segs=segs, kw=kw, buf=buf, spans=spans, ld=ld)


def launch(case, tuning):
    """ops.gemm_rows under the tuning keys, with the log on -> the log."""
    from carca_replication_amd import ops

    kw = dict(case["kw"])
    for key, value in tuning.items():
        ops.set_tuning(key, value)
    try:
        ops.gemm_rows_log(True)
        ops.gemm_rows(case["segs"], kw.pop("bt0"), kw.pop("N"), kw.pop("K0"), case["ld"], **kw)
        torch.cuda.synchronize()
        ops.poll_errors()
        return ops.gemm_rows_log()
    finally:
        ops.gemm_rows_log(False)
        for key in tuning:
            ops.set_tuning(key, 0)


# --------------------------------------------------------------------------------------------------
# the comparison
# --------------------------------------------------------------------------------------------------
_RATIOS = {}


def check_values(kernel, got, ref64, ref32, what):
    assert got.shape == ref64.shape, (kernel, what, got.shape, ref64.shape)
    assert bool(torch.isfinite(got).all()), f"{kernel} {what}: non-finite values"
    scale = float(ref64.abs().max())
    noise = float((ref32.double() - ref64).abs().max())
    err = float((got.double() - ref64).abs().max())
    floor = 4 * EPS32 * scale
    assert noise <= 16 * EPS32 * scale, f"{kernel} {what}: the float32 yardstick itself is off: noise {noise:.3e}, scale {scale:.3e}"
    ratio = err / max(noise, floor / 8) if max(noise, floor) > 0 else (0.0 if err == 0 else math.inf)
    _RATIOS[kernel] = max(_RATIOS.get(kernel, 0.0), ratio)
    print(f"{kernel} {what}: err {err:.3e} noise {noise:.3e} err/noise {ratio:.2f} err/bound {err / max(8 * noise + floor, 1e-300):.2f}")
    assert err <= 8 * noise + floor, f"{kernel} {what}: err {err:.3e} > 8 * noise {noise:.3e} + floor {floor:.3e}"


def check_case(kernel, case, what, values=True):
    """Every segment against the statement; exact zeros; the sentinel around and behind every output."""
    kw = case["kw"]
    kw64, kw32 = cast(kw, torch.float64), kw
    nco = kw["ncols_out"]
    keep = torch.ones_like(case["buf"], dtype=torch.bool)
    for s, (sg, (r0, r)) in enumerate(zip(case["segs"], case["spans"])):
        got = case["buf"][r0:r0 + r, :nco]
        keep[r0:r0 + r, :nco] = False
        z = exact_zero(sg, **kw)
        structural = exact_zero({k_: v for k_, v in sg.items() if k_ != "gate"}, **kw)
        bits = got.contiguous().view(torch.int32)
        assert bool((bits[structural] == 0).all()), f"{kernel} {what} seg {s}: masked rows / pad columns are not all +0"
        assert bool(((bits[z] & 0x7FFFFFFF) == 0).all()), f"{kernel} {what} seg {s}: a dropped gate left a value"
        if values:
            ref64 = gemm_rows_statement(cast(sg, torch.float64), **kw64)
            ref32 = gemm_rows_statement(sg, **kw32)
            check_values(kernel, got, ref64, ref32, f"{what} seg {s} ({r} rows)")
    assert bool((case["buf"][keep] == SENTINEL).all()), f"{kernel} {what}: wrote outside [rows, ncols_out]"


def run(k, *, terms=(), rows=None, N=None, ncols_out=None, K0=None, K1=None, form=None, expect=True, what="", seed=0,
        drop_required=False, **more):
    """One launch of kernel entry k (with its required terms), checked; expect: its name must / must not be in the log."""
    N = k["N"] if N is None else N
    terms = frozenset(terms) | (frozenset() if drop_required else k["required"])
    nco = ncols_out if ncols_out is not None else (N + 5 if "pad" in terms else N)
    rows = rows if rows is not None else row_sets(k, nco)[0]
    K0 = k["K0"] if K0 is None else K0
    K1 = k["K1"] if K1 is None else K1
    if form is None:
        form = k["forms"][0]
    # (the 80 x 96 kernel takes dword-aligned operands only together with add_table; everything else of an `aligned`
    # entry gets 16-byte rows)
    aligned = more.pop("aligned", k["aligned"] and not ("add_table" in terms and k["name"] == "gemm_rows_n96_kernel"))
    more.setdefault("gate_scale", k["gate_scale"])
    case = make_case(rows, N, K0, K1, terms=terms, ncols_out=nco, form=form, aligned=aligned, seed=seed, **more)
    log = launch(case, k["tuning"])
    label = f"{what} terms={sorted(terms)} rows={rows} N={N}/{nco} K={K0}+{K1} {form}"
    if expect:
        assert k["log"] in log, f"{k['name']} {label}: not reached: {log}"
    else:
        assert k["log"] not in log and log, f"{k['name']} {label}: expected another kernel: {log}"
    # (whatever a split-precision kernel computed is no fp32 product: structure only)
    check_case(k["name"] if expect else "(declined)", case, label, values="gemm_rows_split" not in log)
    return log


@pytest.fixture(scope="module", autouse=True)
def _mi355x_only_exact_fp32():
    if not torch.cuda.is_available():
        yield
        return
    from carca_replication_amd import ops

    if ops.num_cus() != 256:
        pytest.skip("the table's shapes reach their kernels on 256 CUs")
    tf32 = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = tf32
    for kname in sorted(_RATIOS):
        print(f"\nmax err/noise  {kname:<36} {_RATIOS[kname]:.2f}", end="")
    print()


# --------------------------------------------------------------------------------------------------
# CPU: the statement against the oracle, and the table against the routes file
# --------------------------------------------------------------------------------------------------
def test_statement_equals_the_oracles_joint_embedding():
    """AllEmbedding (oracle.all_embedding: e = (W_j [E[x] sqrt(d) ; W_f [a ; c] + b_f] + b_j + pos) mask) as two row products
    of the statement, in each of the three operand forms."""
    from oracle import carca_oracle as O

    d, g, na, nc, L, B, n_items = 12, 20, 33, 3, 7, 5, 40
    cfg = O.CarcaConfig(d=d, H=2, n_blocks=1, encoding="learnable")
    P = O.init_params(cfg, n_items, g, nc, na, L, seed=3, dtype=torch.float64)
    gen = torch.Generator().manual_seed(11)
    rnd = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64) * 2 - 1  # noqa: E731
    P["embeds.feats_embed.bias"], P["embeds.joint_embed.bias"] = rnd(g), rnd(d)
    x = torch.randint(0, n_items, (B, L), generator=gen)
    x[0, :3] = 0
    x[-1, -1] = 0
    table = rnd(n_items, na + 4)                      # attribute rows by item id, lda > K
    a_wide = torch.zeros(B, L + 2, na, dtype=torch.float64)
    a_wide[:, :L] = table[x][..., :na]
    a, c = a_wide[:, :L], rnd(B, L, nc)               # a: a [B, T, K] view with strided users
    Wf, Wj, E = P["embeds.feats_embed.weight"], P["embeds.joint_embed.weight"], P["embeds.items_embed.weight"]
    pos = O.position_term(P, cfg, L)
    want_e, want_q, want_z = O.all_embedding(P, cfg, x, a, c, O.get_mask(x, torch.float64), target=False, return_q=True)
    tight = dict(rtol=0, atol=1e-13)
    feats = dict(bt0=Wf[:, :na], N=g, K0=na, bt1=Wf[:, na:], K1=nc, bias=P["embeds.feats_embed.bias"])
    ids = x.reshape(-1)
    q_view = gemm_rows_statement(dict(a0=a, a1=c, ids=ids), **feats)
    q_gather = gemm_rows_statement(dict(a0=table[:, :na], a0_gather=True, a1=c.reshape(-1, nc), ids=ids), **feats)
    q_dense = gemm_rows_statement(dict(a0=a.reshape(-1, na), a1=c.reshape(-1, nc)), **feats)
    for q in (q_view, q_gather, q_dense):
        assert torch.allclose(q, want_q.reshape(-1, g), **tight)
    zq = torch.cat([want_z.reshape(-1, d), q_view], dim=1)
    joint = dict(N=d, bias=P["embeds.joint_embed.bias"], pos=pos, mask_rows=True, ncols_out=d + 4)
    e = gemm_rows_statement(dict(a0=zq, ids=ids, T=L, add_pos=True), bt0=Wj, K0=d + g, **joint)
    assert torch.allclose(e[:, :d], want_e.reshape(-1, d), **tight)
    assert bool((e[:, d:] == 0).all()) and bool((e[ids == 0] == 0).all())
    # the inference form: q's columns of zq (lda > K) against W_j's q columns, the item term from the projected table
    z_table = (E * d ** 0.5) @ Wj[:, :d].T
    e2 = gemm_rows_statement(dict(a0=zq[:, d:], ids=ids, T=L, add_pos=True), bt0=Wj[:, d:], K0=g, add_table=z_table, **joint)
    assert torch.allclose(e2[:, :d], want_e.reshape(-1, d), **tight)
    # the target side: no positions; and the other terms against their own plain statement
    want_t = O.all_embedding(P, cfg, x, a, c, O.get_mask(x, torch.float64), target=True)
    e3 = gemm_rows_statement(dict(a0=zq, ids=ids, T=L, add_pos=False), bt0=Wj, K0=d + g, **joint)
    assert torch.allclose(e3[:, :d], want_t.reshape(-1, d), **tight)
    add, gate, rs, cv = rnd(B * L, d), rnd(B * L, d), rnd(B * L), rnd(d)
    gate[::3] = 0.0
    v = 0.5 * (zq @ Wj.T) + add + rs[:, None] * cv[None, :]
    for drops in (False, True):
        m = torch.where(gate > 0, 0.75, 0.25 * 0.75) * (1.0 if not drops else (gate != 0).double())
        got = gemm_rows_statement(dict(a0=zq, add=add, gate=gate, rowscale=rs), bt0=Wj, N=d, K0=d + g, colvec=cv, alpha=0.5,
                                  gate_slope=0.25, gate_scale=0.75, gate_zero_drops=drops)
        assert torch.allclose(got, v * m, **tight)
        assert bool((got[exact_zero(dict(a0=zq, gate=gate), d, gate_zero_drops=drops)] == 0).all())


def test_the_table_covers_every_kernel_name_and_the_other_entries():
    from tests.test_hip_gemm_routes import KERNEL_NAMES

    logged = " ".join(k["log"] for k in KERNELS) + " " + " ".join(OTHER_ENTRIES)
    for name in KERNEL_NAMES:
        assert name in logged, name
    assert len(set(IDS)) == len(IDS)
    for fn in OTHER_ENTRIES.values():
        assert fn in globals(), fn
    for k in KERNELS:  # an admitted set only names terms, and what a kernel requires it admits
        assert k["admits"] <= ALL and k["required"] <= k["admits"], k["name"]


# --------------------------------------------------------------------------------------------------
# GPU: per kernel
# --------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", IDS)
def test_plain_product(name):
    """alpha = 1 and 0.37, with and without bias."""
    k = BY_NAME[name]
    for i, terms in enumerate([(), ("bias",), ("alpha",), ("alpha", "bias")]):
        run(k, terms=terms, what="plain", seed=i)


@gpu
@pytest.mark.parametrize("name", IDS)
def test_each_admitted_term_and_all_together(name):
    k = BY_NAME[name]
    admitted = [t for t in TERMS if t in k["admits"]]
    for i, t in enumerate(admitted):
        run(k, terms=(t,), what="one term", seed=10 + i)
    run(k, terms=admitted, what="all admitted", seed=30)
    run(k, terms=admitted, rows=row_sets(k, k["N"] + 5 if "pad" in admitted else k["N"])[1], what="all admitted, two segments", seed=31)


@gpu
@pytest.mark.parametrize("name", IDS)
def test_each_declined_term_goes_to_another_kernel_and_is_right(name):
    """A term the launcher does not admit: the same call with it added gives the right values from another kernel.  Also a
    required term taken away, a k-source or operand form the launcher refuses, and the N and K0 next to its envelope."""
    k = BY_NAME[name]
    base = [t for t in ("bias", "mask") if t in k["admits"]]
    for i, t in enumerate(t for t in TERMS if t not in k["admits"]):
        run(k, terms=base + [t], expect=False, what="declined term", seed=40 + i)
    if k["gate_scale"] == 0.0:  # (gemm_rows_sk_kernel: the embedding's gate_scale = 0 only)
        run(k, terms=base, gate_scale=0.8, expect=False, what="declined gate_scale", seed=50)
    if k["required"]:
        run(k, terms=[t for t in base if t not in k["required"]], expect=False, drop_required=True, what="required term dropped", seed=51)
    for i, K1 in enumerate(K1 for K1 in (0, 1, 3, 6, 8) if K1 not in k["k1_ok"]):
        run(k, terms=base, K1=K1, expect=False, what="declined K1", seed=52 + i)
    for i, form in enumerate(f for f in ("dense", "view", "gather") if f not in k["forms"]):
        run(k, terms=base, form=form, expect=False, what="declined operand form", seed=60 + i)
    if k["aligned"] and "dense" in k["forms"]:
        run(k, terms=base, aligned=False, expect=False, what="declined alignment", seed=63)
    for i, (N, nco) in enumerate(k["ns_declined"]):
        run(k, terms=base, N=N, ncols_out=nco, expect=False, what="declined N", seed=64 + i)
    for i, K0 in enumerate(k["k0s_declined"]):
        run(k, terms=base, K0=K0, expect=False, what="declined K0", seed=70 + i)


@gpu
@pytest.mark.parametrize("name", [k["name"] for k in KERNELS if "gate" in k["admits"]])
def test_gate(name):
    """Gate entries positive, negative and exactly 0; gate_zero_drops on and off; gate_scale 0 (= 1), 1 and 0.8."""
    k = BY_NAME[name]
    i = 0
    for drops in (False, True):
        for gs in (0.0, 1.0, 0.8):
            run(k, terms=("gate", "bias", "mask"), gate_scale=gs, zero_drops=drops, what=f"gate drops={drops} scale={gs}", seed=80 + i)
            i += 1


@gpu
@pytest.mark.parametrize("name", IDS)
def test_row_edges(name):
    """1 to 4 segments, lengths BM - 1, BM, BM + 1 and one row; ids with zeros scattered, at a segment's end, as a 64-row chunk."""
    k = BY_NAME[name]
    terms = [t for t in ("bias", "mask", "add_table", "pos") if t in k["admits"]]
    for i, rows in enumerate(row_sets(k, k["N"])):
        run(k, terms=terms, rows=rows, what="rows", seed=90 + i)


@gpu
@pytest.mark.parametrize("name", IDS)
def test_k_edges(name):
    """K0 with tails of 0, 1, 3 and 31 past the kernel's K step where its launcher allows; K1 in {0, 1, 3, 6, 8}."""
    k = BY_NAME[name]
    base = [t for t in ("bias", "mask") if t in k["admits"]]
    for i, K0 in enumerate(k["k0s"]):
        # (the 80 x 96 kernel takes a K0 that is no multiple of 4 only in its loose mode: with add_table)
        terms = base + (["add_table"] if name == "gemm_rows_n96_kernel" and K0 % 4 else [])
        run(k, terms=terms, K0=K0, what="K0", seed=100 + i)
    for i, K1 in enumerate(k["k1_ok"]):
        run(k, terms=base, K1=K1, K0=k["k0s"][-1] if K1 in (1, 8) else None, what="K1", seed=110 + i)


@gpu
@pytest.mark.parametrize("name", IDS)
def test_n_edges(name):
    """Both sides of every column-tile boundary; the narrow last blocks (33, 64, 65, 66 columns); N in {65, 90, 96} with
    ncols_out in {N, 96} for the narrow kernels."""
    k = BY_NAME[name]
    terms = [t for t in ("bias", "mask", "add_table", "gate") if t in k["admits"]]
    for i, (N, nco) in enumerate(k["ns"]):
        run(k, terms=terms, N=N, ncols_out=nco, what="N", seed=120 + i)


@gpu
@pytest.mark.parametrize("name", IDS)
def test_operand_forms(name):
    """a0 as a column slice at a 4-byte-aligned, not 16-byte-aligned address (where the launcher takes it), as a [B, T, K]
    view with strided users, gathered from a table; a1 with lda1 > K1 throughout."""
    k = BY_NAME[name]
    terms = [t for t in ("bias", "mask", "pos") if t in k["admits"]]
    for i, form in enumerate(k["forms"]):
        run(k, terms=terms, form=form, what="operand form", seed=130 + i)
    if name == "gemm_rows_n96_kernel":  # its loose mode: dword-aligned rows
        run(k, terms=terms + ["add_table"], form="dense", K0=130, what="operand form (loose)", seed=135)


# --------------------------------------------------------------------------------------------------
# GPU: the other entry points
# --------------------------------------------------------------------------------------------------
@gpu
def test_grouped_launch_against_float64():
    """ops.gemm_rows_group: narrow products share gemm_rows_group_kernel's launch (the log stays empty: nothing was launched
    one by one), each with its own terms."""
    from carca_replication_amd import ops

    k = BY_NAME["gemm_rows_kernel<128,32,32,4,1>"]
    term_sets = [TERMS, ("bias", "gate", "mask"), ("alpha", "add_table", "pos"), ()]
    cases = [make_case(row_sets(k, 95)[i % 3][:3], 90 - i, 64 + i, 6 if i % 2 else 0, terms=t, seed=140 + i, zero_drops=bool(i % 2),
                       gate_scale=0.8) for i, t in enumerate(term_sets)]
    ops.gemm_rows_log(True)
    try:
        ops.gemm_rows_group([dict(segs=c["segs"], out_ld=c["ld"], **c["kw"]) for c in cases])
        torch.cuda.synchronize()
        log = ops.gemm_rows_log()
    finally:
        ops.gemm_rows_log(False)
    assert log == "", log
    for i, c in enumerate(cases):
        check_case("gemm_rows_group_kernel", c, f"product {i}")
    # and under key 0 = 6 each product takes its own launch of the same kernel: the same bits
    again = [make_case(row_sets(k, 95)[i % 3][:3], 90 - i, 64 + i, 6 if i % 2 else 0, terms=t, seed=140 + i, zero_drops=bool(i % 2),
                       gate_scale=0.8) for i, t in enumerate(term_sets)]
    ops.set_tuning(0, 6)
    try:
        ops.gemm_rows_log(True)
        ops.gemm_rows_group([dict(segs=c["segs"], out_ld=c["ld"], **c["kw"]) for c in again])
        torch.cuda.synchronize()
        log = ops.gemm_rows_log()
    finally:
        ops.gemm_rows_log(False)
        ops.set_tuning(0, 0)
    assert log.count("gemm_rows_kernel<128,32,32,4,1>") == len(again), log
    for a, b in zip(cases, again):
        assert torch.equal(a["buf"], b["buf"])


def _embed_inputs(seed, B, Ts, na, nc, d, g, n_items):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    u = lambda *s: torch.rand(*s, device="cuda", generator=gen) * 2 - 1  # noqa: E731
    w = dict(items_w=u(n_items, d), feats_w=u(g, na + nc), feats_b=u(g), joint_w=u(d, d + g), joint_b=u(d), pos=u(Ts[0], d))
    segs = []
    for i, T in enumerate(Ts):
        ids = make_ids(B * T, gen).view(B, T)
        attrs = u(B, T + 2, na)[:, :T] if i == 0 else u(B, T, na)  # (the profile's users strided: walked in place)
        segs.append((ids, attrs, u(B, T, nc), i == 0))
    return w, segs


@gpu
@pytest.mark.parametrize("own_gather", [False, True], ids=["gather rides", "gather's own launch"])
def test_embed_fwd_all_three_stages(own_gather):
    """ops.embed_fwd (gather + feature product + joint product): q and e against the statement, the gathered item columns
    bit for bit; once with the gather riding in the feature product's launch (one workgroup more than the product has
    tiles), once with its own launch (key 0 = 19)."""
    from carca_replication_amd import ops

    B, Ts, na, nc, d, g, ld_e = 128, (7, 70), 2016, 6, 90, 450, 96
    w, segs = _embed_inputs(150, B, Ts, na, nc, d, g, N_TAB)
    rows = [B * T for T in Ts]
    tuning = {0: 19} if own_gather else {0: 2}
    for key, value in tuning.items():
        ops.set_tuning(key, value)
    try:
        ops.gemm_rows_log(True)
        outs, zq = ops.embed_fwd(segs, w["items_w"], w["feats_w"], w["feats_b"], w["joint_w"], w["joint_b"], w["pos"], ld_e)
        torch.cuda.synchronize()
        log = ops.gemm_rows_log()
    finally:
        ops.gemm_rows_log(False)
        for key in tuning:
            ops.set_tuning(key, 0)
    tiles = sum(-(-r // 384) for r in rows) * 5
    if own_gather:
        assert "gemm_rows_cu_kernel" not in log and "_sk" not in log and f"rows={sum(rows)} N={g}" in log, log
    else:
        assert f"gemm_rows_cu_kernel<0,3> rows={sum(rows)} N={g} K={na + nc} grid={tiles + 1};" in log, log
    ids = torch.cat([s[0].reshape(-1) for s in segs])
    scale = torch.tensor(math.sqrt(d), dtype=torch.float32, device="cuda")
    assert torch.equal(zq[:, :d], w["items_w"][ids.long()] * scale)
    r0 = 0
    for (ids_s, attrs, ctx, add_pos), e, r in zip(segs, outs, rows):
        refs = []
        for dt in (torch.float64, torch.float32):
            W = cast(w, dt)
            q = gemm_rows_statement(dict(a0=attrs.to(dt), a1=ctx.to(dt), ids=ids_s), bt0=W["feats_w"][:, :na], N=g, K0=na,
                                    bt1=W["feats_w"][:, na:], K1=nc, bias=W["feats_b"], mask_rows=True)
            z = W["items_w"][ids_s.reshape(-1).long()] * scale.to(dt)
            ej = gemm_rows_statement(dict(a0=torch.cat([z, q], dim=1), ids=ids_s, T=ids_s.shape[1], add_pos=add_pos),
                                     bt0=W["joint_w"], N=d, K0=d + g, bias=W["joint_b"], pos=W["pos"], mask_rows=True, ncols_out=ld_e)
            refs.append((q, ej))
        check_values("embed_fwd", zq[r0:r0 + r, d:], refs[0][0], refs[1][0], f"q own_gather={own_gather}")
        check_values("embed_fwd", e.reshape(r, ld_e), refs[0][1], refs[1][1], f"e own_gather={own_gather}")
        dead = ids_s.reshape(-1) == 0
        assert bool((zq[r0:r0 + r, d:][dead].view(torch.int32) == 0).all())
        assert bool((e.reshape(r, ld_e)[dead].view(torch.int32) == 0).all()) and bool((e[..., d:].contiguous().view(torch.int32) == 0).all())
        r0 += r


@gpu
def test_dedup_entry_against_float64():
    """gemm_rows_skc_kernel<2>+dedup: the model's evaluation forward at the smallest batch that still takes it (B_MODEL of the
    routes file); q of every row against the statement, rows with id 0 bitwise zero."""
    from carca_replication_amd import ops
    from tests.model_util import build_model
    from tests.test_hip_gemm_routes import B_MODEL, D, G, L, NA, NC, NT

    torch.manual_seed(5)
    model = build_model(dict(d=D, H=3, n_blocks=2), N_TAB, G, NC, NA, L).cuda().eval()
    gen = torch.Generator(device="cuda").manual_seed(160)
    with torch.no_grad():
        model.embeds.feats_embed.bias.copy_(torch.rand(G, device="cuda", generator=gen) * 2 - 1)
        model.embeds.feats_embed.weight.copy_(torch.rand(G, NA + NC, device="cuda", generator=gen) * 2 - 1)
    table = torch.rand(N_TAB, NA, device="cuda", generator=gen) * 2 - 1  # (equal ids bring equal attribute rows: groups to merge)
    segs = []
    for T in (L, NT):
        ids = make_ids(B_MODEL * T, gen).view(B_MODEL, T)
        segs.append((ids, table[ids.long()].contiguous(), torch.rand(B_MODEL, T, NC, device="cuda", generator=gen) * 2 - 1))
    ops.gemm_rows_log(True)
    try:
        with torch.no_grad():
            model(profile=segs[0], targets=[segs[1]])
        torch.cuda.synchronize()
        ops.poll_errors()
        log = ops.gemm_rows_log()
    finally:
        ops.gemm_rows_log(False)
    assert "gemm_rows_skc_kernel<2>+dedup" in log, log
    q = model.__dict__["_plan"]["zq"][:, D:]
    r0 = 0
    for ids, attrs, ctx in segs:
        r = ids.numel()
        refs = []
        for dt in (torch.float64, torch.float32):
            W, b = model.embeds.feats_embed.weight.detach().to(dt), model.embeds.feats_embed.bias.detach().to(dt)
            refs.append(gemm_rows_statement(dict(a0=attrs.to(dt), a1=ctx.to(dt), ids=ids), bt0=W[:, :NA], N=G, K0=NA, bt1=W[:, NA:],
                                            K1=NC, bias=b, mask_rows=True))
        check_values("gemm_rows_skc_kernel<2>+dedup", q[r0:r0 + r], refs[0], refs[1], f"q of {r} rows")
        assert bool((q[r0:r0 + r][ids.reshape(-1) == 0].view(torch.int32) == 0).all())
        r0 += r
