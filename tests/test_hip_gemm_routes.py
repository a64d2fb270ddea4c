"""Which kernel every row product takes (csrc/gemm.hip: gemm_rows_choose + gemm_rows_dispatch, gemm_stream.hip,
gemm_split.hip): a table of (entry point, shape, tuning keys) -> the complete gemm_rows_log string -- kernel name, rows, N,
K and grid.  The expected strings were recorded on an MI355X (256 CUs) BEFORE the three entry points were folded into one
dispatcher; they pin every routing decision, including the differences between the entry points that nobody has
explained yet (the passenger entry never tries gemm_rows_n96s_kernel, see `n96_cu_*`).

Entries: "rows" = carca_gemm_rows (ops.gemm_rows), "group" = carca_gemm_rows_group, "embed" = carca_embed_fwd with all
three stages (the training forward's call: carca_gemm_rows_passenger, then the joint product), "model" = the model's
evaluation forward (carca_gemm_rows_feat_dedup).  Operands are zeros, ids ones: values are not checked here."""
import pytest
import torch

pytestmark = pytest.mark.gpu

C2 = dict(rows=[6400, 12928], N=450, K0=4096, K1=6)  # 128 x (50 + 101) rows of the feature product
C5 = dict(rows=[6400, 128128], N=450, K0=512, K1=6)
JOINT = dict(N=90, K0=450, a_off=90, ld=96, ncols_out=96, table=True)  # the inference joint product (test_hip_gemm_stream)
NARROW = dict(rows=[19328], N=90, K0=512, ld=96, ncols_out=96)
WIDE_N96 = dict(rows=[64000, 129280], N=90, K0=256, ld=180, ncols_out=90)  # N <= 96 with rows enough for GEMM_CU
D, G, NA, NC, L, NT = 90, 450, 4096, 6, 50, 101
B_MODEL = 87  # the smallest batch whose feature product the parent still gave to gemm_rows_skc_kernel


def _case(name, entry, spec, tuning=None, **more):
    return dict(name=name, entry=entry, spec=dict(spec, **more), tuning=tuning or {})


CASES = [
    # ---- the feature product at C2: stream-K kernels, their switches, the forced kernels
    _case("c2", "rows", C2),
    _case("c2_k23", "rows", C2, {0: 23}),
    _case("c2_k15", "rows", C2, {0: 15}),
    _case("c2_k158", "rows", C2, {0: 158}),
    _case("c2_k8", "rows", C2, {0: 8}),
    _case("c2_k19", "rows", C2, {0: 19}),
    _case("c2_k1", "rows", C2, {0: 1}),
    _case("c2_k2", "rows", C2, {0: 2}),
    _case("c2_k3", "rows", C2, {0: 3}),
    _case("c2_k4", "rows", C2, {0: 4}),
    _case("c2_k7", "rows", C2, {0: 7}),
    _case("c2_k7_nomask", "rows", C2, {0: 7}, mask=False),
    _case("c2_nomask", "rows", C2, mask=False),
    _case("c2_n449", "rows", C2, N=449),
    _case("c2_n449_k23", "rows", C2, {0: 23}, N=449),
    _case("c2_n434", "rows", C2, N=434),
    _case("c2_n434_k23", "rows", C2, {0: 23}, N=434),
    _case("c2_k25", "rows", C2, {0: 25}, K0=512),
    # (gemm_rows_sk_kernel takes the plain epilogue only: gate_scale = 0, as the embedding passes it)
    _case("c2_k23_g0", "rows", C2, {0: 23}, gate_scale=0.0),
    _case("c2_n449_k23_g0", "rows", C2, {0: 23}, N=449, gate_scale=0.0),
    _case("c2_k19_g0", "rows", C2, {0: 19}, gate_scale=0.0),
    # 384 x 128 tiles: chosen where they fill one round and 96-wide ones would not (the stream-K kernel first where rows
    # are masked), forced by key 0 = 7 where the tiled kernel would run
    _case("cu128", "rows", C2, rows=[7600, 15352]),
    _case("cu128_nomask", "rows", C2, rows=[7600, 15352], mask=False),
    _case("tiled_k0", "rows", C2, rows=[8960, 17920], mask=False),
    _case("tiled_k7", "rows", C2, {0: 7}, rows=[8960, 17920], mask=False),
    # ---- split precision (key 16), its register-staged kernel (key 0 = 21), and bit 4 at a fixture size
    _case("c2_split1", "rows", C2, {16: 1}),
    _case("c2_split2", "rows", C2, {16: 2}),
    _case("c2_split1_k21", "rows", C2, {16: 1, 0: 21}),
    _case("small_split17", "rows", dict(rows=[1000], N=450, K0=128, K1=6), {16: 17}),
    _case("small_split16_off", "rows", dict(rows=[1000], N=450, K0=128, K1=6)),
    # ---- short K, many tiles per CU: gemm_rows_cus_kernel
    _case("c5", "rows", C5),
    _case("c5_k24", "rows", C5, {0: 24}),
    _case("cus_n449", "rows", dict(rows=[90000, 60000], N=449, K0=192, K1=6)),
    _case("cus_n434", "rows", dict(rows=[90000, 60000], N=434, K0=192, K1=6)),
    # ---- narrow outputs: 80 x 96 blocks, 128 x 32, 64 x 96
    _case("narrow", "rows", NARROW),
    _case("narrow_k12", "rows", NARROW, {0: 12}),
    _case("narrow_k9", "rows", NARROW, {0: 9}),
    _case("narrow_k10", "rows", NARROW, {0: 10}),
    _case("narrow_k4", "rows", NARROW, {0: 4}),
    _case("narrow_k11", "rows", dict(rows=[1000], N=90, K0=64, ld=96, ncols_out=96), {0: 11}),
    _case("narrow_small", "rows", dict(rows=[1000], N=90, K0=64, ld=96, ncols_out=96)),
    # ---- the persistent narrow-output kernel
    _case("joint_c5", "rows", JOINT, rows=[6400, 128128]),
    _case("joint_c5_k26", "rows", JOINT, {0: 26}, rows=[6400, 128128]),
    _case("joint_c2", "rows", JOINT, rows=[6400, 12928]),
    _case("joint_c2_k27", "rows", JOINT, {0: 27}, rows=[6400, 12928]),
    # ---- N <= 96 over enough rows for the one-block-per-CU choice: carca_gemm_rows tries gemm_rows_n96s_kernel first, the
    # passenger entry does not
    _case("n96_cu_rows", "rows", WIDE_N96),
    _case("n96_cu_rows_k26", "rows", WIDE_N96, {0: 26}),
    _case("n96_cu_embed", "embed", dict(B=1280, T=[50, 101], n_attrs=256, n_ctx=0, d=90, g=90)),
    # ---- grouped narrow products
    _case("group", "group", dict(n=2, rows=[1000], N=90, K0=90, ld=96, ncols_out=96)),
    _case("group_k6", "group", dict(n=2, rows=[1000], N=90, K0=90, ld=96, ncols_out=96), {0: 6}),
]
# the training forward's embedding (passenger entry) and the evaluation forward (dedup entry) under the gather's switches
for k0 in (0, 8, 15, 19, 23, 158):
    CASES.append(_case(f"embed_c2_k{k0}", "embed", dict(B=128, T=[L, NT], n_attrs=NA, n_ctx=NC, d=D, g=G), {0: k0}))
    for k20 in (0, 1) if k0 != 23 else ():
        CASES.append(_case(f"model_k{k0}_d{k20}", "model", dict(B=B_MODEL), {0: k0, 20: k20}))

EXPECTED = {
    "c2": "gemm_rows_skc_kernel<2> rows=19328 N=450 K=4102 grid=256;",
    "c2_k23": "gemm_rows_cu_kernel<0,3> rows=19328 N=450 K=4102 grid=255;",
    "c2_k15": "gemm_rows_cu_kernel<0,3> rows=19328 N=450 K=4102 grid=255;",
    "c2_k158": "gemm_rows_cu_kernel<0,3> rows=19328 N=450 K=4102 grid=255;",
    "c2_k8": "gemm_rows_skc_kernel<2> rows=19328 N=450 K=4102 grid=256;",
    "c2_k19": "gemm_rows_skc_kernel<2> rows=19328 N=450 K=4102 grid=256;",
    "c2_k1": "gemm_rows_kernel<128,96,32,1,1> rows=19328 N=450 K=4102 grid=755;",
    "c2_k2": "gemm_rows_skc_kernel<2> rows=19328 N=450 K=4102 grid=256;",
    "c2_k3": "gemm_rows_cu_kernel<0,3> rows=19328 N=450 K=4102 grid=255;",
    "c2_k4": "gemm_rows_kernel<128,96,32,1,0> rows=19328 N=450 K=4102 grid=755;",
    "c2_k7": "gemm_rows_skc_kernel<2> rows=19328 N=450 K=4102 grid=256;",
    "c2_k7_nomask": "gemm_rows_cu_kernel<0,3> rows=19328 N=450 K=4102 grid=255;",
    "c2_nomask": "gemm_rows_cu_kernel<0,3> rows=19328 N=450 K=4102 grid=255;",
    "c2_n449": "gemm_rows_skc_kernel<1> rows=19328 N=449 K=4102 grid=256;",
    "c2_n449_k23": "gemm_rows_cu_kernel<0,3> rows=19328 N=449 K=4102 grid=255;",
    "c2_n434": "gemm_rows_skc_kernel<0> rows=19328 N=434 K=4102 grid=256;",
    "c2_n434_k23": "gemm_rows_cu_kernel<0,3> rows=19328 N=434 K=4102 grid=255;",
    "c2_k25": "gemm_rows_cus_kernel<2> rows=19328 N=450 K=518 grid=255;",
    "c2_k23_g0": "gemm_rows_sk_kernel<2> rows=19328 N=450 K=4102 grid=255;",
    "c2_n449_k23_g0": "gemm_rows_sk_kernel<1> rows=19328 N=449 K=4102 grid=255;",
    "c2_k19_g0": "gemm_rows_skc_kernel<2> rows=19328 N=450 K=4102 grid=256;",
    "cu128": "gemm_rows_skc_kernel<2> rows=22952 N=450 K=4102 grid=256;",
    "cu128_nomask": "gemm_rows_cu_kernel<0,4> rows=22952 N=450 K=4102 grid=240;",
    "tiled_k0": "gemm_rows_kernel<128,96,32,1,1> rows=26880 N=450 K=4102 grid=1050;",
    "tiled_k7": "gemm_rows_cu_kernel<0,4> rows=26880 N=450 K=4102 grid=284;",
    "c2_split1": "gemm_rows_split_dma_kernel<bf16x3> rows=19328 N=450 K=4102 grid=255;",
    "c2_split2": "gemm_rows_split_dma_kernel<fp16x2> rows=19328 N=450 K=4102 grid=255;",
    "c2_split1_k21": "gemm_rows_split_kernel<bf16x3> rows=19328 N=450 K=4102 grid=255;",
    "small_split17": "gemm_rows_split_dma_kernel<bf16x3> rows=1000 N=450 K=134 grid=15;",
    "small_split16_off": "gemm_rows_kernel<128,32,32,4,1> rows=1000 N=450 K=134 grid=120;",
    "c5": "gemm_rows_cus_kernel<2> rows=134528 N=450 K=518 grid=256;",
    "c5_k24": "gemm_rows_cu_kernel<0,3> rows=134528 N=450 K=518 grid=1755;",
    "cus_n449": "gemm_rows_cus_kernel<1> rows=150000 N=449 K=198 grid=256;",
    "cus_n434": "gemm_rows_cus_kernel<0> rows=150000 N=434 K=198 grid=256;",
    "narrow": "gemm_rows_n96_kernel rows=19328 N=90 K=512 grid=242;",
    "narrow_k12": "gemm_rows_kernel<128,32,32,4,1> rows=19328 N=90 K=512 grid=453;",
    "narrow_k9": "gemm_rows_kernel<64,96,32,4,1> rows=19328 N=90 K=512 grid=302;",
    "narrow_k10": "gemm_rows_kernel<64,96,32,2,1> rows=19328 N=90 K=512 grid=302;",
    "narrow_k4": "gemm_rows_kernel<128,32,32,4,0> rows=19328 N=90 K=512 grid=453;",
    "narrow_k11": "gemm_rows_n96_kernel rows=1000 N=90 K=64 grid=13;",
    "narrow_small": "gemm_rows_kernel<128,32,32,4,1> rows=1000 N=90 K=64 grid=24;",
    "joint_c5": "gemm_rows_n96s_kernel rows=134528 N=90 K=450 grid=256;",
    "joint_c5_k26": "gemm_rows_kernel<128,96,32,1,1> rows=134528 N=90 K=450 grid=1051;",
    "joint_c2": "gemm_rows_n96_kernel rows=19328 N=90 K=450 grid=242;",
    "joint_c2_k27": "gemm_rows_n96s_kernel rows=19328 N=90 K=450 grid=121;",
    "n96_cu_rows": "gemm_rows_n96s_kernel rows=193280 N=90 K=256 grid=256;",
    "n96_cu_rows_k26": "gemm_rows_cu_kernel<0,3> rows=193280 N=90 K=256 grid=504;",
    "n96_cu_embed": ("gemm_rows_cu_kernel<0,3> rows=193280 N=90 K=256 grid=504;"
                    "gemm_rows_cu_kernel<0,3> rows=193280 N=90 K=180 grid=504;"),
    "group": "",
    "group_k6": ("gemm_rows_kernel<128,32,32,4,1> rows=1000 N=90 K=90 grid=24;"
                "gemm_rows_kernel<128,32,32,4,1> rows=1000 N=90 K=90 grid=24;"),
    "embed_c2_k0": ("gemm_rows_skc_kernel<2> rows=19328 N=450 K=4102 grid=256;"
                   "gemm_rows_n96_kernel rows=19328 N=90 K=540 grid=242;"),
    "model_k0_d0": ("gemm_rows_kernel<128,32,32,4,1> rows=16 N=90 K=90 grid=3;"
                   "gemm_rows_skc_kernel<2>+dedup rows=13137 N=450 K=4102 grid=256;"
                   "gemm_rows_n96_kernel rows=13137 N=90 K=450 grid=165;"),
    "model_k0_d1": ("gemm_rows_kernel<128,32,32,4,1> rows=16 N=90 K=90 grid=3;"
                   "gemm_rows_skc_kernel<2> rows=13137 N=450 K=4102 grid=256;"
                   "gemm_rows_n96_kernel rows=13137 N=90 K=450 grid=165;"),
    "embed_c2_k8": ("gemm_rows_skc_kernel<2> rows=19328 N=450 K=4102 grid=256;"
                   "gemm_rows_kernel<128,32,32,4,1> rows=19328 N=90 K=540 grid=453;"),
    "model_k8_d0": ("gemm_rows_kernel<128,32,32,4,1> rows=16 N=90 K=90 grid=3;"
                   "gemm_rows_skc_kernel<2>+dedup rows=13137 N=450 K=4102 grid=256;"
                   "gemm_rows_kernel<128,32,32,4,1> rows=13137 N=90 K=450 grid=309;"),
    "model_k8_d1": ("gemm_rows_kernel<128,32,32,4,1> rows=16 N=90 K=90 grid=3;"
                   "gemm_rows_skc_kernel<2> rows=13137 N=450 K=4102 grid=256;"
                   "gemm_rows_kernel<128,32,32,4,1> rows=13137 N=90 K=450 grid=309;"),
    "embed_c2_k15": ("gemm_rows_cu_kernel<0,3> rows=19328 N=450 K=4102 grid=256;"
                    "gemm_rows_kernel<128,32,32,4,1> rows=19328 N=90 K=540 grid=453;"),
    "model_k15_d0": ("gemm_rows_kernel<128,32,32,4,1> rows=16 N=90 K=90 grid=3;"
                    "gemm_rows_cu_kernel<0,3> rows=13137 N=450 K=4102 grid=175;"
                    "gemm_rows_kernel<128,32,32,4,1> rows=13137 N=90 K=450 grid=309;"),
    "model_k15_d1": ("gemm_rows_kernel<128,32,32,4,1> rows=16 N=90 K=90 grid=3;"
                    "gemm_rows_cu_kernel<0,3> rows=13137 N=450 K=4102 grid=175;"
                    "gemm_rows_kernel<128,32,32,4,1> rows=13137 N=90 K=450 grid=309;"),
    "embed_c2_k19": ("gemm_rows_skc_kernel<2> rows=19328 N=450 K=4102 grid=256;"
                    "gemm_rows_kernel<128,32,32,4,1> rows=19328 N=90 K=540 grid=453;"),
    "model_k19_d0": ("gemm_rows_kernel<128,32,32,4,1> rows=16 N=90 K=90 grid=3;"
                    "gemm_rows_skc_kernel<2>+dedup rows=13137 N=450 K=4102 grid=256;"
                    "gemm_rows_kernel<128,32,32,4,1> rows=13137 N=90 K=450 grid=309;"),
    "model_k19_d1": ("gemm_rows_kernel<128,32,32,4,1> rows=16 N=90 K=90 grid=3;"
                    "gemm_rows_skc_kernel<2> rows=13137 N=450 K=4102 grid=256;"
                    "gemm_rows_kernel<128,32,32,4,1> rows=13137 N=90 K=450 grid=309;"),
    "embed_c2_k23": ("gemm_rows_sk_kernel<2> rows=19328 N=450 K=4102 grid=256;"
                    "gemm_rows_kernel<128,32,32,4,1> rows=19328 N=90 K=540 grid=453;"),
    "embed_c2_k158": ("gemm_rows_cu_kernel<0,3> rows=19328 N=450 K=4102 grid=255;"
                     "gemm_rows_kernel<128,32,32,4,1> rows=19328 N=90 K=540 grid=453;"),
    "model_k158_d0": ("gemm_rows_kernel<128,32,32,4,1> rows=16 N=90 K=90 grid=3;"
                     "gemm_rows_cu_kernel<0,3> rows=13137 N=450 K=4102 grid=175;"
                     "gemm_rows_kernel<128,32,32,4,1> rows=13137 N=90 K=450 grid=309;"),
    "model_k158_d1": ("gemm_rows_kernel<128,32,32,4,1> rows=16 N=90 K=90 grid=3;"
                     "gemm_rows_cu_kernel<0,3> rows=13137 N=450 K=4102 grid=175;"
                     "gemm_rows_kernel<128,32,32,4,1> rows=13137 N=90 K=450 grid=309;"),
}

# every kernel-name string the row launchers can log (the 128-row tiled kernel's non-buffer instantiations need operands
# past 4 GiB or key 0 = 4)
KERNEL_NAMES = ["gemm_rows_kernel<128,32,32,4,1>", "gemm_rows_kernel<128,32,32,4,0>", "gemm_rows_kernel<128,96,32,1,1>",
                "gemm_rows_kernel<128,96,32,1,0>", "gemm_rows_kernel<64,96,32,4,1>", "gemm_rows_kernel<64,96,32,2,1>",
                "gemm_rows_cu_kernel<0,3>", "gemm_rows_cu_kernel<0,4>", "gemm_rows_sk_kernel<1>", "gemm_rows_sk_kernel<2>",
                "gemm_rows_skc_kernel<0>", "gemm_rows_skc_kernel<1>", "gemm_rows_skc_kernel<2>", "+dedup",
                "gemm_rows_n96_kernel", "gemm_rows_cus_kernel<0>", "gemm_rows_cus_kernel<1>", "gemm_rows_cus_kernel<2>",
                "gemm_rows_n96s_kernel", "gemm_rows_split_dma_kernel<", "gemm_rows_split_kernel<"]
# the key-0 values that reach a row product (carca_common.h: CARCA_GV_*; the others act on the weight gradient or
# the gather's own launch)
ROW_KEY0 = [1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 15, 19, 21, 23, 24, 25, 26, 27, 158]


def _rows_args(rows, N, K0, K1=0, mask=True, ld=None, ncols_out=None, table=False, a_off=0, gate_scale=1.0):
    ld = ld or (N + 3) // 4 * 4
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    w = z(N, a_off + K0 + K1)
    segs = []
    for r in rows:
        sg = dict(a0=z(r, a_off + K0)[:, a_off:], ids=torch.ones(r, dtype=torch.int32, device="cuda"))
        if K1:
            sg["a1"] = z(r, K1)
        segs.append(sg)
    kw = dict(bias=z(N), mask_rows=mask, ncols_out=ncols_out or N, gate_scale=gate_scale)
    if K1:
        kw.update(bt1=w[:, a_off + K0:], K1=K1)
    if table:
        kw["add_table"] = z(1000, N + 6)[:, :N]
    return dict(segs=segs, bt0=w[:, a_off:a_off + K0], N=N, K0=K0, out_ld=ld, **kw)


def run_case(case):
    """The case's launches, under its tuning keys; returns the log.  (Also what recorded EXPECTED.)"""
    from carca_replication_amd import ops

    spec, entry = case["spec"], case["entry"]
    for key, value in case["tuning"].items():
        ops.set_tuning(key, value)
    try:
        if entry == "rows":
            args = _rows_args(**spec)
            ops.gemm_rows_log(True)
            ops.gemm_rows(args.pop("segs"), args.pop("bt0"), args.pop("N"), args.pop("K0"), args.pop("out_ld"), **args)
        elif entry == "group":
            calls = [_rows_args(**{k: v for k, v in spec.items() if k != "n"}) for _ in range(spec["n"])]
            ops.gemm_rows_log(True)
            ops.gemm_rows_group(calls)
        elif entry == "embed":
            B, d, g, na, nc = spec["B"], spec["d"], spec["g"], spec["n_attrs"], spec["n_ctx"]
            z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
            segs = [(torch.ones(B, T, dtype=torch.int32, device="cuda"), z(B, T, na), z(B, T, nc), False) for T in spec["T"]]
            ops.gemm_rows_log(True)
            ops.embed_fwd(segs, z(16, d), z(g, na + nc), z(g), z(d, d + g), z(d), None, 96)
        else:
            from tests.model_util import build_model

            B = spec["B"]
            model = build_model(dict(d=D, H=3, n_blocks=2), 16, G, NC, NA, L).cuda().eval()
            seg = lambda T: (torch.ones(B, T, dtype=torch.int32, device="cuda"), torch.zeros(B, T, NA, device="cuda"),  # noqa: E731
                             torch.zeros(B, T, NC, device="cuda"))
            ops.gemm_rows_log(True)
            with torch.no_grad():
                model(profile=seg(L), targets=[seg(NT)])
        torch.cuda.synchronize()
        return ops.gemm_rows_log()
    finally:
        ops.gemm_rows_log(False)
        for key in case["tuning"]:
            ops.set_tuning(key, 0)


@pytest.fixture(scope="module", autouse=True)
def _mi355x_only():
    from carca_replication_amd import ops

    if ops.num_cus() != 256:
        pytest.skip("the expected grids were recorded on 256 CUs")


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_route(case):
    assert run_case(case) == EXPECTED[case["name"]]


def test_the_table_covers_every_kernel_name_and_every_row_switch():
    assert sorted(EXPECTED) == sorted(c["name"] for c in CASES)
    logged = "".join(EXPECTED.values())
    for name in KERNEL_NAMES:
        assert name in logged, name
    used = {c["tuning"].get(0, 0) for c in CASES}
    assert set(ROW_KEY0) <= used, sorted(set(ROW_KEY0) - used)
    # the dedup entry at the smallest batch that still takes the stream-K kernel, with the switch on and off
    assert "gemm_rows_skc_kernel" in EXPECTED["model_k0_d1"] and "+dedup" in EXPECTED["model_k0_d0"]
    # the asymmetry between the entry points, as recorded
    assert "gemm_rows_n96s_kernel" in EXPECTED["n96_cu_rows"] and "gemm_rows_n96s_kernel" not in EXPECTED["n96_cu_embed"]
