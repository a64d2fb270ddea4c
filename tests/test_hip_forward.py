"""GPU parity of the HIP forward path (through the C ABI) against golden fixtures and the CPU oracle.

Tolerances: BASELINE.json's north_star asks for outputs within 1e-4 (fp32) of the reference; the
kernels are exact-fp32 MFMA, so the tests hold them to 2e-5 on probabilities and 1e-4 (absolute,
on O(1..10) activations) on intermediates.
"""
import numpy as np
import pytest
import torch

from oracle import carca_oracle as O
from tests.golden_util import G1_NAMES, G7_NAMES, load, oracle_config
from tests.model_util import assert_all_users_match_oracle, dev, model_from_fixture, model_from_params

pytestmark = pytest.mark.gpu

Y_ATOL = 2e-5
ACT_ATOL = 1e-4


def _eval_in(fx, prefix=""):
    g = lambda k: fx.ins[prefix + k].cuda()  # noqa: E731
    return (g("p_x"), g("p_a"), g("p_c")), [(g("o_x"), g("o_a"), g("o_c"))]


def _train_in(fx, prefix=""):
    g = lambda k: fx.ins[prefix + k].cuda()  # noqa: E731
    L = fx.ins[prefix + "p_x"].shape[1]
    pos = tuple(g(k)[:, :L].contiguous() for k in ("o_x", "o_a", "o_c"))
    neg = tuple(g(k)[:, L:].contiguous() for k in ("o_x", "o_a", "o_c"))
    return (g("p_x"), g("p_a"), g("p_c")), [pos, neg]


def test_library_loaded_and_native():
    import carca_replication_amd as pkg

    lib = pkg.load()
    assert lib.carca_abi_version() == 3


@pytest.mark.parametrize("name", G1_NAMES)
def test_g1_eval_forward_matches_reference(name):
    fx = load("g1_" + name)
    model = model_from_fixture(fx).eval()
    profile, targets = _eval_in(fx)
    with torch.no_grad():
        y = model(profile=profile, targets=targets)
        trace = {}
        model.forward_nograd(profile, targets, trace=trace)
    assert y.shape == fx.outs["y"].shape
    assert float((y.cpu() - fx.outs["y"]).abs().max()) < Y_ATOL
    for k in ["p_embed", "p_final", "o_embed0"] + [f"block{i}" for i in range(int(fx.cfg["n_blocks"]))]:
        err = float((trace[k].cpu() - fx.outs[k]).abs().max())
        assert err < ACT_ATOL, (k, err)


@pytest.mark.parametrize("name", G1_NAMES)
def test_g2_train_mode_forward_matches_reference(name):
    """train(): two target groups, tril(-1) cross-attention mask (carca.py:339), p = 0."""
    fx = load("g2_" + name)
    model = model_from_fixture(fx).train()
    profile, targets = _train_in(fx)
    with torch.no_grad():
        y = model(profile=profile, targets=targets)
    assert y.shape == fx.outs["y"].shape
    assert float((y.cpu() - fx.outs["y"]).abs().max()) < Y_ATOL


def test_g6_squeeze_quirks():
    fx = load("g6_shapes")
    model = model_from_fixture(fx).eval()
    for tag, key in (("b1/", "y_b1"), ("n1/", "y_n1")):
        profile, targets = _eval_in(fx, tag)
        with torch.no_grad():
            y = model(profile=profile, targets=targets)
        assert tuple(y.shape) == tuple(fx.outs[key].shape)
        assert float((y.cpu() - fx.outs[key]).abs().max()) < Y_ATOL


@pytest.mark.parametrize("name", G7_NAMES)
def test_g7_variants(name):
    fx = load("g7_" + name)
    model = model_from_fixture(fx)
    with torch.no_grad():
        y = model.eval()(*_eval_in(fx))
        yt = model.train()(*_train_in(fx, "train/"))
    assert float((y.cpu() - fx.outs["y"]).abs().max()) < Y_ATOL
    assert float((yt.cpu() - fx.outs["train/y"]).abs().max()) < Y_ATOL


def test_g8_ranking_hr_ndcg_identical():
    """HR@10 / NDCG@10 and every user's rank equal the reference's on the same candidates."""
    from carca_replication_amd import ops

    fx = load("g8_ranking")
    model = model_from_fixture(fx).eval()
    with torch.no_grad():
        y = model(*_eval_in(fx))
    assert float((y.cpu() - fx.outs["y"]).abs().max()) < Y_ATOL
    sums, rank = ops.rank_metrics(y, 10, want_rank=True)
    assert torch.equal(rank.cpu().long(), fx.outs["rank"].long())
    sums = sums.cpu()
    assert float(sums[0]) == float(fx.outs["hr10"])
    assert abs(float(sums[1]) - float(fx.outs["ndcg10"])) < 1e-4
    assert float(sums[2]) == 0.0


def test_g11_ranking_at_c2_model_dims_is_identical():
    """The same at BASELINE config 2's model dimensions (d = 90, g = 450, H = 3, 2 blocks, L = 50, N = 1 + 100, profile
    lengths U{3..L}) with trained weights: every user's rank of the positive, HR@10 and NDCG@10 equal the reference's;
    the folded scoring kernel and the V-materialising one agree on them too."""
    from carca_replication_amd import _lib, ops

    fx = load("g11_ranking_c2dims")
    assert (fx.cfg["d"], fx.cfg["g"], fx.cfg["H"], fx.dim["L"], fx.dim["N"]) == (90, 450, 3, 50, 101)
    model = model_from_fixture(fx).eval()
    lib = _lib.load()
    try:
        for force_materialised in (0, 1):
            lib.carca_set_tuning(6, force_materialised)
            with torch.no_grad():
                y = model(*_eval_in(fx))
            assert float((y.cpu() - fx.outs["y"]).abs().max()) < Y_ATOL
            sums, rank = ops.rank_metrics(y, 10, want_rank=True)
            assert torch.equal(rank.cpu().long(), fx.outs["rank"].long())
            sums = sums.cpu()
            assert float(sums[0]) == float(fx.outs["hr10"]) and float(sums[2]) == 0.0
            assert abs(float(sums[1]) - float(fx.outs["ndcg10"])) < 1e-4
    finally:
        lib.carca_set_tuning(6, 0)


def test_g4_rank_metrics_kernel():
    from carca_replication_amd import ops

    fx = load("g4_metrics")
    scores = fx.ins["scores"].cuda()
    for k in (1, 5, 10, 20):
        sums, _ = ops.rank_metrics(scores, k)
        sums = sums.cpu()
        assert float(sums[0]) == float(fx.outs[f"hr{k}"])
        assert abs(float(sums[1]) - float(fx.outs[f"ndcg{k}"])) < 1e-4


@pytest.mark.parametrize("name", ["d90h3", "d64h2"])
def test_bce_loss_matches_reference(name):
    from carca_replication_amd import modules as M

    fx = load("g1_" + name)
    y = fx.outs["y"].cuda()
    loss = M.BinaryCrossEntropy()(y, fx.ins["y_true"].cuda(), M.get_mask(fx.ins["o_x"].cuda()))
    assert abs(float(loss) - float(fx.outs["loss"])) < 2e-6
    fx2 = load("g2_" + name)
    loss2 = M.BinaryCrossEntropy()(fx2.outs["y"].cuda(), fx2.ins["y_true"].cuda(), M.get_mask(fx2.ins["o_x"].cuda()))
    assert abs(float(loss2) - float(fx2.outs["loss"])) < 2e-6


def test_bce_gradient_uses_the_callers_normaliser():
    """Sharded steps pass the all-reduced mask count as `denom`: loss AND dL/dy must be scaled by it, not by the local
    count (round-1 race: every lane of wave 0 stored its own normaliser, only lane 0 held the caller's)."""
    from carca_replication_amd import ops

    g = torch.Generator().manual_seed(3)
    n = 7 * 100
    y = torch.rand(n, generator=g) * 0.98 + 0.01
    y_true = (torch.rand(n, generator=g) < 0.5).int()
    ids = (torch.rand(n, generator=g) < 0.7).int() * 5
    mask = (ids != 0).float()
    for denom in (None, 3.0 * float(mask.sum()), 17.0):
        yr = y.clone().requires_grad_(True)
        per = -(y_true * torch.log(yr + 1e-8) + (1 - y_true) * torch.log(1 - yr + 1e-8))
        want = (per * mask).sum() / (float(mask.sum()) if denom is None else denom)
        want.backward()
        dt = None if denom is None else torch.tensor([denom], dtype=torch.float32, device="cuda")
        loss, dy = ops.bce_fwd(y.cuda(), y_true.cuda(), ids.cuda(), 1e-8, want_grad=True, denom=dt)
        assert abs(float(loss) - float(want)) < 2e-6 * max(1.0, abs(float(want)))
        assert torch.allclose(dy.cpu().view(-1), yr.grad, rtol=1e-5, atol=1e-9)


# ---- oracle comparisons at shapes the fixtures do not hold ------------------------------------------
SHAPES = [
    # d, H, g, blocks, B, L, N, n_items, n_attrs, n_ctx
    (90, 3, 450, 2, 7, 50, 101, 300, 64, 6),
    (90, 1, 64, 1, 3, 17, 5, 50, 13, 2),
    (128, 2, 96, 1, 5, 33, 40, 80, 21, 3),
    (64, 4, 100, 2, 6, 64, 101, 400, 36, 1),
    (64, 1, 32, 1, 2, 1, 1, 20, 4, 1),
    (48, 2, 40, 1, 3, 9, 20, 60, 8, 2),
]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("training", [False, True])
def test_random_shapes_vs_oracle(shape, training):
    d, H, g, nb, B, L, N, n_items, n_attrs, n_ctx = shape
    cfg = O.CarcaConfig(d=d, H=H, n_blocks=nb)
    P = O.perturb_params(O.init_params(cfg, n_items, g, n_ctx, n_attrs, L, seed=3), seed=4)
    if training:
        N = L
    profile, target, _ = O.synth_eval_batch(B, L, N, n_items, n_attrs, n_ctx, seed=5, min_len=1)
    targets = [target, (target[0].flip(1).contiguous(), target[1].flip(1).contiguous(), target[2])] if training \
        else [target]
    if training:  # make some target slots padding, as the train sampler does (data.py:112-132)
        tx = targets[0][0].clone()
        tx[:, : L // 3] = 0
        targets[0] = (tx, targets[0][1], targets[0][2])
    want = O.carca_forward(P, cfg, profile, targets, training=training)
    model = model_from_params(P, cfg)
    model.train(training)
    with torch.no_grad():
        got = model(profile=dev(profile), targets=[dev(t) for t in targets])
    assert got.shape == want.shape
    assert float((got.cpu() - want).abs().max()) < Y_ATOL


def test_c2_sized_batch_vs_oracle():
    """BASELINE config C2 at full model size (n_attrs=4096, g=450), B=16 users."""
    cfg = O.CarcaConfig(d=90, H=3, n_blocks=2)
    n_items, n_attrs, n_ctx, g, L, N, B = 2000, 4096, 6, 450, 50, 101, 16
    P = O.perturb_params(O.init_params(cfg, n_items, g, n_ctx, n_attrs, L, seed=0), seed=1)
    profile, target, _ = O.synth_eval_batch(B, L, N, n_items, n_attrs, n_ctx, seed=1234)
    want = O.carca_forward(P, cfg, profile, [target], training=False)
    model = model_from_params(P, cfg).eval()
    with torch.no_grad():
        got = model(profile=dev(profile), targets=[dev(target)])
    assert float((got.cpu() - want).abs().max()) < Y_ATOL
    assert torch.equal(O.positive_rank(got.cpu()), O.positive_rank(want))


def test_cpu_tensors_fail_loudly():
    from carca_replication_amd import CarcaHipError

    fx = load("g1_d90h2")
    model = model_from_fixture(fx, device="cpu").eval()
    g = lambda k: fx.ins[k]  # noqa: E731
    with pytest.raises(CarcaHipError):
        with torch.no_grad():
            model(profile=(g("p_x"), g("p_a"), g("p_c")), targets=[(g("o_x"), g("o_a"), g("o_c"))])


def test_unsupported_shape_is_an_error_not_a_fallback():
    from carca_replication_amd import CarcaHipError

    # (d > 128 runs the composed path since round 5: tests/test_hip_long_profile.py; what stays an error is a profile of more
    # than 1024 slots -- carca_mha_core keeps a query's weights in registers)
    cfg = O.CarcaConfig(d=32, H=2, n_blocks=1)
    P = O.init_params(cfg, 1200, 16, 1, 4, 1030, seed=0)
    profile, target, _ = O.synth_eval_batch(2, 1030, 4, 1200, 4, 1, seed=2)
    model = model_from_params(P, cfg).eval()
    with pytest.raises(CarcaHipError, match="1024"):
        with torch.no_grad():
            model(profile=dev(profile), targets=[dev(target)])


def test_attr_table_gather_equals_dense_batch():
    """register_attr_table: ids-only batches (a = None) give the same scores and gradients as dense attrs."""
    from carca_replication_amd import modules as M

    cfg = O.CarcaConfig(d=90, H=3, n_blocks=1)
    n_items, n_attrs, n_ctx, g, L, N, B = 300, 72, 5, 130, 50, 101, 6
    P = O.perturb_params(O.init_params(cfg, n_items, g, n_ctx, n_attrs, L, seed=0), seed=1)
    profile, target, table = O.synth_eval_batch(B, L, N, n_items, n_attrs, n_ctx, seed=9)
    model = model_from_params(P, cfg).eval()
    with torch.no_grad():
        dense = model(profile=dev(profile), targets=[dev(target)])
    model.embeds.register_attr_table(table.cuda())
    with torch.no_grad():
        gathered = model(profile=(profile[0].cuda(), None, profile[2].cuda()),
                         targets=[(target[0].cuda(), None, target[2].cuda())])
    assert torch.equal(dense, gathered)  # same kernel, same rows, same order of operations
    # training step through the gathered path
    pos = (target[0][:, :L].contiguous(), None, target[2][:, :L].contiguous())
    neg = (target[0][:, L:2 * L].contiguous(), None, target[2][:, L:2 * L].contiguous())
    y_true = torch.cat([torch.ones(B, L), torch.zeros(B, L)], 1).int().cuda()
    o_x = torch.cat([pos[0], neg[0]], 1).cuda()
    model.train()
    grads = []
    for use_table in (True, False):
        model.zero_grad()
        if use_table:
            tg = [(pos[0].cuda(), None, pos[2].cuda()), (neg[0].cuda(), None, neg[2].cuda())]
            pf = (profile[0].cuda(), None, profile[2].cuda())
        else:
            model.embeds.register_attr_table(None)
            tg = [(pos[0].cuda(), table[pos[0]].cuda(), pos[2].cuda()), (neg[0].cuda(), table[neg[0]].cuda(), neg[2].cuda())]
            pf = dev(profile)
        y = model(profile=pf, targets=tg)
        M.BinaryCrossEntropy()(y, y_true, M.get_mask(o_x)).backward()
        grads.append({n: p.grad.clone() for n, p in model.named_parameters()})
    for n in grads[0]:
        ref = grads[1][n]
        assert float((grads[0][n] - ref).abs().max()) <= 1e-4 * float(ref.abs().max()) + 1e-7, n


@pytest.mark.parametrize("case", [
    # BASELINE.json configs beyond C2, at their model shapes (n_attrs kept small so the CPU oracle stays fast)
    dict(name="C3-like B=512", d=90, H=3, g=450, nb=2, B=512, L=50, N=101, n_items=3000, n_attrs=48, n_ctx=6),
    dict(name="C4 shape d=128 g=640 H=4", d=128, H=4, g=640, nb=2, B=32, L=50, N=101, n_items=200000, n_attrs=64, n_ctx=6),
    dict(name="C5 1000-negative ranking", d=90, H=3, g=450, nb=2, B=8, L=50, N=1001, n_items=5000, n_attrs=64, n_ctx=6),
])
def test_baseline_config_shapes(case):
    c = case
    cfg = O.CarcaConfig(d=c["d"], H=c["H"], n_blocks=c["nb"])
    P = O.perturb_params(O.init_params(cfg, c["n_items"], c["g"], c["n_ctx"], c["n_attrs"], c["L"], seed=0), seed=1)
    profile, target, _ = O.synth_eval_batch(c["B"], c["L"], c["N"], c["n_items"], c["n_attrs"], c["n_ctx"], seed=21)
    want = O.carca_forward(P, cfg, profile, [target], training=False)
    model = model_from_params(P, cfg).eval()
    with torch.no_grad():
        got = model(profile=dev(profile), targets=[dev(target)])
    assert got.shape == want.shape
    assert float((got.cpu() - want).abs().max()) < Y_ATOL
    # Ranks: a random-init model scores many candidates within 1e-6 of each other, so a rank is only defined
    # up to those near-ties (the reference's own unstable sort has the same freedom): the kernel's
    # rank must lie between the oracle's ranks computed with the positive moved by -/+ the output tolerance.
    from carca_replication_amd import ops

    _, rank = ops.rank_metrics(got, 10, want_rank=True)
    rank = rank.cpu().long()
    lo = (want[:, 1:] > want[:, :1] + 2 * Y_ATOL).sum(1)
    hi = (want[:, 1:] > want[:, :1] - 2 * Y_ATOL).sum(1)
    assert bool(((rank >= lo) & (rank <= hi)).all())
    clear = lo == hi  # users whose rank is unambiguous
    assert torch.equal(rank[clear], O.positive_rank(want)[clear])


def test_folded_embedding_matches_oracle():
    """CARCA.fold_embedding(True): composed W_jq W_f path (inference shortcut) stays within the output tolerance."""
    cfg = O.CarcaConfig(d=90, H=3, n_blocks=2, encoding="learnable")
    n_items, n_attrs, n_ctx, g, L, N, B = 400, 300, 6, 450, 50, 101, 12
    P = O.perturb_params(O.init_params(cfg, n_items, g, n_ctx, n_attrs, L, seed=0), seed=1)
    profile, target, table = O.synth_eval_batch(B, L, N, n_items, n_attrs, n_ctx, seed=5)
    want = O.carca_forward(P, cfg, profile, [target], training=False)
    model = model_from_params(P, cfg).eval()
    model.fold_embedding(True)
    with torch.no_grad():
        got = model(profile=dev(profile), targets=[dev(target)])
        assert float((got.cpu() - want).abs().max()) < Y_ATOL
        # weights change -> the composed matrix is rebuilt
        model.embeds.feats_embed.weight.mul_(0.5)
        got2 = model(profile=dev(profile), targets=[dev(target)])
        P2 = dict(P)
        P2["embeds.feats_embed.weight"] = P["embeds.feats_embed.weight"] * 0.5
        want2 = O.carca_forward(P2, cfg, profile, [target], training=False)
        assert float((got2.cpu() - want2).abs().max()) < Y_ATOL
        # with the attribute table resident as well
        model.embeds.register_attr_table(table.cuda())
        got3 = model(profile=(profile[0].cuda(), None, profile[2].cuda()), targets=[(target[0].cuda(), None, target[2].cuda())])
        assert float((got3.cpu() - want2).abs().max()) < Y_ATOL
    model.fold_embedding(False)


def test_two_workgroups_per_user_is_bitwise_the_same():
    """Tuning key 1 (1 = one workgroup per user, 2 = two, 3 = one 8-wave workgroup in the scoring kernel): the variants
    only move rows / target tiles between workgroups and waves."""
    from carca_replication_amd import _lib

    cfg = O.CarcaConfig(d=90, H=3, n_blocks=2, encoding="learnable")
    n_items, n_attrs, n_ctx, g, L, N, B = 300, 200, 6, 450, 50, 101, 5
    P = O.perturb_params(O.init_params(cfg, n_items, g, n_ctx, n_attrs, L, seed=0), seed=1)
    profile, target, _ = O.synth_eval_batch(B, L, N, n_items, n_attrs, n_ctx, seed=7)
    model = model_from_params(P, cfg).eval()
    lib = _lib.load()
    outs = {}
    try:
        for tune in (1, 2, 3):
            lib.carca_set_tuning(1, tune)
            with torch.no_grad():
                outs[tune] = model(profile=dev(profile), targets=[dev(target)]).cpu()
    finally:
        lib.carca_set_tuning(1, 0)
    # one vs two 16-wave workgroups: the same instruction stream per tile, bit for bit.  The 8-wave workgroups compute the
    # folded value u = p . wu + cu as an MFMA tile, the 16-wave ones as four partial sums on the VALU: last bits only.
    assert torch.equal(outs[1], outs[2]) and float((outs[1] - outs[3]).abs().max()) < 5e-7
    want = O.carca_forward(P, cfg, profile, [target], training=False)
    assert float((outs[2] - want).abs().max()) < Y_ATOL


def test_big_batch_scoring_variant_is_bitwise_the_same():
    """B > #CUs takes the persistent, user-pipelined scoring kernel (csrc/cross_stream.hip) by itself: the 16-wave
    per-user workgroups' results (tuning key 1 = 1) up to the summation order of the final LayerNorm's row sums and of the
    folded value u, the 8-wave per-user workgroups' (key 7 = 2) likewise, and the oracle's numbers."""
    from carca_replication_amd import _lib

    cfg = O.CarcaConfig(d=90, H=3, n_blocks=1, encoding="learnable")
    n_items, n_attrs, n_ctx, g, L, N, B = 200, 24, 3, 64, 50, 37, 530
    P = O.perturb_params(O.init_params(cfg, n_items, g, n_ctx, n_attrs, L, seed=0), seed=1)
    profile, target, _ = O.synth_eval_batch(B, L, N, n_items, n_attrs, n_ctx, seed=11)
    model = model_from_params(P, cfg).eval()
    lib = _lib.load()
    outs = {}
    try:
        for tune in (0, 1):
            lib.carca_set_tuning(1, tune)
            with torch.no_grad():
                outs[tune] = model(profile=dev(profile), targets=[dev(target)]).cpu()
        lib.carca_set_tuning(1, 0)
        lib.carca_set_tuning(7, 2)
        with torch.no_grad():
            outs[2] = model(profile=dev(profile), targets=[dev(target)]).cpu()
    finally:
        lib.carca_set_tuning(1, 0)
        lib.carca_set_tuning(7, 0)
    assert float((outs[0] - outs[1]).abs().max()) < 1e-6 and float((outs[0] - outs[2]).abs().max()) < 1e-6
    want = O.carca_forward(P, cfg, profile, [target], training=False)
    assert float((outs[0] - want).abs().max()) < Y_ATOL


@pytest.mark.parametrize("d,H,g", [(90, 3, 450), (128, 4, 640)], ids=["C2", "C4-dims"])
def test_c2_full_batch_is_batch_split_invariant(d, H, g):
    """(C4-dims: d = 128, g = 640, H = 4 at the same batch -- the 384 x 128 tiles of the one-block-per-CU kernel.)
    The bench's exact workload (C2: B = 128 users, n_items = 12102, n_attrs = 4096; one-block-per-CU feature GEMM with
    the gather riding along, two workgroups per user) through a size-independent property: a user's scores do not depend
    on who else is in the batch.  The same users in eight batches of 16 take different kernels (tiled feature GEMM, its
    own gather launch) whose B = 16 results are pinned against the oracle above; EVERY user of the full batch is checked
    against the oracle here as well (2e-5, ranks wherever they are unambiguous)."""
    cfg = O.CarcaConfig(d=d, H=H, n_blocks=2)
    n_items, n_attrs, n_ctx, L, N, B = 12102, 4096, 6, 50, 101, 128
    P = O.perturb_params(O.init_params(cfg, n_items, g, n_ctx, n_attrs, L, seed=0), seed=1)
    profile, target, _ = O.synth_eval_batch(B, L, N, n_items, n_attrs, n_ctx, seed=1234)
    model = model_from_params(P, cfg).eval()
    p_dev, t_dev = dev(profile), dev(target)
    with torch.no_grad():
        full = model(profile=p_dev, targets=[t_dev]).cpu()
        parts = [model(profile=tuple(t[i:i + 16] for t in p_dev), targets=[tuple(t[i:i + 16] for t in t_dev)]).cpu()
                 for i in range(0, B, 16)]
    split = torch.cat(parts, dim=0)
    assert full.shape == split.shape == (B, N)
    assert float((full - split).abs().max()) < 2e-5
    # ALL 128 users against the oracle (0.1-0.2 s on the box's cores), not a sample: the compacting feature GEMM, the joint
    # GEMM, both SA blocks and the scoring kernel at the bench's exact shape ("What's weak" 1)
    want = O.carca_forward(P, cfg, profile, [target], training=False)
    assert_all_users_match_oracle(full, want, 2e-5)


# ---- the stand-alone module surface of the ABCs (abstract.py:31, carca.py:25-31, 54-60, 228-265) -----------------------
@pytest.mark.parametrize("name", ["d90h3", "d64h2"])
def test_standalone_mha_returns_the_references_decoder_weights(name):
    """MultiHeadAttention.forward(..., return_w=True) on its own: the weights equal fixture G1's `dec_w0` (captured from
    the reference's decoder.attn with return_w=True, carca.py:262-263) and the output equals the oracle's."""
    fx = load("g1_" + name)
    model = model_from_fixture(fx).eval()
    o_e, p_e = fx.outs["o_embed0"].cuda(), fx.outs["p_final"].cuda()
    o_mask, p_mask = (fx.ins["o_x"] != 0).float().cuda(), fx.outs["p_mask"].cuda()
    with torch.no_grad():
        w, out = model.decoder.attn(o_e, p_e, p_e, q_mask=o_mask, k_mask=p_mask, causal=None, return_w=True)
        out_only = model.decoder.attn(o_e, p_e, p_e, q_mask=o_mask, k_mask=p_mask)
    B, H = o_e.shape[0], model.decoder.attn.H
    assert w.shape == (H * B, o_e.shape[1], p_e.shape[1])  # head-major, head h of user b at h*B + b (carca.py:242-244)
    got = torch.stack(torch.split(w, B, dim=0), dim=1).cpu()
    assert float((got - fx.outs["dec_w0"]).abs().max()) < 2e-6
    P = {k: v for k, v in fx.params.items()}
    w_o, out_o = O.mha(P, "decoder.attn.", H, fx.outs["o_embed0"], fx.outs["p_final"], fx.outs["p_final"],
                       (fx.ins["o_x"] != 0).float(), fx.outs["p_mask"], None)
    assert float((out.cpu() - out_o).abs().max()) < 1e-5 and torch.equal(out, out_only)
    # causal variants (what the blocks pass: 0 in SelfAttentionBlock, -1 in the training decoder)
    L = p_e.shape[1]
    with torch.no_grad():
        for causal in (0, -1):
            wc, oc = model.encoder[0].attn(p_e, p_e, p_e, q_mask=p_mask, k_mask=p_mask, causal=causal, return_w=True)
            w_r, o_r = O.mha(P, "encoder.0.attn.", H, fx.outs["p_final"], fx.outs["p_final"], fx.outs["p_final"],
                             fx.outs["p_mask"], fx.outs["p_mask"], causal)
            assert float((torch.stack(torch.split(wc, B, dim=0), dim=1).cpu() - w_r).abs().max()) < 2e-6
            assert float((oc.cpu() - o_r).abs().max()) < 1e-5
    assert L == fx.dim["L"]


def test_standalone_encodings_add_their_table():
    """Encoding.forward(x) (abstract.py:31): Identity returns x, Learnable / Positional add their first T rows."""
    from carca_replication_amd import CarcaHipError
    from carca_replication_amd import modules as M

    torch.manual_seed(0)
    x = torch.randn(3, 7, 10, device="cuda")
    assert M.IdentityEncoding()(x) is x
    le = M.LearnableEncoding(10, 9).cuda()
    pe = M.PositionalEncoding(10, 9).cuda()
    with torch.no_grad():
        assert torch.equal(le(x), x + le.encoding.weight[:7])
        assert torch.equal(pe(x), x + pe.pe[:, :7])
        view = torch.randn(3, 7, 16, device="cuda")[..., :10]  # rows of a padded buffer
        assert torch.equal(pe(view), view + pe.pe[:, :7])
        with pytest.raises(CarcaHipError):
            le(torch.randn(3, 12, 10, device="cuda"))  # longer than max_len
    # with gradients enabled the same call is differentiable (tests/test_hip_standalone_grad.py)
    y = le(x)
    assert y.requires_grad and torch.equal(y.detach(), x + le.encoding.weight[:7].detach())


# ---- the eval-mode SelfAttentionBlock kernel (csrc/sa_eval.hip) ----------------------------------------------------------
@pytest.mark.parametrize("d,H,L", [(90, 3, 50), (64, 2, 20), (128, 4, 64), (90, 1, 33), (64, 4, 7)])
def test_sa_eval_kernel_equals_oracle_and_training_kernel(d, H, L):
    """Every row of a block's output -- real slots, pads inside the profile, leading pads -- against the oracle's
    sa_block and against the training kernel (tuning key 6 = 1), with and without the pads_uniform promise, one and two
    workgroups per user; profile lengths from 0 (all pad) to L, pads inside the kept range, B beyond one tile of users."""
    from carca_replication_amd import _lib, ops
    from carca_replication_amd import modules as M

    torch.manual_seed(d + H + L)
    B = 11
    blk = M.SelfAttentionBlock(d, H, 0.0, True).cuda().eval()
    with torch.no_grad():
        for p_ in blk.parameters():
            if p_.dim() == 1:
                p_.add_(0.1 * torch.randn_like(p_))
    dpi, _, _ = ops.padded_dims(d, H)
    g = torch.Generator().manual_seed(1)
    lens = torch.tensor([0, 1, 2, L, L, L - 1, 17 % (L + 1), 16 % (L + 1), 15 % (L + 1), 33 % (L + 1), 5 % (L + 1)])
    ids = (torch.arange(L)[None, :] >= (L - lens)[:, None]).int() * 3
    ids[4, L // 2] = 0  # a pad inside a full profile
    if L > 4:
        ids[6, L - 2] = 0
    x = torch.zeros(B, L, dpi)
    x[..., :d] = torch.randn(B, L, d, generator=g)
    # leading pad rows equal within a user (what the masked embedding / an upstream block produce), other rows arbitrary
    lead = (torch.cumsum(ids != 0, dim=1) == 0)
    padrow = torch.zeros(B, 1, dpi)
    padrow[..., :d] = torch.randn(B, 1, d, generator=g)
    x = torch.where(lead[..., None], padrow.expand(B, L, dpi), x)
    P = {"encoder.0." + k: v.detach().cpu() for k, v in blk.state_dict().items()}
    cfg = O.CarcaConfig(d=d, H=H, n_blocks=1)
    want = O.sa_block(P, cfg, 0, x[..., :d], (ids != 0).float())
    lib = _lib.load()
    outs = {}
    try:
        for name, tune6, tune1, uniform in (("train-kernel", 1, 0, False), ("eval", 0, 1, False), ("eval-uniform", 0, 1, True),
                                            ("eval-2wg", 0, 2, False), ("eval-2wg-uniform", 0, 2, True)):
            lib.carca_set_tuning(6, tune6)
            lib.carca_set_tuning(1, tune1)
            with torch.no_grad():
                y = ops.sa_block_fwd(x.cuda(), ids.cuda(), blk.weights_struct(torch.device("cuda")), d, H, True,
                                     pads_uniform=uniform)
            outs[name] = y.cpu()
            assert float(y[..., d:].abs().max()) == 0.0 if dpi > d else True
            err = float((y.cpu()[..., :d] - want).abs().max())
            assert err < ACT_ATOL, (name, err)
    finally:
        lib.carca_set_tuning(6, 0)
        lib.carca_set_tuning(1, 0)
    assert torch.equal(outs["eval"], outs["eval-2wg"])                   # the split only moves tiles between workgroups
    assert torch.equal(outs["eval-uniform"], outs["eval-2wg-uniform"])
    assert float((outs["eval"] - outs["eval-uniform"]).abs().max()) < 1e-6   # (re-based rows: other tile / lane, same sums)


@pytest.mark.parametrize("B,L,N,enc", [(40, 50, 101, "learnable"), (33, 50, 37, "identity"), (7, 23, 5, "positional")])
def test_one_block_per_cu_joint_gemm_equals_the_tiled_one(B, L, N, enc):
    """The 80 x 96 row GEMM (gemm_rows_n96_kernel: narrow output over one k-source -- AllEmbedding.joint_embed,
    carca.py:89, with its positional rows, bias and padding mask in the epilogue) forced on (tuning key 0 = 11) against
    the 128 x 32 blocks (12), at row counts that are no multiple of its tile and a K (d + g = 540) that is no multiple of
    its stage; then the oracle."""
    from carca_replication_amd import _lib

    cfg = O.CarcaConfig(d=90, H=3, n_blocks=1, encoding=enc)
    n_items, n_attrs, n_ctx, g = 300, 40, 6, 450
    P = O.perturb_params(O.init_params(cfg, n_items, g, n_ctx, n_attrs, L, seed=0), seed=1)
    profile, target, _ = O.synth_eval_batch(B, L, N, n_items, n_attrs, n_ctx, seed=B)
    model = model_from_params(P, cfg).eval()
    lib = _lib.load()
    outs = {}
    try:
        for variant in (11, 12):
            lib.carca_set_tuning(0, variant)
            with torch.no_grad():
                outs[variant] = model(profile=dev(profile), targets=[dev(target)]).cpu()
    finally:
        lib.carca_set_tuning(0, 0)
    assert float((outs[11] - outs[12]).abs().max()) < 2e-6
    want = O.carca_forward(P, cfg, profile, [target], training=False)
    assert float((outs[11] - want).abs().max()) < Y_ATOL


# ---- the persistent, user-pipelined scoring kernel (csrc/cross_stream.hip) --------------------------------------------------
@pytest.mark.parametrize("d,H,L,Ns,B,lengths", [
    (90, 3, 50, [101], 300, "uniform"), (90, 3, 50, [101], 261, "holes"), (90, 3, 50, [101], 5, "holes"),
    (90, 3, 50, [1], 270, "holes"), (90, 3, 50, [17], 270, "uniform"), (90, 3, 50, [300], 260, "holes"),
    (90, 3, 50, [5, 130, 33], 270, "holes"), (90, 2, 50, [50, 50], 300, "holes"), (90, 1, 33, [101], 280, "holes"),
    (64, 2, 50, [101], 300, "holes"), (64, 4, 7, [40], 300, "holes"), (64, 1, 64, [20], 300, "full"),
    (96, 3, 64, [129], 300, "holes"),
    # every profile with a NEARLY EMPTY last slot tile (1..4 slots: its K rows are computed on the VALU, csrc/cross_stream.hip)
    (90, 3, 50, [101], 300, "full"), (90, 3, 49, [101], 270, "full"), (64, 2, 36, [40], 300, "full"),
    (90, 3, 4, [33], 280, "full"), (64, 4, 20, [101], 300, "full"), (96, 3, 35, [50], 300, "full")])
def test_stream_scoring_kernel_equals_oracle_and_per_user_kernels(d, H, L, Ns, B, lengths):
    """cross_stream_kernel (what B > #CUs launches in eval mode; forced here with tuning key 7 = 3 at any B) against the
    oracle's final norm + cross_block and against the two per-user kernels (folded: key 7 = 2, V-materialising: key 6 = 1):
    several rounds of target tiles (N = 300), several groups, one-target groups, pads inside profiles, all-pad users,
    batches that leave some workgroups one user more than others, every head layout with an instantiation."""
    from carca_replication_amd import _lib, ops
    from tests.model_util import build_model

    torch.manual_seed(d * 7 + H + L)
    model = build_model(dict(d=d, H=H, n_blocks=1), 50, 16, 2, 8, L).eval().cuda()
    with torch.no_grad():
        for p_ in model.parameters():
            if p_.dim() == 1:
                p_.add_(0.1 * torch.randn_like(p_))
    dpi, _, _ = ops.padded_dims(d, H)
    cw = model.decoder.weights_struct(torch.device("cuda"), model.norm)
    g = torch.Generator().manual_seed(B)
    x = torch.zeros(B, L, dpi)
    x[..., :d] = torch.randn(B, L, d, generator=g)
    ln = torch.full((B,), L) if lengths == "full" else torch.randint(min(3, L), L + 1, (B,), generator=g)
    p_ids = (torch.arange(L)[None, :] >= (L - ln)[:, None]).int() * 7
    if lengths == "holes":
        p_ids = p_ids * (torch.rand(B, L, generator=g) > 0.2).int()
        p_ids[0] = 0
        p_ids[B // 2] = 0
    groups = []
    for N in Ns:
        o = torch.zeros(B, N, dpi)
        o[..., :d] = torch.randn(B, N, d, generator=g)
        o_ids = torch.randint(1, 5, (B, N), generator=g).int()
        o_ids[:, -1] = 0
        groups.append((o, o_ids))
    lib = _lib.load()
    outs = {}
    try:
        for name, t7, t6 in (("stream", 3, 0), ("fold", 2, 0), ("mat", 2, 1)):
            lib.carca_set_tuning(7, t7)
            lib.carca_set_tuning(6, t6)
            with torch.no_grad():
                ys, _ = ops.cross_score_fwd(x.cuda(), p_ids.cuda(), [(o.cuda(), i.cuda()) for o, i in groups], cw, d, H, True,
                                            False)
            outs[name] = [y.cpu() for y in ys]
    finally:
        lib.carca_set_tuning(7, 0)
        lib.carca_set_tuning(6, 0)
    P = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    cfg = O.CarcaConfig(d=d, H=H, n_blocks=1)
    nu = min(B, 24)  # the oracle on the first users (they include an all-pad profile), the kernels on all of them
    p_mask = (p_ids[:nu] != 0).float()
    pn = O.layer_norm(x[:nu, :, :d], P["norm.weight"], P["norm.bias"])
    for gi, (o, o_ids) in enumerate(groups):
        want = O.cross_block(P, cfg, o[:nu, :, :d], (o_ids[:nu] != 0).float(), pn, p_mask, training=False).reshape(nu, -1)
        assert float((outs["stream"][gi][:nu] - want).abs().max()) < Y_ATOL
        assert bool(torch.isfinite(outs["stream"][gi]).all())
        assert float((outs["stream"][gi] - outs["fold"][gi]).abs().max()) < 2e-6
        assert float((outs["stream"][gi] - outs["mat"][gi]).abs().max()) < 2e-6


def test_stream_k_feature_gemm_hands_over_fresh_partials():
    """gemm_rows_sk_kernel (C2's feature GEMM): the last column block's workgroup computes the last K steps of its four
    neighbours' tiles and hands them over through memory (agent-scope stores, a flag, plain loads on the taker's side --
    which rely on every launch starting with an invalidated L2).  Alternating two DIFFERENT batches through the same
    two-slot ring must give, every time, what the one-tile-per-workgroup kernel (tuning variant 15) gives for that batch:
    a stale partial (5 % of the K sum, from another batch) would show at 1e-2; the two kernels group the K sum
    differently, so they agree to round-off, not bitwise."""
    from carca_replication_amd import _lib

    cfg = O.CarcaConfig(d=90, H=3, n_blocks=1)
    n_items, n_attrs, n_ctx, g, L, N, B = 3000, 4096, 6, 450, 50, 101, 128
    P = O.perturb_params(O.init_params(cfg, n_items, g, n_ctx, n_attrs, L, seed=0), seed=1)
    model = model_from_params(P, cfg).eval()
    batches = []
    for seed in (11, 12):
        profile, target, _ = O.synth_eval_batch(B, L, N, n_items, n_attrs, n_ctx, seed=seed)
        batches.append((dev(profile), dev(target)))
    lib = _lib.load()
    with torch.no_grad():
        lib.carca_set_tuning(0, 15)
        try:
            want = [model(profile=p, targets=[t]).clone() for p, t in batches]
        finally:
            lib.carca_set_tuning(0, 0)
        assert float((want[0] - want[1]).abs().max()) > 1e-2  # (the batches really differ)
        for it in range(8):
            p, t = batches[it % 2]
            got = model(profile=p, targets=[t])
            assert float((got - want[it % 2]).abs().max()) < 2e-5, it
    # and the embedding itself (q = [a ; c] W_f^T + b_f, every column incl. the two VALU ones) against the oracle
    profile, target, _ = O.synth_eval_batch(B, L, N, n_items, n_attrs, n_ctx, seed=11)
    trace = {}
    with torch.no_grad():
        model.forward_nograd(dev(profile), [dev(target)], trace=trace)
    p_x, p_a, p_c = profile
    want_e = O.embedding(P, cfg, p_x[:4].long(), p_a[:4], p_c[:4], (p_x[:4] != 0).float(), False)
    assert float((trace["p_embed"][:4].cpu() - want_e).abs().max()) < 2e-5


@pytest.mark.parametrize("B,N", [(128, 101), (7, 21), (16, 1001), (1, 2)])
def test_eval_metrics_in_one_launch_equals_the_separate_kernels(B, N):
    """carca_eval_metrics (HR@k, NDCG@k, ties, masked-mean BCE loss, user count of one evaluation batch in one launch,
    train.py:45-51) against carca_rank_metrics + carca_bce_fwd, and the loss against the oracle's."""
    from carca_replication_amd import ops

    g = torch.Generator().manual_seed(B * 1000 + N)
    y = torch.rand(B, N, generator=g).clamp(1e-4, 1 - 1e-4)
    y[B // 2, 1] = y[B // 2, 0]  # a tie
    ids = torch.randint(0, 50, (B, N), generator=g).int()
    ids[:, 0] = 7
    y_true = torch.zeros(B, N, dtype=torch.int32)
    y_true[:, 0] = 1
    yd, idd, ytd = y.cuda(), ids.cuda(), y_true.cuda()
    sums = torch.zeros(5, device="cuda")
    sums[0] = 3.0  # (accumulated into)
    ops.eval_metrics(yd, ytd, idd, 10, sums)
    ref, _ = ops.rank_metrics(yd, 10)
    loss, _ = ops.bce_fwd(yd, ytd, idd, 1e-8)
    assert float(sums[0]) == 3.0 + float(ref[0]) and float(sums[2]) == float(ref[2]) >= 1.0
    assert abs(float(sums[1]) - float(ref[1])) <= 1e-5 * max(1.0, float(ref[1]))
    assert float(sums[3]) == float(loss) and float(sums[4]) == B
    want = O.bce_loss(y, y_true, (ids != 0).float())
    assert abs(float(sums[3]) - float(want)) < 2e-6


@pytest.mark.parametrize("d,H,g,B", [(90, 3, 450, 128), (128, 4, 640, 128), (64, 2, 256, 8), (90, 3, 450, 7)])
def test_projected_item_table_equals_the_gathered_item_rows(d, H, g, B, monkeypatch):
    """Inference takes the joint embedding's item term from AllEmbedding.z_table() = sqrt(d) E W_jz^T (one row per ITEM,
    cached per weight version) and runs the product over q's g columns only (K = 450: no multiple of 4, rows 8-byte
    aligned -- the one-block-per-CU kernel's ragged last stage at B = 128, the tiled kernels below): same scores as the
    reference's order (gather E[x] sqrt(d), one product over d + g columns, carca.py:87-89) to round-off, the oracle's to
    2e-5, and a weight update invalidates the table."""
    from carca_replication_amd import modules as M

    cfg = O.CarcaConfig(d=d, H=H, n_blocks=2, encoding="learnable")
    n_items, n_attrs, n_ctx, L, N = 700, 96, 6, 50, 101
    P = O.perturb_params(O.init_params(cfg, n_items, g, n_ctx, n_attrs, L, seed=0), seed=1)
    profile, target, _ = O.synth_eval_batch(B, L, N, n_items, n_attrs, n_ctx, seed=5)
    model = model_from_params(P, cfg).eval()
    p_dev, t_dev = dev(profile), dev(target)
    with torch.no_grad():
        got = model(profile=p_dev, targets=[t_dev])
        assert model.embeds.__dict__.get("_ztab_cache") is not None  # (the table path was taken)
        monkeypatch.setattr(M, "USE_Z_TABLE", False)
        ref = model(profile=p_dev, targets=[t_dev])
        monkeypatch.setattr(M, "USE_Z_TABLE", True)
        assert float((got - ref).abs().max()) < 2e-6
        want = O.carca_forward(P, cfg, profile, [target], training=False)
        assert_all_users_match_oracle(got, want, 2e-5)
        # another weight version: items_embed and joint_embed move, the cached table must not survive
        model.embeds.items_embed.weight.mul_(1.25)
        model.embeds.joint_embed.weight[:, :d].mul_(0.5)
        M.note_training_forward()
        P2 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        got2 = model(profile=p_dev, targets=[t_dev])
        want2 = O.carca_forward(P2, cfg, profile, [target], training=False)
        assert float((got2 - got).abs().max()) > 1e-3
        assert_all_users_match_oracle(got2, want2, 2e-5)
