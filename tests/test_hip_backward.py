"""GPU parity of the HIP backward pass: parameter gradients of one train-mode step (p = 0) against the
reference's own loss.backward() (fixture G2/G7) and against torch.autograd over the CPU oracle.

Tolerance: the reference's fp32 gradients themselves carry ~1e-6 relative noise (sum order); the
weight-gradient kernels combine row splits with fp32 atomics.  Each gradient tensor must agree to
1e-4 of its own largest entry (+1e-7 absolute for tensors whose true gradient is 0, e.g. key biases).
"""
import pytest
import torch

from oracle import carca_oracle as O
from tests.golden_util import G1_NAMES, G7_NAMES, G9_NAMES, load
from tests.model_util import dev, model_from_fixture, model_from_params

pytestmark = pytest.mark.gpu


def _train_in(fx, prefix=""):
    g = lambda k: fx.ins[prefix + k].cuda()  # noqa: E731
    L = fx.ins[prefix + "p_x"].shape[1]
    # exactly what train.py:86-88 builds: torch.split views of the 2L-wide target tensors
    pos = tuple(torch.split(g(k), L, dim=1)[0] for k in ("o_x", "o_a", "o_c"))
    neg = tuple(torch.split(g(k), L, dim=1)[1] for k in ("o_x", "o_a", "o_c"))
    return (g("p_x"), g("p_a"), g("p_c")), [pos, neg]


def _check_grads(model, ref_grads, rtol=1e-4):
    bad = []
    for name, prm in model.named_parameters():
        ref = ref_grads[name]
        got = prm.grad
        assert got is not None, name
        scale = float(ref.abs().max())
        err = float((got.cpu() - ref).abs().max())
        if err > rtol * scale + 1e-7:
            bad.append((name, err, scale))
    assert not bad, bad


def _step(model, fx, in_prefix=""):
    from carca_replication_amd import modules as M

    model.train()
    model.zero_grad()
    profile, targets = _train_in(fx, in_prefix)
    y = model(profile=profile, targets=targets)
    o_x = fx.ins[in_prefix + "o_x"].cuda()
    loss = M.BinaryCrossEntropy()(y, fx.ins[in_prefix + "y_true"].cuda(), M.get_mask(o_x))
    loss.backward()
    return y, loss


@pytest.fixture(params=[0, 1, 3], ids=["shared-users", "one-workgroup-per-user", "eight-wave-scoring-workgroups"])
def attn_variant(request):
    """The attention kernels (forward and backward) give a user to two workgroups while users <= CUs / 2 -- which every
    fixture-sized batch satisfies -- and to one otherwise (tuning key 1 = 1 forces that path, what B > 128 takes; 3 forces
    the scoring kernel's 8-wave workgroups, what B >= 512 takes)."""
    from carca_replication_amd import _lib

    lib = _lib.load()
    lib.carca_set_tuning(1, request.param)
    yield request.param
    lib.carca_set_tuning(1, 0)


@pytest.mark.parametrize("name", G1_NAMES)
def test_g2_gradients_match_reference(name, attn_variant):
    fx = load("g2_" + name)
    model = model_from_fixture(fx)
    y, loss = _step(model, fx)
    assert float((y.detach().cpu() - fx.outs["y"]).abs().max()) < 2e-5
    assert abs(float(loss) - float(fx.outs["loss"])) < 2e-6
    _check_grads(model, {k[len("grad/"):]: v for k, v in fx.outs.items() if k.startswith("grad/")})


@pytest.mark.parametrize("name", G1_NAMES)
def test_g2_gradients_match_reference_with_the_two_stream_backward(name, monkeypatch):
    from carca_replication_amd import autograd

    monkeypatch.setattr(autograd, "SPLIT_EMBED_BWD", True)
    monkeypatch.setattr(autograd, "SPLIT_MAIN_TARGET_USERS", 0.5)
    fx = load("g2_" + name)
    model = model_from_fixture(fx)
    _step(model, fx)
    _check_grads(model, {k[len("grad/"):]: v for k, v in fx.outs.items() if k.startswith("grad/")})


@pytest.mark.parametrize("name", G7_NAMES)
def test_g7_variant_gradients(name):
    fx = load("g7_" + name)
    model = model_from_fixture(fx)
    _step(model, fx, "train/")
    _check_grads(model, {k[len("train/grad/"):]: v for k, v in fx.outs.items() if k.startswith("train/grad/")})


@pytest.mark.parametrize("name", G9_NAMES)
def test_g9_ablation_variants_forward_and_gradients(name):
    """The reference's other embeddings / decoders (carca.py:98-198,352-399) on the HIP path:
    eval scores, train-mode scores, loss and every parameter gradient against the fixtures made from the reference."""
    from carca_replication_amd import modules as M

    fx = load("g9_" + name)
    model = model_from_fixture(fx)
    model.eval()
    with torch.no_grad():
        y = model(profile=tuple(fx.ins[k].cuda() for k in ("p_x", "p_a", "p_c")),
                  targets=[tuple(fx.ins[k].cuda() for k in ("o_x", "o_a", "o_c"))])
    assert y.shape == fx.outs["y"].shape
    assert float((y.cpu() - fx.outs["y"]).abs().max()) < 2e-5
    loss = M.BinaryCrossEntropy()(y, fx.ins["y_true"].cuda(), M.get_mask(fx.ins["o_x"].cuda()))
    ref = float(fx.outs["loss"])
    assert abs(float(loss) - ref) < 2e-5 * max(1.0, abs(ref))
    y, loss = _step(model, fx, "train/")
    assert float((y.detach().cpu() - fx.outs["train/y"]).abs().max()) < 2e-5
    ref = float(fx.outs["train/loss"])
    assert abs(float(loss) - ref) < 2e-5 * max(1.0, abs(ref))
    _check_grads(model, {k[len("train/grad/"):]: v for k, v in fx.outs.items() if k.startswith("train/grad/")})


def test_g3_three_adam_steps():
    """torch.optim.Adam on the HIP gradients reproduces the reference's 3-step trajectory (training.py:174)."""
    fx = load("g3_adam")
    model = model_from_fixture(fx)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=0.0, betas=(0.9, 0.98))
    for step in range(3):
        _, loss = _step(model, fx)
        # weight gradients are combined with fp32 atomics (order varies run to run) and Adam's first steps are
        # sign-like, so the trajectory is reproduced to ~1e-6 typically and 2e-5 in the worst run seen
        assert abs(float(loss) - float(fx.outs[f"loss{step}"])) < 2e-5
        opt.step()
    for k, v in model.state_dict().items():
        if k.endswith("WK.bias"):  # true gradient is 0: Adam turns round-off into +-lr steps
            continue
        # Entries whose true gradient is ~0 get +-lr steps from round-off through Adam's normalisation (3 steps x 1e-3):
        # require the bulk to match tightly and no entry to move by more than a fraction of that range.
        diff = (v.cpu() - fx.outs["final/" + k]).abs()
        assert float(diff.max()) < 5e-4, k
        assert float((diff > 2e-5).float().mean()) < 2e-3, k


def test_gradients_vs_oracle_autograd_c2_like():
    """Bigger than the fixtures: d=90 H=3 g=450, n_attrs=300, B=9 users, L=50."""
    cfg = O.CarcaConfig(d=90, H=3, n_blocks=2)
    n_items, n_attrs, n_ctx, g, L, B = 400, 300, 6, 450, 50, 9
    P = O.perturb_params(O.init_params(cfg, n_items, g, n_ctx, n_attrs, L, seed=0), seed=1)
    profile, pos, _ = O.synth_eval_batch(B, L, L, n_items, n_attrs, n_ctx, seed=3, min_len=1)
    neg = (pos[0].flip(1).contiguous(), pos[1].flip(1).contiguous(), pos[2])
    px = profile[0]
    pos = (pos[0] * (px != 0), pos[1], pos[2])  # targets padded where the profile is (data.py:112-132)
    neg = (neg[0] * (px != 0), neg[1], neg[2])
    y_true = torch.cat([(px != 0).int(), torch.zeros_like(px)], dim=1)
    o_x = torch.cat([pos[0], neg[0]], dim=1)
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    y = O.carca_forward(Pg, cfg, profile, [pos, neg], training=True)
    loss = O.bce_loss(y, y_true, O.get_mask(o_x))
    loss.backward()
    from carca_replication_amd import modules as M

    model = model_from_params(P, cfg).train()
    yg = model(profile=dev(profile), targets=[dev(pos), dev(neg)])
    lg = M.BinaryCrossEntropy()(yg, y_true.cuda(), M.get_mask(o_x.cuda()))
    lg.backward()
    assert abs(float(lg) - float(loss)) < 2e-6
    _check_grads(model, {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in Pg.items()})


def test_engine_train_step_and_eval_batch():
    """engine.train_step == the reference's loop body (train.py:84-96); eval_batch == train.py:42-51."""
    from carca_replication_amd import engine

    fx = load("g3_adam")
    model = model_from_fixture(fx).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=0.0, betas=(0.9, 0.98))
    batch = tuple(fx.ins[k].cuda() for k in ("p_x", "p_a", "p_c", "o_x", "o_a", "o_c", "y_true"))
    for step in range(3):
        loss = engine.train_step(model, opt, batch)
        assert abs(float(loss) - float(fx.outs[f"loss{step}"])) < 2e-5
    fx8 = load("g8_ranking")
    m8 = model_from_fixture(fx8).eval()
    batch = tuple(fx8.ins[k].cuda() for k in ("p_x", "p_a", "p_c", "o_x", "o_a", "o_c", "y_true"))
    y, sums = engine.eval_batch(m8, batch, k=10)
    sums = sums.cpu()
    assert float(sums[0]) == float(fx8.outs["hr10"]) and abs(float(sums[1]) - float(fx8.outs["ndcg10"])) < 1e-4
    assert float(sums[2]) == 0.0 and float(sums[4]) == 64.0


@pytest.mark.parametrize("name", ["d90h3", "d128h4"])
def test_folded_training_path_matches_reference_gradients(name):
    """CARCA.fold_embedding(True, training=True): the re-associated embedding (no F -> g product in either direction)
    gives the reference's outputs and gradients -- same tolerances as the plain path -- and stays close to it."""
    fx = load("g2_" + name)
    model = model_from_fixture(fx)
    y0, loss0 = _step(model, fx)
    plain = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    model.fold_embedding(True, training=True)
    y, loss = _step(model, fx)
    assert float((y.detach().cpu() - fx.outs["y"]).abs().max()) < 2e-5
    assert abs(float(loss) - float(fx.outs["loss"])) < 2e-6
    _check_grads(model, {k[len("grad/"):]: v for k, v in fx.outs.items() if k.startswith("grad/")})
    for n, p in model.named_parameters():
        scale = float(plain[n].abs().max()) + 1e-12
        assert float((p.grad - plain[n]).abs().max()) <= 2e-5 * scale + 1e-7, n
    model.fold_embedding(False)
    y1, _ = _step(model, fx)
    assert torch.equal(y1, y0)  # and switching it off restores the plain path exactly


def test_c2_full_batch_gradients_are_the_weighted_sum_of_its_halves():
    """The bench's train workload at full size (C2: B = 128, n_attrs = 4096: persistent one-block-per-CU weight-gradient
    kernel, grouped small products) through a size-independent property: the loss is a mean over unmasked targets
    (carca.py:443), so loss and every gradient of a batch are the mask-count-weighted means of those of its two halves
    -- which run the B = 64 kernel choices (two workgroups per user, other row splits)."""
    from carca_replication_amd import engine
    from carca_replication_amd.synth import eval_batch
    from tests.model_util import build_model

    B, L, d, g, H, n_items, n_attrs, n_ctx = 128, 50, 90, 450, 3, 12102, 4096, 6
    torch.manual_seed(0)
    model = build_model(dict(d=d, H=H, n_blocks=2, encoding="learnable"), n_items, g, n_ctx, n_attrs, L).cuda().train()
    profile, pos, _ = eval_batch(B, L, L, n_items, n_attrs, n_ctx, seed=77)
    px = profile[0]
    o_x = torch.cat([pos[0] * (px != 0), pos[0].flip(1) * (px != 0)], dim=1)
    o_a = torch.cat([pos[1], pos[1].flip(1)], dim=1)
    o_c = torch.cat([pos[2], pos[2]], dim=1)
    y_true = torch.cat([(px != 0).int(), torch.zeros_like(px)], dim=1)
    batch = tuple(t.cuda() for t in (profile[0], profile[1], profile[2], o_x, o_a, o_c, y_true))
    opt = torch.optim.SGD(model.parameters(), lr=0.0)

    def run(lo, hi):
        sub = tuple(t[lo:hi].contiguous() for t in batch)
        loss = engine._forward_backward(model, opt, sub, None)
        n = float((sub[3] != 0).sum())
        return float(loss), n, {k: p.grad.detach().clone() for k, p in model.named_parameters()}

    lf, nf, gf = run(0, B)
    l1, n1, g1 = run(0, B // 2)
    l2, n2, g2 = run(B // 2, B)
    assert nf == n1 + n2
    assert lf == pytest.approx((n1 * l1 + n2 * l2) / nf, rel=1e-5)
    for k in gf:
        want = (n1 * g1[k] + n2 * g2[k]) / nf
        assert float((gf[k] - want).abs().max()) <= 1e-4 * float(want.abs().max()) + 1e-7, k


def test_c2_full_batch_train_step_against_oracle_autograd():
    """The bench's train workload at FULL size -- B = 128, L = 50, n_attrs = 4096, n_items = 12,102, d = 90 / g = 450 / H = 3
    (the compacting feature GEMM over the kept rows, the compacted feats_embed weight gradient, the grouped small products)
    -- loss and EVERY parameter gradient against torch.autograd over the CPU oracle on the same batch: once
    through the eager pass and once replayed from the captured two-stream graph (lr = 0, so the weights stay put)."""
    from carca_replication_amd import engine
    from carca_replication_amd.optim import Adam

    cfg = O.CarcaConfig(d=90, H=3, n_blocks=2)
    n_items, n_attrs, n_ctx, g, L, B = 12102, 4096, 6, 450, 50, 128
    P = O.perturb_params(O.init_params(cfg, n_items, g, n_ctx, n_attrs, L, seed=0), seed=1)
    profile, pos, _ = O.synth_eval_batch(B, L, L, n_items, n_attrs, n_ctx, seed=1234)
    px = profile[0]
    neg = (pos[0].flip(1).contiguous(), pos[1].flip(1).contiguous(), pos[2])
    pos = (pos[0] * (px != 0), pos[1], pos[2])  # targets padded where the profile is (data.py:112-132)
    neg = (neg[0] * (px != 0), neg[1], neg[2])
    y_true = torch.cat([(px != 0).int(), torch.zeros_like(px)], dim=1)
    o_x = torch.cat([pos[0], neg[0]], dim=1)
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    y = O.carca_forward(Pg, cfg, profile, [pos, neg], training=True)
    loss = O.bce_loss(y, y_true, O.get_mask(o_x))
    loss.backward()
    ref = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in Pg.items()}

    model = model_from_params(P, cfg).train()
    batch = tuple(t.cuda() for t in (profile[0], profile[1], profile[2], o_x, torch.cat([pos[1], neg[1]], dim=1),
                                     torch.cat([pos[2], neg[2]], dim=1), y_true))
    opt = Adam(model.parameters(), lr=0.0, betas=(0.9, 0.98))
    lg = engine._forward_backward(model, opt, batch, None)
    assert abs(float(lg) - float(loss)) < 2e-6
    _check_grads(model, ref)
    step = engine.GraphedTrainStep(model, opt, batch)
    try:
        for _ in range(2):
            lr_ = step(batch)
            assert abs(float(lr_) - float(loss)) < 2e-6
            _check_grads(model, ref)
    finally:
        step.close()


@pytest.mark.parametrize("n_groups", [2, 3])
def test_two_stream_embedding_backward_agrees_with_the_single_stream_pass(n_groups, monkeypatch):
    """The backward pass hands the target rows' embedding backward to a second stream once the decoder's backward has
    produced their d e (autograd._SideEmbed): same gradients as the single-stream pass (fp32 summation order aside), with
    the balance slice (SPLIT_MAIN_TARGET_USERS) on and off, and at CARCA_MAX_SEGS segments (profile + 3 target groups:
    no room for the slice).  As shipped the split is taken while a hipGraph is captured: tests/test_hip_graph.py replays
    it against the eager single-stream step; the test below forces it on the reference's G2 gradients."""
    from carca_replication_amd import autograd, engine
    from carca_replication_amd import modules as M
    from carca_replication_amd.synth import eval_batch
    from tests.model_util import build_model

    B, L, d, g, H, n_items, n_attrs, n_ctx = 128, 50, 90, 450, 3, 12102, 512, 6
    torch.manual_seed(0)
    model = build_model(dict(d=d, H=H, n_blocks=2, encoding="learnable"), n_items, g, n_ctx, n_attrs, L).cuda().train()
    profile, pos, _ = eval_batch(B, L, L, n_items, n_attrs, n_ctx, seed=78)
    profile = tuple(t.cuda() for t in profile)
    px = profile[0]
    groups = [tuple(t.cuda() for t in (pos[0] * (px.cpu() != 0), pos[1], pos[2]))]
    for k in range(1, n_groups):
        groups.append(tuple(t.cuda() for t in (pos[0].roll(k, 0) * (px.cpu() != 0), pos[1].roll(k, 0), pos[2])))
    y_true = torch.cat([(px != 0).int()] + [torch.zeros_like(px)] * (n_groups - 1), dim=1)

    def run(split, frac):
        monkeypatch.setattr(autograd, "SPLIT_EMBED_BWD", split)
        monkeypatch.setattr(autograd, "SPLIT_MAIN_TARGET_USERS", frac)
        model.zero_grad(set_to_none=True)
        y = model(profile=profile, targets=groups)  # (the groups' scores: modules.JointScores)
        loss = M.BinaryCrossEntropy()(y, y_true, M.get_mask(torch.cat([grp[0] for grp in groups], dim=1)))
        loss.backward()
        torch.cuda.synchronize()
        return float(loss), {k: p.grad.detach().clone() for k, p in model.named_parameters()}

    l0, g0 = run(False, 0.0)
    for frac in (0.0, 0.3):
        l1, g1 = run(True, frac)
        assert l1 == l0
        for k in g0:
            assert float((g1[k] - g0[k]).abs().max()) <= 2e-5 * float(g0[k].abs().max()) + 1e-7, (k, frac)
    assert any(float(v.abs().max()) > 0 for k, v in g0.items() if "feats_embed" in k)


@pytest.mark.parametrize("rows,d,ld,out_ld", [(6400, 90, 96, 96), (6401, 128, 128, 128), (333, 50, 64, 64),
                                              (77, 6, 8, 8), (129, 90, 91, 96), (64, 128, 256, 128),
                                              (130, 192, 192, 192), (77, 300, 301, 304), (9, 1024, 1024, 1024),
                                              (16, 961, 961, 961), (7, 1000, 1003, 1024), (4101, 130, 131, 132)])
def test_layernorm_backward_kernels_against_torch(rows, d, ld, out_ld):
    """Both LayerNorm-backward kernels (16-byte row pairs for the padded internal strides, one row per wave otherwise)
    against torch.autograd of nn.LayerNorm (carca.py:421 / 440, eps 1e-5), with the fused addend and pad columns.
    (4101 rows of 130: above the wide kernel's 256 blocks x 16 rows, so its stride loop runs.)"""
    from carca_replication_amd import ops
    torch.manual_seed(rows + d)
    xs = torch.randn(rows, ld, device="cuda") * 2 + 0.5
    dys = torch.randn(rows, ld, device="cuda")
    add = torch.randn(rows, ld, device="cuda")
    gamma = torch.randn(d, device="cuda")
    dg, db = torch.zeros(d, device="cuda"), torch.zeros(d, device="cuda")
    dx = ops.layernorm_bwd(dys, xs, gamma, d, out_ld, addend=add, dgamma=dg, dbeta=db)
    xr = xs[:, :d].double().requires_grad_(True)
    gr = gamma.double().requires_grad_(True)
    br = torch.zeros(d, dtype=torch.float64, device="cuda", requires_grad=True)
    torch.nn.functional.layer_norm(xr, (d,), gr, br, 1e-5).backward(dys[:, :d].double())
    assert torch.allclose(dx[:, :d].double(), xr.grad + add[:, :d].double(), rtol=1e-4, atol=1e-5)
    assert torch.equal(dx[:, d:], torch.zeros_like(dx[:, d:]))
    assert torch.allclose(dg.double(), gr.grad, rtol=1e-4, atol=1e-4 * float(gr.grad.abs().max()))
    assert torch.allclose(db.double(), br.grad, rtol=1e-4, atol=1e-4 * float(br.grad.abs().max()))
    dx2 = ops.layernorm_bwd(dys, xs, gamma, d, out_ld)  # no addend, no parameter gradients
    assert torch.allclose(dx2[:, :d].double(), xr.grad, rtol=1e-4, atol=1e-5)
