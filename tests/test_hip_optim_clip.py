"""Clipping by global gradient norm inside the one-launch optimizer (Adam(max_grad_norm=...)), the
decoupled-decay variant optim.AdamW, and optim.global_grad_norm: against float64, against torch.nn.utils.clip_grad_norm_
followed by torch's optimizers, and bit for bit against this optimizer's own unclipped / dense / eager paths."""
import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1,), (3, 5), (1024,), (1025,), (90, 540), (7, 1, 13), (300000,)]  # (test_adam_matches_torch's)
LR, BETAS, EPS = 1e-3, (0.9, 0.98), 1e-8


def _params_with_grads(shapes, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in shapes]
    for p in ps:
        p.grad = (torch.randn(p.shape, generator=g) * scale).cuda()
    return ps


def _norm64(grads):
    return math.sqrt(sum(float((g.detach().double().cpu() ** 2).sum()) for g in grads))


NORM_CASES = {
    **{f"shape{'x'.join(map(str, s))}": [s] for s in SHAPES + [(1023,)]},
    "all_shapes": SHAPES + [(1023,)],
    "fifty_tensors_two_launches": [(17,)] * 50,
}


@pytest.mark.parametrize("case", sorted(NORM_CASES))
def test_global_grad_norm_against_float64(case):
    """global_grad_norm within 2e-6 relative of the float64 norm of the same fp32 gradients, and the same bits on a
    second call.  The bound: every term is >= 0 (no cancellation).  Within a chunk a sum passes through at most
    4 roundings in the thread (one product and three fused multiply-adds: <= 1 + 3), 6 in the wave butterfly and 3 over
    the four wave sums = 13 fp32 roundings, < 13 * 2^-24 = 7.8e-7 relative on the sum of squares and half that, < 4e-7,
    on the norm; the double-precision finish and the cast to fp32 add < 1e-7.  2e-6 leaves ~4x margin."""
    from carca_replication_amd.optim import global_grad_norm

    ps = _params_with_grads(NORM_CASES[case], 21, scale=3.0)
    want = _norm64([p.grad for p in ps])
    got = global_grad_norm(ps)
    again = global_grad_norm(ps)
    assert got.is_cuda and got.dim() == 0 and got.dtype == torch.float32
    assert torch.equal(got, again)
    print(case, "norm", float(got), "float64", want, "rel", abs(float(got) - want) / want)
    assert abs(float(got) - want) <= 2e-6 * want


def test_global_grad_norm_of_a_misaligned_gradient():
    """A contiguous 1025-element gradient that starts one float into its buffer: no 16-byte load may touch it."""
    from carca_replication_amd.optim import global_grad_norm

    buf = torch.randn(1030, generator=torch.Generator().manual_seed(22)).cuda()
    p = torch.nn.Parameter(torch.zeros(1025, device="cuda"))
    p.grad = buf[1:1026]
    assert p.grad.data_ptr() % 16 == 4 and p.grad.is_contiguous()
    want = _norm64([p.grad])
    got = global_grad_norm([p])
    assert torch.equal(got, global_grad_norm([p]))
    assert abs(float(got) - want) <= 2e-6 * want


@pytest.mark.parametrize("row_len", [90, 128])
def test_masked_norm_equals_the_dense_norm(row_len):
    """A row mask only keeps rows whose gradient is exactly 0 from being read: adding 0.0 is exact, and which elements a
    thread adds does not depend on the mask, so the norm over a masked table has the bits of the norm without the mask."""
    from carca_replication_amd import _lib
    from carca_replication_amd.ops import _stream

    gen = torch.Generator().manual_seed(23)
    rows = torch.randperm(512, generator=gen)[:200]
    grad = torch.zeros(512, row_len)
    grad[rows] = torch.randn(200, row_len, generator=gen)
    grad = grad.cuda()
    mask = torch.zeros(512, dtype=torch.uint8)
    mask[rows] = 1
    mask = mask.cuda()
    lib = _lib.load()
    outs = []
    for with_mask in (True, False):
        arr = (_lib.AdamTensor * 1)()
        arr[0].g, arr[0].n = grad.data_ptr(), grad.numel()
        if with_mask:
            arr[0].row_mask, arr[0].row_len = mask.data_ptr(), row_len
        chunks = (grad.numel() + 1023) // 1024
        partials = torch.full((chunks,), float("nan"), device="cuda")
        out = torch.full((2,), float("nan"), device="cuda")
        _lib.check(lib.carca_grad_norm(arr, 1, 2.0, partials.data_ptr(), chunks, out.data_ptr(), _stream()), "grad_norm")
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    want = _norm64([grad])
    assert abs(float(outs[0][0]) - want) <= 2e-6 * want
    assert float(outs[0][1]) == pytest.approx(2.0 / want, rel=1e-5) and want > 2.0


def test_grad_norm_rejects_bad_arguments():
    from carca_replication_amd import _lib
    from carca_replication_amd.ops import CarcaHipError, _stream

    lib = _lib.load()
    g = torch.ones(2049, device="cuda")
    arr = (_lib.AdamTensor * 1)()
    arr[0].g, arr[0].n = g.data_ptr(), g.numel()
    partials, out = torch.zeros(3, device="cuda"), torch.zeros(2, device="cuda")
    for args in ((1.0, None, 3, out.data_ptr()), (1.0, partials.data_ptr(), 3, None), (0.0, partials.data_ptr(), 3, out.data_ptr()),
                 (-1.0, partials.data_ptr(), 3, out.data_ptr()), (1.0, partials.data_ptr(), 2, out.data_ptr())):
        with pytest.raises(CarcaHipError):
            _lib.check(lib.carca_grad_norm(arr, 1, args[0], args[1], args[2], args[3], _stream()), "grad_norm")
    _lib.check(lib.carca_grad_norm(arr, 1, 1.0, partials.data_ptr(), 3, out.data_ptr(), _stream()), "grad_norm")
    assert float(out[0]) == pytest.approx(math.sqrt(2049.0), rel=2e-6)


# ---- trajectories against torch and float64 ------------------------------------------------------------------------------
def _f64_step(kind, wd, p, g, m, v, t, max_norm):
    """clip_grad_norm_ then torch.optim.Adam / AdamW, restated in float64 on the CPU (lists of tensors, in place)."""
    norm = math.sqrt(sum(float((x * x).sum()) for x in g))
    scale = min(1.0, max_norm / (norm + 1e-6))
    b1, b2 = BETAS
    for i in range(len(p)):
        gi = g[i] * scale
        if kind == "adamw":
            p[i] *= 1.0 - LR * wd
        else:
            gi = gi + wd * p[i]
        m[i] += (1.0 - b1) * (gi - m[i])
        v[i].mul_(b2).add_((1.0 - b2) * gi * gi)
        p[i] -= (LR / (1.0 - b1 ** t)) * m[i] / (v[i].sqrt() / math.sqrt(1.0 - b2 ** t) + EPS)
    return norm


def _make(kind, params, wd, max_grad_norm=None, ours=True):
    from carca_replication_amd.optim import Adam, AdamW

    if ours:
        cls = AdamW if kind == "adamw" else Adam
        return cls(params, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, max_grad_norm=max_grad_norm)
    cls = torch.optim.AdamW if kind == "adamw" else torch.optim.Adam
    return cls(params, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd)


@pytest.mark.parametrize("kind,wd", [("adam", 0.0), ("adam", 0.01), ("adamw", 0.01)])
def test_clipped_trajectories_match_torch(kind, wd):
    """max_grad_norm = 1000 against clip_grad_norm_(params, 1000) + torch's optimizer over test_adam_matches_torch's tensors
    and gradients (349,641 elements, norms from 59 to 3020: the first two steps are not clipped, the other four are).  Parameters within
    that test's 2e-6 * (step + 1); moments at most 2x as far from a float64 restatement as torch's own fp32 result on the
    same tensor, plus that test's atol (both are fp32 evaluations of one formula that differ in rounding order)."""
    max_norm = 1000.0
    gen = torch.Generator().manual_seed(3)
    init = [torch.randn(s, generator=gen) for s in SHAPES]
    a = [torch.nn.Parameter(x.clone().cuda()) for x in init]
    b = [torch.nn.Parameter(x.clone().cuda()) for x in init]
    p64 = [x.double() for x in init]
    m64 = [torch.zeros_like(x) for x in p64]
    v64 = [torch.zeros_like(x) for x in p64]
    ours = _make(kind, a, wd, max_grad_norm=max_norm)
    ref = _make(kind, b, wd, ours=False)
    assert ours.last_grad_norm is None
    g = torch.Generator().manual_seed(4)
    norms = []
    for step in range(6):
        grads = [torch.randn(p.shape, generator=g) * (0.1 + step) for p in a]
        for p, q, grad in zip(a, b, grads):
            p.grad, q.grad = grad.cuda(), grad.cuda()
        kept = [p.grad.clone() for p in a]
        ours.step()
        torch.nn.utils.clip_grad_norm_(b, max_norm)
        ref.step()
        norm64 = _f64_step(kind, wd, p64, [x.double() for x in grads], m64, v64, step + 1, max_norm)
        norms.append(float(ours.last_grad_norm))
        assert abs(norms[-1] - norm64) <= 2e-6 * norm64  # (the bound of test_global_grad_norm_against_float64)
        for p, q, k in zip(a, b, kept):
            assert torch.equal(p.grad, k)  # (the documented difference from torch: p.grad is left unscaled)
            assert float((p - q).abs().max()) <= 2e-6 * (step + 1), (step, tuple(p.shape))
    print(kind, wd, "norms", norms)
    assert any(n < max_norm for n in norms) and any(n > max_norm for n in norms), norms
    for p, q, m, v in zip(a, b, m64, v64):
        so, sr = ours.state[p], ref.state[q]
        assert float(so["step"]) == float(sr["step"]) == 6
        for key, want, atol in (("exp_avg", m, 2e-6), ("exp_avg_sq", v, 1e-7)):
            d_ours = float((so[key].double().cpu() - want).abs().max())
            d_ref = float((sr[key].double().cpu() - want).abs().max())
            print(kind, wd, tuple(p.shape), key, "ours", d_ours, "torch", d_ref)
            assert d_ours <= 2 * d_ref + atol, (key, tuple(p.shape), d_ours, d_ref)


@pytest.mark.parametrize("kind,wd", [("adam", 0.0), ("adam", 0.01), ("adamw", 0.01)])
def test_inactive_clip_is_the_identity(kind, wd):
    """max_grad_norm = 1e30 never clips: scale = 1.0f and g * 1.0f = g, so every tensor and every state entry has the
    bits of max_grad_norm = None -- on each of the kernel's four paths: full aligned chunks and ragged tails of dense
    tensors, and touched-row tables with rows on and off the 16-byte grid.  (Three parameter groups: the one norm is over
    all of them; the tables' group has no decay, which a row mask requires.)"""
    shapes = [(3, 5), (1025,), (90, 540), (4100,), (64, 128), (64, 90)]
    gen = torch.Generator().manual_seed(31)
    init = [torch.randn(s, generator=gen).cuda() for s in shapes]
    ids = torch.arange(1, 64, 3, dtype=torch.int32).cuda()
    runs = []
    for max_norm in (1e30, None):
        ps = [torch.nn.Parameter(x.clone()) for x in init]
        opt = _make(kind, [dict(params=ps[:2]), dict(params=ps[2:4], lr=2e-3), dict(params=ps[4:], weight_decay=0.0)], wd,
                    max_grad_norm=max_norm)
        g = torch.Generator().manual_seed(32)
        for step in range(3):
            for p in ps:
                p.grad = (torch.randn(p.shape, generator=g) * (1 + step)).cuda()
            for table in ps[4:]:
                keep = torch.zeros_like(table.grad)
                keep[ids.long()] = table.grad[ids.long()]
                table.grad = keep
                assert opt.mark_rows(table, ids)
            opt.step()
        runs.append((ps, opt))
    (pa, oa), (pb, ob) = runs
    assert float(oa.last_grad_norm) > 0 and ob.last_grad_norm is None
    assert "row_touched" in oa.state[pa[4]] and "row_touched" in ob.state[pb[5]]
    for p, q, x in zip(pa, pb, init):
        assert torch.equal(p, q) and not torch.equal(p, x)
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(oa.state[p][key], ob.state[q][key])
        assert float(oa.state[p]["step"]) == float(ob.state[q]["step"]) == 3


def test_adamw_matches_torch_without_clipping():
    """optim.AdamW alone (no clip) against torch.optim.AdamW: test_adam_matches_torch's bound."""
    gen = torch.Generator().manual_seed(3)
    init = [torch.randn(s, generator=gen).cuda() for s in SHAPES]
    a = [torch.nn.Parameter(x.clone()) for x in init]
    b = [torch.nn.Parameter(x.clone()) for x in init]
    ours, ref = _make("adamw", a, 0.05), _make("adamw", b, 0.05, ours=False)
    g = torch.Generator().manual_seed(4)
    for step in range(6):
        for p, q in zip(a, b):
            grad = (torch.randn(p.shape, generator=g) * (0.1 + step)).cuda()
            p.grad, q.grad = grad.clone(), grad.clone()
        ours.step()
        ref.step()
        for p, q in zip(a, b):
            assert float((p - q).abs().max()) <= 2e-6 * (step + 1), (step, tuple(p.shape))
    for p, q in zip(a, b):
        assert torch.allclose(ours.state[p]["exp_avg"], ref.state[q]["exp_avg"], rtol=1e-5, atol=2e-6)
        assert torch.allclose(ours.state[p]["exp_avg_sq"], ref.state[q]["exp_avg_sq"], rtol=1e-5, atol=1e-7)


def test_touched_row_adam_stays_bit_exact_under_clipping():
    """test_touched_row_adam_is_bit_exact with the clip active: the masked table's norm has the dense norm's bits, so
    both runs step with the same factor and stay equal in every bit -- parameters, exp_avg and exp_avg_sq."""
    from carca_replication_amd.optim import Adam

    n_rows, dim, steps = 4096, 64, 3
    gen = torch.Generator().manual_seed(41)
    w0 = torch.randn(n_rows, dim, generator=gen).cuda()
    small0 = [torch.randn(33, 7, generator=gen).cuda(), torch.randn(1025, generator=gen).cuda()]
    tabs = [torch.nn.Parameter(w0.clone()) for _ in range(2)]
    smalls = [[torch.nn.Parameter(x.clone()) for x in small0] for _ in range(2)]
    masked = Adam([tabs[0]] + smalls[0], lr=LR, betas=BETAS, max_grad_norm=0.5)
    dense = Adam([tabs[1]] + smalls[1], lr=LR, betas=BETAS, max_grad_norm=0.5)
    touched = torch.zeros(n_rows, dtype=torch.bool, device="cuda")
    for step in range(steps):
        ids = torch.randint(1, n_rows, (8, 40), generator=gen).to(torch.int32).cuda()
        grad = torch.zeros(n_rows, dim, device="cuda")
        grad.index_add_(0, ids.reshape(-1).long(), torch.randn(ids.numel(), dim, generator=gen).cuda())
        gs = [torch.randn(x.shape, generator=gen).cuda() for x in small0]
        touched[ids.reshape(-1).long()] = True
        for t, ss in zip(tabs, smalls):
            t.grad = grad.clone()
            for s_, g_ in zip(ss, gs):
                s_.grad = g_.clone()
        assert masked.mark_rows(tabs[0], ids)
        masked.step()
        dense.step()
        assert torch.equal(masked.last_grad_norm, dense.last_grad_norm) and float(masked.last_grad_norm) > 0.5
    sm, sd = masked.state[tabs[0]], dense.state[tabs[1]]
    assert "row_touched" in sm and "row_touched" not in sd
    assert 0 < int(touched.sum()) < n_rows // 2 and torch.equal(sm["row_touched"].bool(), touched)
    assert torch.equal(tabs[0], tabs[1])
    assert torch.equal(sm["exp_avg"], sd["exp_avg"]) and torch.equal(sm["exp_avg_sq"], sd["exp_avg_sq"])
    for a, b in zip(smalls[0], smalls[1]):
        assert torch.equal(a, b)
        assert torch.equal(masked.state[a]["exp_avg"], dense.state[b]["exp_avg"])
    assert torch.equal(tabs[0][~touched], w0[~touched]) and not torch.equal(tabs[0], w0)
    # weight decay of either style would move untouched rows: refused
    from carca_replication_amd.optim import AdamW

    assert AdamW([tabs[0]], lr=LR).mark_rows(tabs[0], ids) is False


def test_adamw_state_dict_interchangeable_with_torch():
    """test_adam_state_dict_interchangeable_with_torch for AdamW, with the clip on: ours -> torch.optim.AdamW and back,
    the next step agreeing within the trajectory test's bounds; max_grad_norm travels in param_groups."""
    from carca_replication_amd.optim import AdamW

    shapes = [(17, 9), (130,)]
    gen = torch.Generator().manual_seed(5)
    init = [torch.randn(s, generator=gen).cuda() for s in shapes]
    a = [torch.nn.Parameter(x.clone()) for x in init]
    b = [torch.nn.Parameter(x.clone()) for x in init]
    ours = AdamW(a, lr=2e-3, betas=BETAS, weight_decay=0.02, max_grad_norm=3.0)
    for _ in range(2):
        for p in a:
            p.grad = torch.ones_like(p)
        ours.step()
    sd = ours.state_dict()
    assert all(g["max_grad_norm"] == 3.0 for g in sd["param_groups"])
    ref = torch.optim.AdamW(b, lr=1e-1)
    ref.load_state_dict(copy.deepcopy(sd))  # ours -> torch (hyper-parameters travel with the groups)
    assert ref.param_groups[0]["lr"] == 2e-3 and ref.param_groups[0]["weight_decay"] == 0.02
    for p, q in zip(a, b):
        q.data.copy_(p.data)
        p.grad = torch.full_like(p, 0.5)
        q.grad = torch.full_like(q, 0.5)
    ours.step()
    torch.nn.utils.clip_grad_norm_(b, 3.0)
    ref.step()
    norm = math.sqrt(0.25 * (17 * 9 + 130))
    assert abs(float(ours.last_grad_norm) - norm) <= 2e-6 * norm and norm > 3.0
    for p, q in zip(a, b):
        assert float((p - q).abs().max()) <= 2e-6
    a2 = [torch.nn.Parameter(x.clone()) for x in init]
    back = AdamW(a2, lr=1e-1, max_grad_norm=3.0)
    back.load_state_dict(copy.deepcopy(ref.state_dict()))  # torch -> ours: step counts and hyper-parameters carry over
    assert back.param_groups[0]["max_grad_norm"] == 3.0 and back.param_groups[0]["lr"] == 2e-3
    for p2, q in zip(a2, b):
        p2.data.copy_(q.data)
        p2.grad = torch.full_like(p2, -0.25)
        q.grad = torch.full_like(q, -0.25)
    back.step()
    torch.nn.utils.clip_grad_norm_(b, 3.0)
    ref.step()
    for p2, q in zip(a2, b):
        assert float(back.state[p2]["step"]) == 4
        assert float((p2 - q).abs().max()) <= 2e-6
        assert torch.allclose(back.state[p2]["exp_avg"], ref.state[q]["exp_avg"], rtol=1e-5, atol=2e-6)
    # ours -> ours: the threshold of the SAVED optimizer wins over the constructor's, like every group entry
    again = AdamW(a2, lr=1e-1, max_grad_norm=7.0)
    again.load_state_dict(copy.deepcopy(sd))
    assert again.param_groups[0]["max_grad_norm"] == 3.0


# ---- through the engine --------------------------------------------------------------------------------------------------
@pytest.fixture
def det():
    from carca_replication_amd import ops

    ops.set_deterministic(True)
    yield
    ops.set_deterministic(False)


MAX_NORM_ENGINE = 1e-3  # (the BCE gradient of this model has a norm of order 0.1-1: every step is clipped, asserted below)


def _engine_setup():
    from carca_replication_amd.optim import AdamW
    from carca_replication_amd.synth import eval_batch
    from tests.model_util import build_model

    d, H, L, B, n_items, n_attrs, n_ctx, g = 64, 2, 16, 8, 300, 40, 6, 64
    torch.manual_seed(7)
    base = build_model(dict(d=d, H=H, n_blocks=1, encoding="learnable"), n_items, g, n_ctx, n_attrs, L).cuda().train()
    profile, pos, _ = eval_batch(B, L, L, n_items, n_attrs, n_ctx, seed=5)
    px = profile[0]
    o_x = torch.cat([pos[0] * (px != 0), pos[0].flip(1) * (px != 0)], dim=1)
    batch = tuple(t.cuda() for t in (profile[0], profile[1], profile[2], o_x, torch.cat([pos[1], pos[1].flip(1)], 1),
                                     torch.cat([pos[2], pos[2]], 1), torch.cat([(px != 0).int(), torch.zeros_like(px)], 1)))

    def fresh():
        m = copy.deepcopy(base)
        return m, AdamW(m.parameters(), lr=1e-3, betas=BETAS, weight_decay=0.01, max_grad_norm=MAX_NORM_ENGINE)

    def rebuilt(model):
        m = build_model(dict(d=d, H=H, n_blocks=1, encoding="learnable"), n_items, g, n_ctx, n_attrs, L).cuda()
        m.load_state_dict(copy.deepcopy(model.state_dict()))
        return m

    return fresh, rebuilt, batch


def _equal_models(model_a, opt_a, model_b, opt_b, what):
    for (n, a), (_, b) in zip(model_a.named_parameters(), model_b.named_parameters()):
        assert torch.equal(a, b), f"{what}: parameter {n}: max |diff| {float((a - b).abs().max())}"
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(opt_a.state[a][key], opt_b.state[b][key]), f"{what}: {key} of {n}"


def test_clipped_step_through_the_engine_eager_graphed_and_repacked(det):
    """A clipped AdamW step driven by engine.train_step and by GraphedTrainStep replays (the optimizer runs behind the
    replay, outside the graph) from the same start, in deterministic mode: every step is clipped, and three of each leave
    the same bits.  The forward after them sees the stepped weights (the packed-weight caches go by the version bump)."""
    from carca_replication_amd import engine

    fresh, rebuilt, batch = _engine_setup()
    other = tuple(t.roll(1, 0) for t in batch)
    model_e, opt_e = fresh()
    model_g, opt_g = fresh()
    step_g = engine.GraphedTrainStep(model_g, opt_g, batch)
    before = [p.detach().clone() for p in model_e.parameters()]
    for bt in (batch, other, batch):
        le = float(engine.train_step(model_e, opt_e, bt))
        norm_e = float(opt_e.last_grad_norm)
        lg = float(step_g(bt))
        assert norm_e > 10 * MAX_NORM_ENGINE and float(opt_g.last_grad_norm) == norm_e and le == lg
    _equal_models(model_e, opt_e, model_g, opt_g, "eager vs graphed")
    assert any(not torch.equal(p, q) for p, q in zip(model_e.parameters(), before))
    step_g.close()
    profile, targets = batch[:3], [tuple(t[:, :16].contiguous() for t in batch[3:6])]
    twin = rebuilt(model_e)
    for mode in (False, True):
        model_e.train(mode)
        twin.train(mode)
        with torch.set_grad_enabled(mode):
            assert torch.equal(model_e(profile=profile, targets=targets), twin(profile=profile, targets=targets))


def test_clipped_sharded_step_equals_the_plain_step(det):
    """The 1-rank sharded step (dist.FORCE_COLLECTIVES: every pointer, view and stream hand-off of the sharded path runs;
    a 1-rank sum is the identity) with the clip on against the plain step: the optimizer sees the reduced flat buffer, the
    norm needs no collective of its own, and the parameters are equal bit for bit."""
    import os
    import socket

    import torch.distributed as dist

    from carca_replication_amd import dist as cdist
    from carca_replication_amd import engine

    fresh, _, batch = _engine_setup()
    other = tuple(t.roll(1, 0) for t in batch)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        model_p, opt_p = fresh()
        model_s, opt_s = fresh()
        for bt in (batch, other, batch):
            cdist.FORCE_COLLECTIVES = True
            cdist.last_reduce = {}
            ls = engine.train_step(model_s, opt_s, bt, sharded=True)
            assert cdist.last_reduce.get("path") == "flat-inplace"
            cdist.FORCE_COLLECTIVES = False
            lp = engine.train_step(model_p, opt_p, bt)
            assert float(ls) == float(lp)
            assert float(opt_s.last_grad_norm) == float(opt_p.last_grad_norm) > 10 * MAX_NORM_ENGINE
        _equal_models(model_s, opt_s, model_p, opt_p, "sharded vs plain")
    finally:
        cdist.FORCE_COLLECTIVES = False
        dist.destroy_process_group()
